// generator.hip — ConvTranspose generator forward + input-gradient (J_G^T) and the posterior
// Langevin loop (sample_langevin_post_z_with_prior, workspace/src/MCMC.py:48-74).
//
// Layout in HBM: every hidden activation is NHWC fp32 (channels contiguous = the GEMM K axis);
// the caller's x / x_hat stay NCHW.  Per step:
//   fwd : PROJ (GEMM z.W, bias+lrelu)  ->  UP2 x n (4-phase implicit GEMM, bias+lrelu)
//         -> SMALLC (to-RGB conv, tanh, residual delta = (x_hat - x)/s^2 * (1 - x_hat^2))
//   bwd : SMALLC dgrad * lrelu'  ->  UP2 dgrad (stride-2 conv implicit GEMM) * lrelu'
//         -> PROJ dgrad (split-K GEMM into slabs)  ->  fused EBM grad + slab sum + z update
// dgrad outputs overwrite the activation they are masked with (same thread reads h, writes dh).
// This file: weight packing, plan / workspace, the hidden layers, the training backward and the C ABI; the SMALLC
// output layer's kernels and the choices among them are smallc.hip (smallc.h).
#include <cstdlib>
#include <mutex>
#include <vector>

#include "gemm.h"
#include "smallc.h"
#include "wgrad.h"

using damc::GemmArgs;
using damc::smallc_ntile;

int damc_launch_posterior_update(const damc_ebm_t* e, float* z, const float* slabs, int nslab, long slab_stride, int B,
                                 int nz, double step, int with_noise, const float* noise, uint64_t seed,
                                 uint64_t step_idx, uint64_t chain_base, float* diag, hipStream_t s,
                                 unsigned short* z3 = nullptr, bool* wrote_z3 = nullptr,
                                 const damc_draw_state_t* ds = nullptr);
bool damc_posterior_update_fusable(const damc_ebm_t* e, int nz);

namespace {

// ------------------------------------------------------------------------------ packing
// PROJ: w (Cin,Cout,k,k) -> fwd [ci][(oy,ox,co)], bwd [(oy,ox,co)][ci]
__global__ void pack_proj_kernel(const float* w, int cin, int cout, int k, float* wf, float* wb) {
  const long n = (long)cin * cout * k * k;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // i enumerates torch layout
  long t = i;
  const int kx = (int)(t % k);
  t /= k;
  const int ky = (int)(t % k);
  t /= k;
  const int co = (int)(t % cout);
  const int ci = (int)(t / cout);
  const long col = ((long)ky * k + kx) * cout + co;
  const float v = w[i];
  wf[(long)ci * ((long)k * k * cout) + col] = v;
  wb[col * cin + ci] = v;
}
// UP2 (k4 s2 p1): fwd [phase(py,px)][ty][tx][ci][co] = W[ci][co][3-py-2ty][3-px-2tx];
//                 bwd [ky][kx][co][ci] = W[ci][co][ky][kx]
// or, for the K-major engine (conv_kmajor_ok of the gathered channel count), the same matrices
// transposed to [n][k]: fwd [phase][co][ty][tx][ci], bwd [ci][ky][kx][co]
__global__ void pack_up2_kernel(const float* w, int cin, int cout, int km_f, int km_b, float* wf, float* wb) {
  const long n = (long)cin * cout * 16;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long t = i;
  const int kx = (int)(t % 4);
  t /= 4;
  const int ky = (int)(t % 4);
  t /= 4;
  const int co = (int)(t % cout);
  const int ci = (int)(t / cout);
  const float v = w[i];
  // ky = 3 - py - 2 ty  ->  py = (3 - ky) & 1, ty = (3 - ky - py) / 2
  const int py = (3 - ky) & 1, ty = (3 - ky - py) >> 1;
  const int px = (3 - kx) & 1, tx = (3 - kx - px) >> 1;
  const int phase = py * 2 + px;
  if (km_f)
    wf[(((long)phase * cout + co) * 4 + ty * 2 + tx) * cin + ci] = v;
  else
    wf[((((long)phase * 2 + ty) * 2 + tx) * cin + ci) * cout + co] = v;
  if (km_b)
    wb[(((long)ci * 4 + ky) * 4 + kx) * cout + co] = v;
  else
    wb[(((long)ky * 4 + kx) * cout + co) * cin + ci] = v;
}
// SMALLC: fwd [ky][kx][ci][co]; bwd (the two-stage projection) [(ky*k+kx)*cout + co][ci] (rows padded
// to a multiple of 32 with zeros by the caller's memset)
__global__ void pack_smallc_kernel(const float* w, int cin, int cout, int k, float* wf, float* wb) {
  const long n = (long)cin * cout * k * k;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long t = i;
  const int kx = (int)(t % k);
  t /= k;
  const int ky = (int)(t % k);
  t /= k;
  const int co = (int)(t % cout);
  const int ci = (int)(t / cout);
  wf[(((long)ky * k + kx) * cin + ci) * cout + co] = w[i];
  if (wb) wb[((long)(ky * k + kx) * cout + co) * cin + ci] = w[i];
}
// LINEAR: w (out,in): fwd = W^T (in,out), bwd = W (out,in)
__global__ void pack_linear_kernel(const float* w, int in, int out, float* wf, float* wb) {
  const long n = (long)in * out;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long o = i / in, c = i - o * in;
  wf[c * out + o] = w[i];
  wb[i] = w[i];
}

// fixed-order (deterministic) reduction of the split-K slabs: one thread per element, loads unrolled
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ slabs, int nslab, long n,
                                                       float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  int k = 0;
  for (; k + 8 <= nslab; k += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = slabs[(long)(k + u) * n + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; k < nslab; ++k) acc += slabs[(long)k * n + i];
  out[i] = acc;
}

// the same sums with 4x the parallelism: a block owns 64 outputs (16 float4) and splits the slabs over 16
// groups of 16 threads; a thread adds slabs g, g+16, g+32, ... in order (loads in flight together), then the
// 16 group sums are added in group order.  Fixed order per element, independent of n (so of the batch split).
__global__ __launch_bounds__(256) void slab_sum4_kernel(const float* __restrict__ slabs, int nslab, long n4,
                                                        float* __restrict__ out) {
  __shared__ f32x4 part[16][16];
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long i4 = (long)blockIdx.x * 16 + q;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (i4 < n4) {
    const f32x4* src = reinterpret_cast<const f32x4*>(slabs) + i4;
#pragma unroll 16
    for (int k = g; k < nslab; k += 16) acc += src[(long)k * n4];
  }
  part[g][q] = acc;
  __syncthreads();
  if (threadIdx.x < 16 && i4 < n4) {
    f32x4 t = part[0][q];
#pragma unroll
    for (int j = 1; j < 16; ++j) t += part[j][q];
    reinterpret_cast<f32x4*>(out)[i4] = t;
  }
}

// p[0 .. n) = 0: the slab slices a shortened split-K never writes (dz_slabs)
__global__ __launch_bounds__(256) void zero_floats_kernel(float* __restrict__ p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

int slab_sum(const float* slabs, int nslab, long n, float* out, hipStream_t s) {
  ProfScope ps("slab_sum", 0.0, s);
  if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(slabs) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    const long n4 = n >> 2;
    hipLaunchKernelGGL(slab_sum4_kernel, dim3((unsigned)((n4 + 15) / 16)), dim3(256), 0, s, slabs, nslab, n4, out);
  } else {
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slabs, nslab, n, out);
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------- plan helpers
long act_floats(const damc_layer_t& L, int B) { return (long)B * L.hout * L.wout * L.cout; }

int validate(const damc_generator_t* g) {
  if (!g || g->n_layers < 1 || g->n_layers > DAMC_MAX_LAYERS) return DAMC_ERR_ARG;
  for (int i = 0; i < g->n_layers; ++i) {
    const damc_layer_t& L = g->layers[i];
    const bool last = i == g->n_layers - 1;
    switch (L.kind) {
      case DAMC_LAYER_PROJ:
        if (i != 0 || L.hin != 1 || L.win != 1 || L.stride != 1 || L.pad != 0 || L.hout != L.k) return DAMC_ERR_ARG;
        break;
      case DAMC_LAYER_UP2:
        if (i == 0 || last || L.k != 4 || L.stride != 2 || L.pad != 1 || L.hout != 2 * L.hin) return DAMC_ERR_ARG;
        break;
      case DAMC_LAYER_SMALLC:
        if (!last || i == 0 || L.cout > 4 || L.act != DAMC_ACT_TANH) return DAMC_ERR_ARG;
        break;
      case DAMC_LAYER_LINEAR:
        if (L.hin != 1 || L.hout != 1) return DAMC_ERR_ARG;
        break;
      default:
        return DAMC_ERR_ARG;
    }
    if (L.engine != DAMC_ENGINE_LIMB && L.engine != DAMC_ENGINE_FP32) return DAMC_ERR_ARG;
    if (i > 0) {
      const damc_layer_t& P = g->layers[i - 1];
      if (P.cout != L.cin || P.hout != L.hin || P.wout != L.win) return DAMC_ERR_ARG;
      if (P.engine != L.engine) return DAMC_ERR_ARG;  // one engine per generator
    }
    if (!last && L.act == DAMC_ACT_TANH) return DAMC_ERR_UNSUPPORTED;
  }
  const damc_layer_t& F = g->layers[g->n_layers - 1];
  if (F.kind == DAMC_LAYER_PROJ || F.kind == DAMC_LAYER_UP2) return DAMC_ERR_UNSUPPORTED;
  if (g->layers[0].cin != g->nz) return DAMC_ERR_ARG;
  return 0;
}

// split-K slices for the PROJ/LINEAR-first-layer dgrad: depends on K only (never on the batch),
// so per-chain results are bitwise identical for any sharding of the batch.
int proj_slices(long K) {
  long s = K / 256;
  if (s < 1) s = 1;
  if (s > 512) s = 512;
  return (int)s;
}
// slice length: a multiple of the K-major engine's K tile (depends on K only, never on the batch)
int proj_k_per(long K, int S) { return (int)(((K + S - 1) / S + 31) / 32 * 32); }

// Limb engine (gemm_x3.hip, fp32-accurate bf16 MFMA) for the UP2 convolutions whose gathered channel
// count is a multiple of 32.  Packed weights and workspaces always carry the x3 copies such a layer
// can use; a descriptor whose layers say engine = DAMC_ENGINE_FP32 routes the launches to the fp32-MFMA
// K-major engine instead.  The choice travels in the descriptor (no process-global state), so two
// streams or threads may use different engines at once.
bool limb(const damc_layer_t& L) { return L.engine == DAMC_ENGINE_LIMB; }
bool x3_fwd_cap(const damc_layer_t& L) {
  return L.kind == DAMC_LAYER_UP2 && L.cin % damc::KM_BK == 0 && L.cout % 8 == 0;
}
bool x3_bwd_cap(const damc_layer_t& L) {
  return L.kind == DAMC_LAYER_UP2 && L.cout % damc::KM_BK == 0 && L.cin % 8 == 0;
}
bool x3_fwd(const damc_layer_t& L) { return limb(L) && x3_fwd_cap(L); }
// first layer z.W as a 1x1 convolution on the limb engine (z split into limbs per call)
bool x3_proj_cap(const damc_layer_t& L) {
  return L.kind == DAMC_LAYER_PROJ && L.cin % damc::KM_BK == 0 && L.cout % 8 == 0;
}
bool x3_proj(const damc_layer_t& L) { return limb(L) && x3_proj_cap(L); }
bool x3_bwd(const damc_layer_t& L) { return limb(L) && x3_bwd_cap(L); }
size_t up2_floats(const damc_layer_t& L) { return (size_t)L.cin * L.cout * 16; }
// the sign block of a UP2 layer's forward (K = 4 Cin per phase) and input-gradient (K = 16 Cout) limb weights
// (damc::x3_conv_negk: by shape, the same for the packing and every launch that reads it)
int up2_negk_fwd(const damc_layer_t& L) { return damc::x3_conv_negk((long)L.hin * L.win, L.cout, 4 * L.cin, 4); }
int up2_negk_bwd(const damc_layer_t& L) { return damc::x3_conv_negk((long)L.hin * L.win, L.cin, 16 * L.cout, 1); }
// x3 copy of a packed weight matrix, stored behind its fp32 packing (n floats, 16-B aligned)
const unsigned short* x3_of(const float* w, size_t n) { return reinterpret_cast<const unsigned short*>(w + n); }

// GemmArgs of a k4 s2 p1 ConvT forward (4 output phases, 2 x 2 taps each) and of its input gradient (a stride-2
// convolution over the output grid): geometry, weights and, on the limb engine, the limb copy with its K order.  The
// Langevin step and the per-op hooks both start from these; a caller adds its operand (A, then a_f32 or A3), its
// outputs (C / C3 / sgn), the mask, split-K slabs and the fused projection.
GemmArgs up2_fwd_args(const damc_layer_t& L, int B) {
  GemmArgs a;
  a.bias = L.bias;
  a.bias_mod = L.cout;
  a.act = L.act;
  a.slope = L.slope;
  a.Hin = L.hin;
  a.Win = L.win;
  a.Cg = L.cin;
  a.Hq = L.hin;
  a.Wq = L.win;
  a.kw = 2;
  a.stride = 1;
  a.B = L.w_fwd;
  a.b_kmajor = damc::conv_kmajor_ok(L.cin);
  a.ldb = a.b_kmajor ? 4L * L.cin : L.cout;
  a.b_zstride = 4L * L.cin * L.cout;
  a.ldc = L.cout;
  a.M = B * L.hin * L.win;
  a.N = L.cout;
  a.K = 4 * L.cin;
  a.Hout = L.hout;
  a.Wout = L.wout;
  if (x3_fwd(L)) {
    a.B3 = x3_of(L.w_fwd, up2_floats(L));
    a.b_negblk = 1;
    a.negk = up2_negk_fwd(L);
    a.kwalk = damc::x3_up2_walk(L.cin);  // the limb copy's K order (damc_pack_generator_layer)
    a.tapshare = 1;
  }
  return a;
}
GemmArgs up2_dgrad_args(const damc_layer_t& L, int B) {
  GemmArgs a;
  a.Hin = L.hout;
  a.Win = L.wout;
  a.Cg = L.cout;
  a.Hq = L.hin;
  a.Wq = L.win;
  a.kw = 4;
  a.stride = 2;
  a.pad_y = 1;
  a.pad_x = 1;
  a.B = L.w_bwd;
  a.b_kmajor = damc::conv_kmajor_ok(L.cout);
  a.ldb = a.b_kmajor ? 16L * L.cout : L.cin;
  a.ldc = L.cin;
  a.M = B * L.hin * L.win;
  a.N = L.cin;
  a.K = 16 * L.cout;
  a.k_per_z = a.K;
  if (x3_bwd(L)) {
    a.B3 = x3_of(L.w_bwd, up2_floats(L));
    a.b_negblk = 1;
    a.negk = up2_negk_bwd(L);
    a.kwalk = damc::x3_up2_walk(L.cout);  // the limb copy's K order (damc_pack_generator_layer)
    a.tapshare = 1;
  }
  return a;
}
// activation j needs an x3 copy when layer j+1 consumes it in the forward pass, or layer j consumes its
// gradient (stored in the same buffer) in the backward pass
bool h_needs_x3(const damc_generator_t* g, int j) {
  return (j + 1 < g->n_layers && x3_fwd_cap(g->layers[j + 1])) || (j >= 1 && x3_bwd_cap(g->layers[j]));
}

// Activation j as sign bits: its producer is a limb-engine epilogue with LReLU, and the kernel that
// masks the next gradient with it (limb dgrad of layer j+1, or the output layer's dgrad) reads bits.
bool hbits_cap(const damc_generator_t* g, int j) {
  if (j + 1 >= g->n_layers) return false;
  const damc_layer_t& L = g->layers[j];
  const damc_layer_t& N = g->layers[j + 1];
  const bool prod = (j == 0) ? x3_proj_cap(L) : x3_fwd_cap(L);
  return prod && L.act == DAMC_ACT_LRELU && (x3_bwd_cap(N) || damc::smallc_dgrad_reads_bits(N));
}
bool hbits(const damc_generator_t* g, int j) { return limb(g->layers[0]) && hbits_cap(g, j); }
// the fp32 activation j is stored unless sign bits carry the mask and the next layer's forward gathers
// limbs (the output layer's forward reads fp32)
bool h_f32(const damc_generator_t* g, int j) {
  return !(hbits(g, j) && j + 1 < g->n_layers && x3_fwd(g->layers[j + 1]));
}

struct Workspace {
  std::vector<float*> h;  // activations (NHWC), one per layer except the final one
  std::vector<unsigned char*> hb;  // sign bits of h (LReLU' masks) or nullptr
  std::vector<unsigned short*> h3;  // x3 limb copies of h (limb engine operands) or nullptr
  unsigned short* z3;               // x3 limbs of z (limb-engine first layer) or nullptr
  float* delta;           // final-layer pre-activation gradient (NHWC / row-major)
  float* slabs;           // split-K partial gradients
  float* glik;            // their fixed-order sum: grad of the likelihood term (B, nz)
  float* pbuf;            // per-tap projections of the output layer (two-stage forward)
  float* kslab;           // split-K slabs of the limb-engine convolutions at small batch (or nullptr)
  long kslab_floats;
  int nslab;
  size_t bytes;
};

size_t carve(const damc_generator_t* g, int B, char* base, Workspace* w) {
  size_t off = 0;
  auto take = [&](long floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += ((size_t)floats * sizeof(float) + 255) / 256 * 256;
    return p;
  };
  if (w) {
    w->h.clear();
    w->h3.clear();
  }
  for (int i = 0; i + 1 < g->n_layers; ++i) {
    float* p = take(act_floats(g->layers[i], B));
    if (w) w->h.push_back(p);
  }
  for (int i = 0; i + 1 < g->n_layers; ++i) {
    unsigned short* p = nullptr;
    if (h_needs_x3(g, i)) p = reinterpret_cast<unsigned short*>(take(act_floats(g->layers[i], B) * 3 / 2));
    if (w) w->h3.push_back(p);
  }
  if (w) w->hb.clear();
  for (int i = 0; i + 1 < g->n_layers; ++i) {
    unsigned char* p = nullptr;
    if (hbits_cap(g, i)) p = reinterpret_cast<unsigned char*>(take(act_floats(g->layers[i], B) / 32 + 4));
    if (w) w->hb.push_back(p);
  }
  const damc_layer_t& F = g->layers[g->n_layers - 1];
  float* d = take(act_floats(F, B));
  const damc_layer_t& L0 = g->layers[0];
  const long K0 = (long)L0.hout * L0.wout * L0.cout;
  const int S = (g->n_layers == 1) ? 1 : proj_slices(K0);
  float* sl = take((long)S * B * g->nz);
  float* gl = take((long)B * g->nz);
  // the output layer's per-tap projections, one buffer per 128-channel chunk of its input (proj16's partials)
  float* pb = (F.kind == DAMC_LAYER_SMALLC)
                  ? take((long)B * F.hin * F.win * smallc_ntile(F) * 32 * ((F.cin + damc::PROJ_CHUNK - 1) / damc::PROJ_CHUNK))
                  : nullptr;
  unsigned short* z3 =
      x3_proj_cap(L0) ? reinterpret_cast<unsigned short*>(take((long)B * g->nz * 3 / 2 + 4)) : nullptr;
  // split-K slabs: the largest any UP2 forward / input gradient of this batch uses (damc::x3_ksplit)
  long ksf = 0;
  for (int i = 0; i < g->n_layers; ++i) {
    const damc_layer_t& L = g->layers[i];
    if (L.kind != DAMC_LAYER_UP2) continue;
    if (x3_fwd_cap(L))
      ksf = std::max(ksf, damc::x3_ksplit_floats(B * L.hin * L.win, L.cout, 4 * L.cin, 4, up2_negk_fwd(L)));
    if (x3_bwd_cap(L))
      ksf = std::max(ksf, damc::x3_ksplit_floats(B * L.hin * L.win, L.cin, 16 * L.cout, 1, up2_negk_bwd(L)));
  }
  float* ks = ksf ? take(ksf) : nullptr;
  if (w) {
    w->kslab = ks;
    w->kslab_floats = ksf;
    w->z3 = z3;
    w->delta = d;
    w->slabs = sl;
    w->glik = gl;
    w->pbuf = pb;
    w->nslab = S;
    w->bytes = off;
  }
  return off;
}

double conv_flops(const damc_layer_t& L, int B) {
  // MACs of the transposed conv = outputs x Cin x (taps hitting each output)
  const double taps = (double)L.k * L.k / ((double)L.stride * L.stride);
  return 2.0 * B * (double)L.hout * L.wout * L.cout * L.cin * taps;
}

// forward of layers [0, n-1) into ws.h; returns 0 on success.  z3_ready: ws.z3 already holds z's limbs (the previous
// posterior update wrote them)
// f32a: limb-engine convolutions gather their input as fp32 (gemm_x3.hip X3_F32A), so every activation is stored fp32
// and no limb copy is written
// proj: the last hidden layer's epilogue also runs the output layer's projection into ws.pbuf (proj_fusable)
int forward_hidden(const damc_generator_t* g, const float* z, int B, Workspace& ws, hipStream_t s,
                   bool z3_ready = false, bool f32a = false, bool proj = false) {
  for (int i = 0; i + 1 < g->n_layers; ++i) {
    const damc_layer_t& L = g->layers[i];
    GemmArgs a;
    a.bias = L.bias;
    a.bias_mod = L.cout;
    a.act = L.act;
    a.slope = L.slope;
    a.C = ws.h[i];
    int rc;
    bool wrote_x3 = false;  // the epilogue already wrote ws.h3[i]
    if (x3_proj(L) && i == 0) {
      // z . W on the limb engine: z -> limbs, 1x1 "convolution" against the x3 copy of the dgrad
      // packing [(oy,ox,co)][ci]; the epilogue writes the next layer's limbs too
      const int N = L.hout * L.wout * L.cout;
      if (!z3_ready) {
        ProfScope ps("split_x3", 0.0, s);
        if ((rc = damc::launch_split_x3(z, (long)B * L.cin, ws.z3, s))) return rc;
      }
      a.A = z;
      a.A3 = ws.z3;
      a.B3 = x3_of(L.w_bwd, (size_t)L.cin * N);
      a.b32k = L.w_bwd;  // the same weights as fp32 rows (the skinny kernel splits them in registers)
      a.b_negblk = 1;
      a.Cg = L.cin;
      a.ldc = N;
      a.M = B;
      a.N = N;
      a.K = L.cin;
      a.k_per_z = a.K;
      if (g->n_layers > 1 && x3_fwd(g->layers[1])) {
        if (!f32a) a.C3 = ws.h3[0];
        wrote_x3 = true;
      }
      if (hbits(g, 0)) a.sgn = ws.hb[0];
      if (!h_f32(g, 0) && !f32a) a.C = nullptr;
      rc = damc::launch_gemm(a, damc::A_CONV, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "proj_fwd",
                             2.0 * B * (double)N * L.cin, s);
    } else if (L.kind == DAMC_LAYER_PROJ && damc::conv_kmajor_ok(L.cin)) {
      // z . W as a 1x1 "convolution" on the K-major engine; its B operand [(oy,ox,co)][ci] is the
      // dgrad packing
      const int N = L.hout * L.wout * L.cout;
      a.A = (i == 0) ? z : ws.h[i - 1];
      a.Cg = L.cin;
      a.B = L.w_bwd;
      a.b_kmajor = 1;
      a.ldb = L.cin;
      a.ldc = N;
      a.M = B;
      a.N = N;
      a.K = L.cin;
      a.k_per_z = a.K;
      rc = damc::launch_gemm(a, damc::A_CONV, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "proj_fwd",
                             2.0 * B * (double)N * L.cin, s);
    } else if (L.kind == DAMC_LAYER_PROJ || L.kind == DAMC_LAYER_LINEAR) {
      const int N = L.hout * L.wout * L.cout;
      a.A = (i == 0) ? z : ws.h[i - 1];
      a.lda = L.cin;
      a.B = L.w_fwd;
      a.ldb = N;
      a.ldc = N;
      a.M = B;
      a.N = N;
      a.K = L.cin;
      a.k_per_z = a.K;
      // a first layer whose nz is no multiple of 32 (SVHN, CelebA-64: nz = 100): the small-GEMM kernel, one 16 x 16
      // tile per wave (SVHN B=64: 2048 waves; the tiled engine ran 64 workgroups for 29 us); chosen by shape, never by
      // batch, so sharded chains stay bitwise the whole batch's
      rc = DAMC_ERR_UNSUPPORTED;
      if (L.kind == DAMC_LAYER_PROJ) {
        ProfScope ps("proj_fwd", 2.0 * B * (double)N * L.cin, s);
        rc = damc::launch_small_gemm(a.A, a.lda, a.B, a.ldb, L.bias, a.C, a.ldc, B, N, L.cin, s, L.cout, L.act,
                                     L.slope);
      }
      if (rc == DAMC_ERR_UNSUPPORTED)
        rc = damc::launch_gemm(a, damc::A_DENSE, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "proj_fwd",
                               2.0 * B * (double)N * L.cin, s);
    } else {  // UP2
      a = up2_fwd_args(L, B);
      a.A = ws.h[i - 1];
      a.C = ws.h[i];
      if (x3_fwd(L)) {
        if (f32a)
          a.a_f32 = 1;  // A = ws.h[i - 1] as fp32
        else
          a.A3 = ws.h3[i - 1];
        if (i + 1 < g->n_layers && x3_fwd(g->layers[i + 1])) {  // the next layer's operand
          if (!f32a) a.C3 = ws.h3[i];
          wrote_x3 = true;
        }
        if (hbits(g, i)) a.sgn = ws.hb[i];
        if (!h_f32(g, i) && !f32a) a.C = nullptr;
        a.kslab = ws.kslab;  // split-K when the batch leaves the grid under-filled
        a.kslab_floats = ws.kslab_floats;
        if (proj && i + 2 == g->n_layers) {  // the output layer's per-tap projections (smallc_fwd's stage 1, smallc.hip)
          const damc_layer_t& F = g->layers[i + 1];
          a.proj_w = F.w_bwd;
          a.proj_ldw = F.cin;
          a.proj_np = 32 * smallc_ntile(F);
          a.proj_out = ws.pbuf;
          a.proj_pstride = (long)B * F.hin * F.win * a.proj_np;
          // the activation itself is not stored when its sign bits carry the output layer's dgrad mask (k3 output
          // layers, hbits); a k4 s2 output layer's dgrad reads the fp32 activation's sign
          a.proj_nostore = hbits(g, i) ? 1 : 0;
          if (!a.C) a.C = ws.h[i];
        }
      }
      rc = damc::launch_gemm(a, damc::A_CONV, damc::EPI_BIAS_ACT, damc::O_PHASE, 4, "upconv_fwd", conv_flops(L, B), s);
    }
    if (rc) return rc;
    if (i + 1 < g->n_layers && x3_fwd(g->layers[i + 1]) && !wrote_x3 && !f32a) {
      ProfScope ps("split_x3", 0.0, s);
      if ((rc = damc::launch_split_x3(ws.h[i], act_floats(L, B), ws.h3[i], s))) return rc;
    }
  }
  return 0;
}

// the output layer's projection can run in the epilogue of the ConvT before it (limb engine, k4 s2, every channel in
// one 128 x 256 tile)
bool proj_fusable(const damc_generator_t* g, const Workspace& ws) {
  const int n = g->n_layers;
  if (n < 3 || !ws.pbuf) return false;
  const damc_layer_t& F = g->layers[n - 1];
  const damc_layer_t& L = g->layers[n - 2];
  return F.kind == DAMC_LAYER_SMALLC && damc::smallc_fwd_path(F, true, true) == damc::SMALLC_FWD_PROJ16 &&
         L.kind == DAMC_LAYER_UP2 && x3_fwd(L) && L.cout == F.cin &&
         (F.cin <= damc::PROJ_CHUNK || F.cin % damc::PROJ_CHUNK == 0);
}

// final layer forward: delta (+ optional x_hat NCHW / row-major) and |x_hat-x|^2/(2s^2) into sqerr
int forward_final(const damc_generator_t* g, int B, const float* z, const float* x, float inv_s2, Workspace& ws,
                  float* xhat, float* sqerr, bool want_delta, hipStream_t s, bool p_ready = false) {
  const int n = g->n_layers;
  const damc_layer_t& F = g->layers[n - 1];
  const float* hin = n >= 2 ? ws.h[n - 2] : z;
  if (F.kind == DAMC_LAYER_SMALLC)
    return damc::smallc_fwd(F, hin, B, want_delta ? x : nullptr, inv_s2, want_delta ? ws.delta : nullptr, xhat, sqerr,
                      ws.pbuf, s, p_ready);
  // LINEAR final layer
  GemmArgs a;
  a.A = hin;
  a.lda = F.cin;
  a.B = F.w_fwd;
  a.ldb = F.cout;
  a.ldc = F.cout;
  a.M = B;
  a.N = F.cout;
  a.K = F.cin;
  a.k_per_z = a.K;
  a.bias = F.bias;
  a.bias_mod = F.cout;
  a.act = F.act;
  a.slope = F.slope;
  if (want_delta) {
    a.C = ws.delta;
    a.xres = x;
    a.inv_s2 = inv_s2;
    a.xhat = xhat;
    a.sqerr = sqerr;
    int rc = damc::launch_gemm(a, damc::A_DENSE, damc::EPI_RESID, damc::O_DENSE, 1, "linear_out",
                               2.0 * B * (double)F.cout * F.cin, s);
    return rc;
  }
  a.C = xhat;
  return damc::launch_gemm(a, damc::A_DENSE, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "linear_out",
                           2.0 * B * (double)F.cout * F.cin, s);
}

// input gradient of layer i >= 1 from d (the gradient w.r.t. its pre-activation), masked with the
// activation derivative of layer i-1: the result (the pre-activation gradient of layer i-1) overwrites
// ws.h[i-1] and/or, when only a limb-engine dgrad reads it, ws.h3[i-1] (*x3_only = true)
// f32a: the gradients limb-engine dgrads read are stored fp32 (d_f32: the incoming d is fp32 even where a limb copy
// would have been read); *f32_out reports the form written
int dgrad_layer(const damc_generator_t* g, int B, Workspace& ws, int i, const float* d, bool* x3_only,
                hipStream_t s, bool f32a = false, bool d_f32 = false, bool* f32_out = nullptr) {
  if (f32_out) *f32_out = false;
  {
    const damc_layer_t& L = g->layers[i];
    const damc_layer_t& P = g->layers[i - 1];
    float* out = ws.h[i - 1];  // dgrad overwrites the activation it is masked with
    int rc;
    bool x3_out = false;  // the gradient went straight into its x3 copy
    if (L.kind == DAMC_LAYER_SMALLC) {
      const bool bits = hbits(g, i - 1);
      const damc::SmallcGrad form = damc::smallc_grad_form(L, bits, x3_bwd(P), f32a);
      x3_out = form == damc::SMALLC_GRAD_LIMBS;
      rc = damc::smallc_dgrad(L, out, B, d, P.act, P.slope, ws.h3[i - 1], bits ? ws.hb[i - 1] : nullptr, form, s);
      if (form == damc::SMALLC_GRAD_F32A && f32_out) *f32_out = true;
    } else if (L.kind == DAMC_LAYER_UP2) {
      GemmArgs a = up2_dgrad_args(L, B);
      a.A = d;
      a.C = out;
      a.mask = out;
      a.mask_act = P.act;
      a.mask_slope = P.slope;
      if (x3_bwd(L)) {
        if (d_f32)
          a.a_f32 = 1;  // A = d as fp32
        else
          a.A3 = ws.h3[i];
        a.kslab = ws.kslab;
        a.kslab_floats = ws.kslab_floats;
        if (hbits(g, i - 1)) {
          a.mask_sgn = ws.hb[i - 1];
          a.mask = nullptr;
        }
        if (x3_bwd(P) && f32a && hbits(g, i - 1)) {  // the next dgrad gathers this gradient as fp32
          if (f32_out) *f32_out = true;
        } else if (x3_bwd(P)) {  // only the next dgrad reads this gradient: limbs only, the fp32 activation stays
          a.C3 = ws.h3[i - 1];
          a.C = nullptr;
          x3_out = true;
        }
      }
      rc = damc::launch_gemm(a, damc::A_CONV, damc::EPI_MASK, damc::O_DENSE, 1, "upconv_dgrad", conv_flops(L, B), s);
    } else {  // LINEAR hidden/final
      GemmArgs a;
      a.A = d;
      a.lda = L.cout;
      a.B = L.w_bwd;
      a.ldb = L.cin;
      a.C = out;
      a.ldc = L.cin;
      a.M = B;
      a.N = L.cin;
      a.K = L.cout;
      a.k_per_z = a.K;
      a.mask = out;
      a.mask_act = P.act;
      a.mask_slope = P.slope;
      rc = damc::launch_gemm(a, damc::A_DENSE, damc::EPI_MASK, damc::O_DENSE, 1, "linear_dgrad",
                             2.0 * B * (double)L.cin * L.cout, s);
    }
    if (rc) return rc;
    if (x3_bwd(P) && !x3_out && !(f32_out && *f32_out)) {  // the next dgrad reads this gradient through the limb engine
      ProfScope ps("split_x3", 0.0, s);
      if ((rc = damc::launch_split_x3(out, act_floats(P, B), ws.h3[i - 1], s))) return rc;
    }
    *x3_only = x3_out;
  }
  return 0;
}

// first layer: dz = dA0 . W0^T  (split-K into slabs); d = the fp32 pre-activation gradient of layer 0
int dz_slabs(const damc_generator_t* g, int B, Workspace& ws, const float* d, hipStream_t s) {
  const damc_layer_t& L0 = g->layers[0];
  const long K = (long)L0.hout * L0.wout * L0.cout;
  GemmArgs a;
  a.A = d;
  a.lda = K;
  a.B = L0.w_bwd;
  a.ldb = L0.cin;
  const bool km = L0.kind == DAMC_LAYER_PROJ && damc::conv_kmajor_ok((int)K);
  if (km) {  // 1x1 "convolution" with Cg = K; B operand [ci][(oy,ox,co)] is the forward packing
    a.Cg = (int)K;
    a.B = L0.w_fwd;
    a.b_kmajor = 1;
    a.ldb = K;
  }
  a.C = ws.slabs;
  a.ldc = L0.cin;
  a.c_zstride = (long)B * L0.cin;
  a.M = B;
  a.N = L0.cin;
  a.K = (int)K;
  a.k_per_z = proj_k_per(K, ws.nslab);
  const int S = (int)((K + a.k_per_z - 1) / a.k_per_z);
  // slices beyond S (when rounding shrank the count) must contribute zeros.  Written by a kernel: this used to be a
  // hipMemsetAsync of all the slabs, the one kind of node a replayed graph does not order before the kernels behind
  // it; a captured G update then replayed with the memset landing on slices the GEMM had already
  // written (tests/test_gpu_gen_ops.py, the 7 x 7 first layer: 11 of 12 slices run)
  if (S < ws.nslab) {
    const long n = (long)(ws.nslab - S) * B * L0.cin;
    hipLaunchKernelGGL(zero_floats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       ws.slabs + (long)S * B * L0.cin, n);
    DAMC_LAUNCH_CHECK();
  }
  return damc::launch_gemm(a, km ? damc::A_CONV : damc::A_DENSE, damc::EPI_STORE, damc::O_DENSE, S, "proj_dgrad",
                           2.0 * B * (double)K * L0.cin, s);
}

// backward from ws.delta to the PROJ/first-layer split-K slabs (f32a: see dgrad_layer)
int backward(const damc_generator_t* g, int B, Workspace& ws, hipStream_t s, bool f32a = false) {
  const float* d = ws.delta;  // gradient w.r.t. the pre-activation of layer i (current)
  bool d_f32 = false;
  for (int i = g->n_layers - 1; i >= 1; --i) {
    bool x3_only = false, fo = false;
    int rc = dgrad_layer(g, B, ws, i, d, &x3_only, s, f32a, d_f32, &fo);
    if (rc) return rc;
    d = ws.h[i - 1];
    d_f32 = fo;
  }
  return dz_slabs(g, B, ws, d, s);
}

// ------------------------------------------------------------------ training backward (weight gradients)
// The G update of a training iteration (workspace/train_gen_recon.py:222-231): after the forward above,
// dL/dx_hat -> per-layer dL/dW, dL/db (and optionally dL/dz).  Layer i's weight gradient is taken before
// its input gradient overwrites the activation buffers it reads.  k4 s2 p1 and first-layer weight
// gradients run on the limb engine (gemm_x3.hip O_WGRAD) over pixel-major transposes (wgrad.hip) of the layer
// input and of the pre-activation gradient, the latter split into the 4 output phases; batches are padded
// to Bp = a multiple of 32 samples with zeros.
struct TrainWs {
  unsigned short* tin;  // transposed layer input, x3 [Cin][pixels][Bp]
  unsigned short* tdl;  // transposed pre-activation gradient, x3 [phase][Cout][pixels][Bp]
  float* wslab;         // O_WGRAD split-K slabs
  float* part;          // bias partial sums / output-layer wgrad partials
  float* ctmp;          // column-sum scratch
};

int bp_of(int B) { return (B + 31) / 32 * 32; }

// split-K of a k4 s2 p1 weight gradient: >= 512 workgroups; slice length a multiple of 32 (depends on the
// shape and Bp only)
void up2_wgrad_split(const damc_layer_t& L, int Bp, int* S, int* kper) {
  const long M = 4L * L.cin, N = L.cout, K = (long)L.hin * L.win * Bp;
  const long base = ((M + 255) / 256) * ((N + 127) / 128) * 4;
  const long nkt = K / 32;
  long sl = std::max(1L, std::min(std::min((512 + base - 1) / base, 16L), nkt));
  const long kp = (nkt + sl - 1) / sl * 32;
  *kper = (int)kp;
  *S = (int)((K + kp - 1) / kp);
}

// What train_backward's launches refuse by shape, asked on the host before the first launch of the G update (a
// refusal half way through the backward would come after out_delta and the output layer's kernels had run and the
// train record was consumed): launch_wgrad_x3 takes N = Cout (k4 s2 p1) or Cout k0 k0 (first layer) in whole octets
// and operands within 32-bit byte offsets; launch_smallc_wgrad has an instantiation and an LDS window for the output
// layer.  The plain forward and the Langevin entry points do not depend on any of this.
int train_supported(const damc_generator_t* g, int B) {
  const int Bp = bp_of(B);
  for (int i = 0; i < g->n_layers; ++i) {
    const damc_layer_t& L = g->layers[i];
    if (L.kind == DAMC_LAYER_UP2 || L.kind == DAMC_LAYER_PROJ) {
      const bool up2 = L.kind == DAMC_LAYER_UP2;
      const long N = up2 ? L.cout : (long)L.cout * L.hout * L.wout;
      const double K = (double)(up2 ? (long)L.hin * L.win : 1L) * Bp;
      if (N % 8 != 0) return DAMC_ERR_UNSUPPORTED;
      if (K >= 2147483647.0 || L.cin * K * 6 >= 2147483647.0 || N * K * 6 >= 2147483647.0) return DAMC_ERR_UNSUPPORTED;
    } else if (L.kind == DAMC_LAYER_SMALLC) {
      if (int rc = damc::smallc_wgrad_supported(L, B)) return rc;
    }
  }
  return 0;
}

size_t carve_train(const damc_generator_t* g, int B, char* base, TrainWs* t) {
  const int Bp = bp_of(B);
  size_t tin = 0, tdl = 0, wslab = 0, part = 0, ctmp = 0;
  for (int i = 0; i < g->n_layers; ++i) {
    const damc_layer_t& L = g->layers[i];
    const size_t nb = Bp / 32;
    if (L.kind == DAMC_LAYER_UP2) {
      const size_t P = (size_t)L.hin * L.win;
      int S, kp;
      up2_wgrad_split(L, Bp, &S, &kp);
      tin = std::max(tin, (size_t)L.cin * P * Bp);
      tdl = std::max(tdl, 4 * (size_t)L.cout * P * Bp);
      wslab = std::max(wslab, 4 * (size_t)S * 4 * L.cin * L.cout);
      part = std::max(part, 4 * P * nb * L.cout);
      ctmp = std::max(ctmp, damc::colsum_tmp_floats((long)(4 * P * nb), L.cout));
    } else if (L.kind == DAMC_LAYER_PROJ) {
      const size_t Pd = (size_t)L.hout * L.wout;
      tin = std::max(tin, (size_t)L.cin * Bp);
      tdl = std::max(tdl, (size_t)L.cout * Pd * Bp);
      part = std::max(part, Pd * nb * L.cout);
      ctmp = std::max(ctmp, damc::colsum_tmp_floats((long)(Pd * nb), L.cout));
    } else if (L.kind == DAMC_LAYER_SMALLC) {
      part = std::max(part, damc::smallc_wgrad_part_floats(L, B));
      ctmp = std::max(ctmp, damc::smallc_wgrad_tmp_floats(L, B));
      ctmp = std::max(ctmp, damc::colsum_tmp_floats((long)B * L.hout * L.wout, L.cout));
    } else {
      ctmp = std::max(ctmp, damc::colsum_tmp_floats(B, L.cout));
    }
  }
  size_t off = 0;
  auto take = [&](size_t bytes) -> char* {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return p;
  };
  char* p_tin = take(tin * 6);
  char* p_tdl = take(tdl * 6);
  char* p_ws = take(wslab * 4);
  char* p_part = take(part * 4);
  char* p_ct = take(ctmp * 4);
  if (t) {
    t->tin = reinterpret_cast<unsigned short*>(p_tin);
    t->tdl = reinterpret_cast<unsigned short*>(p_tdl);
    t->wslab = reinterpret_cast<float*>(p_ws);
    t->part = reinterpret_cast<float*>(p_part);
    t->ctmp = reinterpret_cast<float*>(p_ct);
  }
  return off;
}

int train_backward(const damc_generator_t* g, int B, const float* z, const float* xhat, const float* gx,
                   const damc_generator_grads_t* gr, float* gz, Workspace& ws, TrainWs& tw, hipStream_t s) {
  const int n = g->n_layers;
  const damc_layer_t& F = g->layers[n - 1];
  const int Bp = bp_of(B), nb = Bp / 32;
  int rc;
  {
    ProfScope ps("out_delta", 0.0, s);
    const int hw = F.kind == DAMC_LAYER_LINEAR ? 1 : F.hout * F.wout;
    if ((rc = damc::launch_out_delta(gx, xhat, B, F.cout, hw, F.act, ws.delta, s))) return rc;
  }
  const float* d = ws.delta;  // pre-activation gradient of layer i: fp32 ...
  bool d_x3 = false;          // ... or (when a limb dgrad wrote it) only the limbs in ws.h3[i]
  for (int i = n - 1; i >= 0; --i) {
    const damc_layer_t& L = g->layers[i];
    float* dW = gr->w[i];
    float* db = L.bias ? gr->b[i] : nullptr;
    const float* in32 = i ? ws.h[i - 1] : z;
    if (L.kind == DAMC_LAYER_SMALLC) {
      if (i == 0 || !h_f32(g, i - 1) || d_x3) return DAMC_ERR_UNSUPPORTED;
      if (dW && (rc = damc::launch_smallc_wgrad(L, in32, d, B, tw.part, tw.ctmp, dW, s))) return rc;
      if (db && (rc = damc::launch_colsum(d, (long)B * L.hout * L.wout, L.cout, L.cout, db, tw.ctmp, s))) return rc;
    } else if (L.kind == DAMC_LAYER_LINEAR) {
      if (d_x3 || (i > 0 && !h_f32(g, i - 1))) return DAMC_ERR_UNSUPPORTED;
      if (dW && (rc = damc::launch_linear_wgrad(d, in32, B, L.cout, L.cin, dW, s))) return rc;
      if (db && (rc = damc::launch_colsum(d, B, L.cout, L.cout, db, tw.ctmp, s))) return rc;
    } else {
      const bool up2 = L.kind == DAMC_LAYER_UP2;
      const int hq = up2 ? L.hin : 1, wq = up2 ? L.win : 1;
      const long P = (long)hq * wq;
      // layer input, pixel-major (the limbs the forward gathered, else fp32)
      const unsigned short* in3 = (up2 && x3_fwd(L)) ? ws.h3[i - 1] : nullptr;
      if (up2 && !in3 && !h_f32(g, i - 1)) return DAMC_ERR_UNSUPPORTED;
      if (dW && (rc = damc::launch_transpose_x3(in3 ? nullptr : in32, in3, B, hq, wq, L.cin, hq, wq, 1, 1, 0, 0, Bp,
                                                tw.tin, nullptr, s)))
        return rc;
      const float* d32 = d_x3 ? nullptr : d;
      const unsigned short* d3 = d_x3 ? ws.h3[i] : nullptr;
      if (up2) {  // the 4 output phases of the gradient, each on the input grid
        rc = damc::launch_transpose_x3_4ph(d32, d3, B, L.hout, L.wout, L.cout, L.hin, L.win, Bp, tw.tdl,
                                           (long)L.cout * P * Bp * 3, db ? tw.part : nullptr, (long)P * nb * L.cout, s);
        if (rc) return rc;
      } else {  // PROJ: rows (co, output pixel) = the PyTorch (Cin, Cout, k, k) column order
        rc = damc::launch_transpose_x3(d32, d3, B, L.hout, L.wout, L.cout, L.hout, L.wout, 1, 1, 0, 0, Bp, tw.tdl,
                                       db ? tw.part : nullptr, s);
        if (rc) return rc;
      }
      if (dW) {
        GemmArgs a;
        a.A3 = tw.tin;
        a.B3 = tw.tdl;
        a.Cg = L.cin;
        a.Hin = hq;
        a.Win = wq;
        a.K = (int)(P * Bp);
        a.wg_bp = Bp;
        if (up2) {
          int S, kp;
          up2_wgrad_split(L, Bp, &S, &kp);
          a.kw = 2;
          a.wg_phases = 4;
          a.M = 4 * L.cin;
          a.N = L.cout;
          a.ldc = L.cout;
          a.c_zstride = (long)a.M * a.N;
          a.b_zstride = (long)L.cout * a.K;
          a.k_per_z = kp;
          a.C = tw.wslab;
          if ((rc = damc::launch_wgrad_x3(a, S, "wgrad_up2", conv_flops(L, B), s))) return rc;
          if ((rc = damc::launch_up2_wgrad_reduce(tw.wslab, S, L.cin, L.cout, dW, s))) return rc;
        } else {
          a.kw = 1;
          a.wg_phases = 1;
          a.M = L.cin;
          a.N = L.cout * L.hout * L.wout;
          a.ldc = a.N;
          a.c_zstride = (long)a.M * a.N;
          a.k_per_z = a.K;
          a.C = dW;
          if ((rc = damc::launch_wgrad_x3(a, 1, "wgrad_proj", 2.0 * B * (double)a.M * a.N, s))) return rc;
        }
      }
      if (db) {
        const long rows = (up2 ? 4 * P : (long)L.hout * L.wout) * nb;
        if ((rc = damc::launch_colsum(tw.part, rows, L.cout, L.cout, db, tw.ctmp, s))) return rc;
      }
    }
    if (i >= 1) {
      bool x3o = false;
      if ((rc = dgrad_layer(g, B, ws, i, d, &x3o, s))) return rc;
      d = ws.h[i - 1];
      d_x3 = x3o;
    } else if (gz) {
      if (n < 2 || d_x3) return DAMC_ERR_UNSUPPORTED;
      if ((rc = dz_slabs(g, B, ws, d, s))) return rc;
      if ((rc = slab_sum(ws.slabs, ws.nslab, (long)B * g->nz, gz, s))) return rc;
    }
  }
  return 0;
}

}  // namespace

// =============================================================================== C ABI
extern "C" int damc_generator_layer_packed_sizes(const damc_layer_t* L, size_t* fwd, size_t* bwd) {
  if (!L || !fwd || !bwd) return DAMC_ERR_ARG;
  const size_t n = (size_t)L->cin * L->cout * (L->kind == DAMC_LAYER_LINEAR ? 1 : (size_t)L->k * L->k);
  switch (L->kind) {
    case DAMC_LAYER_UP2:
      // fp32 packing, then (limb engine) its x3 copy: 3 bf16 per element = 1.5 floats
      *fwd = n + (x3_fwd_cap(*L) ? n * 3 / 2 : 0);
      *bwd = n + (x3_bwd_cap(*L) ? n * 3 / 2 : 0);
      return 0;
    case DAMC_LAYER_PROJ:
      *fwd = n;
      *bwd = n + (x3_proj_cap(*L) ? n * 3 / 2 : 0);
      return 0;
    case DAMC_LAYER_LINEAR:
      *fwd = n;
      *bwd = n;
      return 0;
    case DAMC_LAYER_SMALLC:
      *fwd = n;
      *bwd = (size_t)smallc_ntile(*L) * 32 * L->cin;  // two-stage projection layout
      return 0;
  }
  return DAMC_ERR_ARG;
}

extern "C" int damc_x3_layer_sign_block(const damc_layer_t* L, int input_grad) {
  if (!L) return 0;
  if (input_grad) return x3_bwd_cap(*L) ? up2_negk_bwd(*L) : 0;
  return x3_fwd_cap(*L) ? up2_negk_fwd(*L) : 0;
}

extern "C" int damc_x3_layer_walk(const damc_layer_t* L, int input_grad) {
  if (!L) return 0;
  if (input_grad) return x3_bwd_cap(*L) ? damc::x3_up2_walk(L->cout) : 0;
  return x3_fwd_cap(*L) ? damc::x3_up2_walk(L->cin) : 0;
}

extern "C" int damc_x3_walk_ktile(int input_grad, int kt, int* channel0, int* tap) {
  if (kt < 0) return DAMC_ERR_ARG;
  const int wt = input_grad ? 16 : 4, pos = kt % wt;
  if (channel0) *channel0 = (kt / wt) * 32;
  if (tap) *tap = input_grad ? damc::x3_walk_tap(pos) : pos;
  return 0;
}

extern "C" int damc_x3_layer_tapshare(const damc_layer_t* L, int input_grad) {
  if (!damc_x3_layer_walk(L, input_grad)) return 0;
  const int nk = input_grad ? up2_negk_bwd(*L) : up2_negk_fwd(*L);
  return (damc::x3_tapshare_ok(L->hin, L->win) && nk % 128 == 0 && L->hout == 2 * L->hin && L->wout == 2 * L->win) ? 1 : 0;
}

extern "C" int damc_pack_generator_layer(const damc_layer_t* L, const float* w, float* wf, float* wb, void* stream) {
  if (!L || !w || !wf) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  const long n = (long)L->cin * L->cout * (L->kind == DAMC_LAYER_LINEAR ? 1 : (long)L->k * L->k);
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  // LDS-tiled packing (fp32 + limbs in one pass) unless DAMC_PACK_TILED=0 (the element-wise A/B; bitwise the same)
  const char* pt = getenv("DAMC_PACK_TILED");
  const bool tiled = !(pt && pt[0] == '0');
  switch (L->kind) {
    case DAMC_LAYER_PROJ:
      if (!wb) return DAMC_ERR_ARG;
      if (tiled) {
        const int rc = damc::launch_pack_proj_tiled(
            w, L->cin, L->cout, L->k * L->k, wf, wb,
            x3_proj_cap(*L) ? reinterpret_cast<unsigned short*>(wb + n) : nullptr, s);
        if (rc != 1) return rc;
      }
      hipLaunchKernelGGL(pack_proj_kernel, grid, blk, 0, s, w, L->cin, L->cout, L->k, wf, wb);
      if (x3_proj_cap(*L))
        DAMC_CHECK((hipError_t)damc::launch_split_x3_negblk(wb, n, L->cin, reinterpret_cast<unsigned short*>(wb + n), s));
      break;
    case DAMC_LAYER_UP2:
      if (!wb || L->k != 4) return DAMC_ERR_ARG;
      if (tiled) {
        const int rc = damc::launch_pack_up2_tiled(
            w, L->cin, L->cout, wf, x3_fwd_cap(*L) ? reinterpret_cast<unsigned short*>(wf + n) : nullptr, wb,
            x3_bwd_cap(*L) ? reinterpret_cast<unsigned short*>(wb + n) : nullptr, s, up2_negk_fwd(*L),
            up2_negk_bwd(*L));
        if (rc != 1) return rc;
      }
      hipLaunchKernelGGL(pack_up2_kernel, grid, blk, 0, s, w, L->cin, L->cout, (int)damc::conv_kmajor_ok(L->cin),
                         (int)damc::conv_kmajor_ok(L->cout), wf, wb);
      // x3 copies with sign-alternating K blocks (gemm.h GemmArgs::b_negblk): rows of 4 Cin (forward, per phase
      // and output channel) and 16 Cout (input gradient, per input channel)
      // (in the K order the limb-engine kernels walk: damc::launch_split_x3_conv)
      // (in the slice-major order of damc::x3_up2_walk, which the capability implies)
      if (x3_fwd_cap(*L))
        DAMC_CHECK((hipError_t)(damc::x3_up2_walk(L->cin)
                                    ? damc::launch_split_x3_cmaj(wf, n, 4 * L->cin, L->cin, 32,
                                                                 reinterpret_cast<unsigned short*>(wf + n), s, up2_negk_fwd(*L))
                                    : damc::launch_split_x3_conv(wf, n, 4 * L->cin, L->cin,
                                                                 reinterpret_cast<unsigned short*>(wf + n), s, up2_negk_fwd(*L))));
      if (x3_bwd_cap(*L))
        DAMC_CHECK((hipError_t)(damc::x3_up2_walk(L->cout)
                                    ? damc::launch_split_x3_walk(wb, n, 16 * L->cout, L->cout,
                                                                 reinterpret_cast<unsigned short*>(wb + n), s, up2_negk_bwd(*L))
                                    : damc::launch_split_x3_conv(wb, n, 16 * L->cout, L->cout,
                                                                 reinterpret_cast<unsigned short*>(wb + n), s, up2_negk_bwd(*L))));
      break;
    case DAMC_LAYER_SMALLC:
      if (wb) DAMC_CHECK(hipMemsetAsync(wb, 0, sizeof(float) * smallc_ntile(*L) * 32 * (size_t)L->cin, s));
      hipLaunchKernelGGL(pack_smallc_kernel, grid, blk, 0, s, w, L->cin, L->cout, L->k, wf, wb);
      break;
    case DAMC_LAYER_LINEAR:
      if (!wb) return DAMC_ERR_ARG;
      hipLaunchKernelGGL(pack_linear_kernel, grid, blk, 0, s, w, L->cin, L->cout, wf, wb);
      break;
    default:
      return DAMC_ERR_ARG;
  }
  return (int)hipGetLastError();
}

extern "C" size_t damc_posterior_workspace_bytes(const damc_generator_t* g, int B) {
  if (validate(g) || B <= 0) return 0;
  return carve(g, B, nullptr, nullptr);
}

static int setup_ws(const damc_generator_t* g, int B, void* wsp, size_t wsb, Workspace* ws) {
  int rc = validate(g);
  if (rc) return rc;
  if (B <= 0) return DAMC_ERR_ARG;
  const size_t need = carve(g, B, nullptr, nullptr);
  if (!wsp || wsb < need) return DAMC_ERR_WORKSPACE;
  carve(g, B, reinterpret_cast<char*>(wsp), ws);
  return 0;
}

extern "C" int damc_generator_forward(const damc_generator_t* g, const float* z, int B, float* xhat, void* wsp,
                                      size_t wsb, void* stream) {
  Workspace ws;
  int rc = setup_ws(g, B, wsp, wsb, &ws);
  if (rc) return rc;
  if (!z || !xhat) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  rc = forward_hidden(g, z, B, ws, s);
  if (rc) return rc;
  return forward_final(g, B, z, nullptr, 1.f, ws, xhat, nullptr, false, s);
}

extern "C" int damc_likelihood_grad(const damc_generator_t* g, const float* z, const float* x, int B, double sigma,
                                    float* grad, void* wsp, size_t wsb, void* stream) {
  Workspace ws;
  int rc = setup_ws(g, B, wsp, wsb, &ws);
  if (rc) return rc;
  if (!z || !x || !grad) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  const float inv_s2 = (float)(1.0 / (sigma * sigma));
  if ((rc = forward_hidden(g, z, B, ws, s))) return rc;
  if ((rc = forward_final(g, B, z, x, inv_s2, ws, nullptr, nullptr, true, s))) return rc;
  if (g->n_layers == 1) {
    // single layer: the delta is the gradient w.r.t. layer-0 pre-activation; dz = delta . W
    return DAMC_ERR_UNSUPPORTED;
  }
  if ((rc = backward(g, B, ws, s))) return rc;
  const long n = (long)B * g->nz;
  return slab_sum(ws.slabs, ws.nslab, n, grad, s);
}

// ---- per-op hooks for ONE k4 s2 p1 ConvTranspose2d layer (damc_convT_fwd / damc_convT_dgrad),
// NHWC activations, the same kernels and engine choice as inside the Langevin step (both start from up2_fwd_args /
// up2_dgrad_args)
static bool hook_f32a(const float* act) {
  const char* fa = getenv("DAMC_X3_F32A");
  return !(fa && fa[0] == '0') && (uintptr_t)act % 16 == 0;
}
static bool up2_hook_ok(const damc_layer_t* L, int B) {
  return L && B > 0 && L->kind == DAMC_LAYER_UP2 && L->k == 4 && L->stride == 2 && L->pad == 1 && L->cin > 0 &&
         L->cout > 0 && L->hout == 2 * L->hin && L->wout == 2 * L->win && L->w_fwd && L->w_bwd;
}

extern "C" size_t damc_convT_workspace_bytes(const damc_layer_t* L, int B) {
  if (!up2_hook_ok(L, B)) return 0;
  const size_t in = (size_t)B * L->hin * L->win * L->cin, out = (size_t)B * L->hout * L->wout * L->cout;
  return (std::max(in, out) * 6 + 255) / 256 * 256;  // limb copy of the A operand
}

extern "C" int damc_convT_fwd(const damc_layer_t* L, const float* in, int B, float* out, void* wsp, size_t wsb,
                              void* stream) {
  if (!up2_hook_ok(L, B) || !in || !out) return DAMC_ERR_ARG;
  if (!wsp || wsb < damc_convT_workspace_bytes(L, B)) return DAMC_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  GemmArgs a = up2_fwd_args(*L, B);
  a.C = out;
  a.A = in;
  int rc;
  if (x3_fwd(*L)) {
    // the fp32 input gathered as it is (gemm_x3.hip X3_F32A), as inside the Langevin step; DAMC_X3_F32A=0 (read per call)
    // gathers a limb copy (bitwise the same)
    if (hook_f32a(in)) {
      a.a_f32 = 1;
    } else {
      unsigned short* a3 = reinterpret_cast<unsigned short*>(wsp);
      if ((rc = damc::launch_split_x3(in, (long)B * L->hin * L->win * L->cin, a3, s))) return rc;
      a.A3 = a3;
    }
  }
  return damc::launch_gemm(a, damc::A_CONV, damc::EPI_BIAS_ACT, damc::O_PHASE, 4, "upconv_fwd", conv_flops(*L, B), s);
}

extern "C" int damc_convT_dgrad(const damc_layer_t* L, const float* gout, int B, const float* mask_pre, int mask_act,
                                float mask_slope, float* gin, void* wsp, size_t wsb, void* stream) {
  if (!up2_hook_ok(L, B) || !gout || !gin) return DAMC_ERR_ARG;
  if (!wsp || wsb < damc_convT_workspace_bytes(L, B)) return DAMC_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  GemmArgs a = up2_dgrad_args(*L, B);
  a.A = gout;
  a.C = gin;
  a.mask = mask_pre;
  a.mask_act = mask_pre ? mask_act : DAMC_ACT_NONE;
  a.mask_slope = mask_slope;
  int rc;
  if (x3_bwd(*L)) {
    if (hook_f32a(gout)) {
      a.a_f32 = 1;
    } else {
      unsigned short* a3 = reinterpret_cast<unsigned short*>(wsp);
      if ((rc = damc::launch_split_x3(gout, (long)B * L->hout * L->wout * L->cout, a3, s))) return rc;
      a.A3 = a3;
    }
  }
  return damc::launch_gemm(a, damc::A_CONV, mask_pre ? damc::EPI_MASK : damc::EPI_STORE, damc::O_DENSE, 1,
                           "upconv_dgrad", conv_flops(*L, B), s);
}

// ds: the drawn form's device-resident key (the update kernel reads it, common.h draw_key), null for a host seed
static int posterior_langevin_impl(const damc_generator_t* g, const damc_ebm_t* ebm, float* z, const float* x, int B,
                                   int n_steps, double sigma, double step, int with_noise, const float* noise,
                                   uint64_t seed, uint64_t step_offset, uint64_t chain_base, float* diag, void* wsp,
                                   size_t wsb, void* stream, const damc_draw_state_t* ds) {
  Workspace ws;
  int rc = setup_ws(g, B, wsp, wsb, &ws);
  if (rc) return rc;
  if (!z || !x || n_steps < 0) return DAMC_ERR_ARG;
  if (g->n_layers < 2) return DAMC_ERR_UNSUPPORTED;
  if (ebm && (ebm->nz != g->nz || !ebm->w1t || !ebm->w2t)) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  if (diag) DAMC_CHECK(hipMemsetAsync(diag, 0, sizeof(float) * 4 * (size_t)n_steps, s));
  const float inv_s2 = (float)(1.0 / (sigma * sigma));
  // the register-resident update kernel sums the first layer's split-K slabs itself (slab_sum4's order) and writes
  // z's limbs for the next step's first layer; DAMC_POST_FUSE=0 (read per call) keeps the separate kernels
  const char* pf = getenv("DAMC_POST_FUSE");
  const bool fuse = !(pf && pf[0] == '0');
  // the limb-engine convolutions gather fp32 activations and gradients (gemm_x3.hip X3_F32A), bitwise the limb-gathering
  // form; DAMC_X3_F32A=0 (read per call) gathers limbs (CIFAR B=128 bench 51.1K -> 56.1K z-steps/s, B=16 per-rank
  // step 0.625 -> 0.478 ms; profiles/r04/bench_f32a_ab.txt, step_f32a_ab.txt)
  const char* fa = getenv("DAMC_X3_F32A");
  const bool f32a = !(fa && fa[0] == '0');
  // DAMC_SMALLC_FUSE (read per call, default on): the last ConvT's epilogue runs the output layer's projection on both
  // paths: the F32A tile projects its own 128-channel chunk per N tile (the gather adds the chunks' partials), the
  // limb-gathering path (DAMC_X3_F32A=0) projects every channel in the 128 x 256 tile
  const char* sf = getenv("DAMC_SMALLC_FUSE");
  const bool proj = !(sf && sf[0] == '0') && proj_fusable(g, ws);
  const bool z3_use = x3_proj(g->layers[0]) && ws.z3;
  bool z3_ready = false;
  for (int i = 0; i < n_steps; ++i) {
    float* dg = diag ? diag + 4 * i : nullptr;
    if ((rc = forward_hidden(g, z, B, ws, s, z3_ready, f32a, proj))) return rc;
    if ((rc = forward_final(g, B, z, x, inv_s2, ws, nullptr, dg ? dg + 1 : nullptr, true, s, proj))) return rc;
    if ((rc = backward(g, B, ws, s, f32a))) return rc;
    const float* nz_i = noise ? noise + (size_t)i * B * g->nz : nullptr;
    const long n = (long)B * g->nz;
    // fused only where slab_sum takes its slab_sum4 order (the order the update kernel reproduces)
    const bool f = fuse && damc_posterior_update_fusable(ebm, g->nz) && (n & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(ws.slabs) | reinterpret_cast<uintptr_t>(ws.glik)) & 15) == 0;
    if (!f && (rc = slab_sum(ws.slabs, ws.nslab, n, ws.glik, s))) return rc;
    bool wrote = false;
    rc = damc_launch_posterior_update(ebm, z, f ? ws.slabs : ws.glik, f ? ws.nslab : 1, n, B, g->nz, step,
                                      with_noise, nz_i, seed, step_offset + i, chain_base, dg, s,
                                      (f && z3_use) ? ws.z3 : nullptr, &wrote, ds);
    if (rc) return rc;
    z3_ready = wrote;
  }
  return 0;
}

extern "C" int damc_posterior_langevin(const damc_generator_t* g, const damc_ebm_t* ebm, float* z, const float* x,
                                       int B, int n_steps, double sigma, double step, int with_noise, const float* noise,
                                       uint64_t seed, uint64_t step_offset, uint64_t chain_base, float* diag,
                                       void* wsp, size_t wsb, void* stream) {
  return posterior_langevin_impl(g, ebm, z, x, B, n_steps, sigma, step, with_noise, noise, seed, step_offset,
                                 chain_base, diag, wsp, wsb, stream, nullptr);
}

extern "C" int damc_posterior_langevin_ds(const damc_generator_t* g, const damc_ebm_t* ebm, float* z, const float* x,
                                          int B, int n_steps, double sigma, double step, int with_noise,
                                          const float* noise, const damc_draw_state_t* state, uint64_t step_offset,
                                          uint64_t chain_base, float* diag, void* wsp, size_t wsb, void* stream) {
  if (!state) return DAMC_ERR_ARG;
  return posterior_langevin_impl(g, ebm, z, x, B, n_steps, sigma, step, with_noise, noise, 0, step_offset, chain_base,
                                 diag, wsp, wsb, stream, state);
}

// ------------------------------------------------------------------------------------ training (G update)
extern "C" size_t damc_generator_train_workspace_bytes(const damc_generator_t* g, int B) {
  if (validate(g) || B <= 0 || train_supported(g, B)) return 0;
  return carve(g, B, nullptr, nullptr) + carve_train(g, B, nullptr, nullptr);
}

static int setup_train(const damc_generator_t* g, int B, void* wsp, size_t wsb, Workspace* ws, TrainWs* tw) {
  int rc = validate(g);
  if (rc) return rc;
  if (B <= 0) return DAMC_ERR_ARG;
  if ((rc = train_supported(g, B))) return rc;
  const size_t n0 = carve(g, B, nullptr, nullptr);
  const size_t n1 = carve_train(g, B, nullptr, nullptr);
  if (!wsp || wsb < n0 + n1) return DAMC_ERR_WORKSPACE;
  carve(g, B, reinterpret_cast<char*>(wsp), ws);
  carve_train(g, B, reinterpret_cast<char*>(wsp) + n0, tw);
  return 0;
}

// The engine a G-update forward ran on decides which buffers it filled (limbs + sign bits, or fp32
// activations), so the backward must run on the same one: train_forward records (batch, engine) per
// workspace and train_backward refuses a descriptor that disagrees (DAMC_ERR_ARG) instead of reading
// buffers the forward never wrote.  Keyed by the caller's workspace, so concurrent streams / threads with
// their own workspaces do not interfere.  The backward consumes the record: it overwrites activation buffers
// as it goes, so a second backward of one forward (retain_graph) is refused rather than run on clobbered
// inputs.  The table is a bounded ring: a forward that is never backpropagated holds one slot until 64 newer
// workspaces have been recorded.
static std::mutex g_train_mu;
constexpr int TRAIN_REC_SLOTS = 64;
static const void* g_train_ws[TRAIN_REC_SLOTS];
static long g_train_key[TRAIN_REC_SLOTS];
static int g_train_next = 0;
static long train_key(const damc_generator_t* g, int B) { return (long)B * 4 + g->layers[0].engine; }
static int train_rec_find(const void* wsp) {
  for (int i = 0; i < TRAIN_REC_SLOTS; ++i)
    if (g_train_ws[i] == wsp) return i;
  return -1;
}

extern "C" int damc_generator_train_forward(const damc_generator_t* g, const float* z, int B, float* xhat, void* wsp,
                                            size_t wsb, void* stream) {
  Workspace ws;
  TrainWs tw;
  int rc = setup_train(g, B, wsp, wsb, &ws, &tw);
  if (rc) return rc;
  if (!z || !xhat) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  if ((rc = forward_hidden(g, z, B, ws, s))) return rc;
  if ((rc = forward_final(g, B, z, nullptr, 1.f, ws, xhat, nullptr, false, s))) return rc;
  std::lock_guard<std::mutex> lk(g_train_mu);
  int i = train_rec_find(wsp);
  if (i < 0) {
    i = g_train_next;
    g_train_next = (g_train_next + 1) % TRAIN_REC_SLOTS;
    g_train_ws[i] = wsp;
  }
  g_train_key[i] = train_key(g, B);
  return 0;
}

extern "C" int damc_generator_train_backward(const damc_generator_t* g, const float* z, const float* xhat,
                                             const float* grad_xhat, int B, const damc_generator_grads_t* grads,
                                             float* grad_z, void* wsp, size_t wsb, void* stream) {
  Workspace ws;
  TrainWs tw;
  int rc = setup_train(g, B, wsp, wsb, &ws, &tw);
  if (rc) return rc;
  if (!z || !xhat || !grad_xhat || !grads) return DAMC_ERR_ARG;
  {
    std::lock_guard<std::mutex> lk(g_train_mu);
    const int i = train_rec_find(wsp);
    if (i < 0 || g_train_key[i] != train_key(g, B)) return DAMC_ERR_ARG;
    g_train_ws[i] = nullptr;
  }
  return train_backward(g, B, z, xhat, grad_xhat, grads, grad_z, ws, tw, as_stream(stream));
}
