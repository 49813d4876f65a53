// encoder.hip — the amortizer's image encoder Encoder_* (workspace/src/diffusion_net.py:227-413):
// [Conv2d -> InstanceNorm2d(affine, eps=1e-5) -> LeakyReLU(0.2)]* -> Conv2d, on NHWC activations.
// This file: the whole forward in one call (damc_q_encoder_fwd: its shapes, workspace and steps) and the per-op conv
// entry points.  Convolutions run on the fp32 MFMA implicit-GEMM engine (gemm.hip) or the limb engine (gemm_x3.hip).
// The stages the forward calls live in their own files and share enc_impl.h: the first layer (enc_first.hip), the
// InstanceNorm + LeakyReLU forms and the per-op norm calls (enc_norm.hip), the dense head (enc_head.hip).
#include <algorithm>

#include "enc_impl.h"

namespace {

// (Cout,Cin,k,k) -> [(ky,kx,ci)][co], or [co][(ky,kx,ci)] for the K-major engine (km)
__global__ void pack_conv_kernel(const float* w, int cout, int cin, int k, int km, float* wp) {
  const long n = (long)cout * cin * k * k;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long t = i;
  const int kx = (int)(t % k);
  t /= k;
  const int ky = (int)(t % k);
  t /= k;
  const int ci = (int)(t % cin);
  const int co = (int)(t / cin);
  const long kk = ((long)ky * k + kx) * cin + ci;
  if (km)
    wp[(long)co * k * k * cin + kk] = w[i];
  else
    wp[kk * cout + co] = w[i];
}

__global__ void nchw_to_nhwc_kernel(const float* x, int B, int C, int HW, float* y) {
  const long n = (long)B * C * HW;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // i enumerates the NHWC output
  const int c = (int)(i % C);
  const long t = i / C;
  const int p = (int)(t % HW);
  const int b = (int)(t / HW);
  y[i] = x[((long)b * C + c) * HW + p];
}

// split-K slices for a K-major conv whose output tiles would not fill the chip (the encoder's deeper
// layers: 64 / 8 tiles at B=128), each slice >= 8 K tiles; 1 = no split
int conv_split(long M, int N, int K) {
  const long tiles = ((M + 127) / 128) * ((N + 127) / 128);
  if (tiles >= 192 || K < 512) return 1;
  const long s = std::min<long>((256 + tiles - 1) / tiles, K / 256);
  return (int)std::max<long>(1, s);
}

// y[m][n] = sum of the S slabs [S][M][N] + bias[n], fixed order
__global__ __launch_bounds__(256) void conv_slab_sum_kernel(const float* __restrict__ slabs, int S, long M, int N,
                                                            const float* __restrict__ bias, float* __restrict__ y) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * N) return;
  float acc = 0.f;
  for (int z = 0; z < S; ++z) acc += slabs[(long)z * M * N + i];
  if (bias) acc += bias[i % N];
  y[i] = acc;
}

}  // namespace

extern "C" int damc_pack_conv2d(const float* w, int cout, int cin, int k, float* wp, void* stream) {
  if (!w || !wp || cout <= 0 || cin <= 0 || k <= 0) return DAMC_ERR_ARG;
  const long n = (long)cout * cin * k * k;
  hipLaunchKernelGGL(pack_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), w, cout, cin,
                     k, (int)damc::conv_kmajor_ok(cin), wp);
  return (int)hipGetLastError();
}

extern "C" int damc_nchw_to_nhwc(const float* x, int B, int C, int HW, float* y, void* stream) {
  if (!x || !y || B <= 0 || C <= 0 || HW <= 0) return DAMC_ERR_ARG;
  const long n = (long)B * C * HW;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, B, C,
                     HW, y);
  return (int)hipGetLastError();
}

extern "C" size_t damc_conv2d_workspace_floats(int B, int hin, int win, int cin, int cout, int k, int stride,
                                               int pad) {
  if (B <= 0 || cin <= 0 || cout <= 0 || k <= 0 || stride <= 0) return 0;
  const int hout = (hin + 2 * pad - k) / stride + 1, wout = (win + 2 * pad - k) / stride + 1;
  if (hout <= 0 || wout <= 0 || !damc::conv_kmajor_ok(cin)) return 0;
  const long M = (long)B * hout * wout;
  const int S = conv_split(M, cout, k * k * cin);
  return S > 1 ? (size_t)S * M * cout : 0;
}

extern "C" int damc_conv2d_nhwc(const float* x, int B, int hin, int win, int cin, const float* wp, const float* bias,
                                int cout, int k, int stride, int pad, float* y, float* workspace,
                                size_t workspace_floats, void* stream) {
  if (!x || !wp || !y || B <= 0) return DAMC_ERR_ARG;
  const int hout = (hin + 2 * pad - k) / stride + 1, wout = (win + 2 * pad - k) / stride + 1;
  if (hout <= 0 || wout <= 0) return DAMC_ERR_ARG;
  damc::GemmArgs a;
  a.A = x;
  a.Hin = hin;
  a.Win = win;
  a.Cg = cin;
  a.Hq = hout;
  a.Wq = wout;
  a.kw = k;
  a.stride = stride;
  a.pad_y = pad;
  a.pad_x = pad;
  a.B = wp;
  a.b_kmajor = damc::conv_kmajor_ok(cin);
  a.ldb = a.b_kmajor ? (long)k * k * cin : cout;
  a.C = y;
  a.ldc = cout;
  a.M = B * hout * wout;
  a.N = cout;
  a.K = k * k * cin;
  a.k_per_z = a.K;
  a.bias = bias;
  a.bias_mod = cout;
  a.act = DAMC_ACT_NONE;
  hipStream_t s = as_stream(stream);
  const double flops = 2.0 * a.M * (double)cout * a.K;
  int S = a.b_kmajor ? conv_split(a.M, cout, a.K) : 1;
  if (S > 1 && workspace && workspace_floats >= (size_t)S * a.M * cout) {
    // split K over S slices (multiples of the engine's 32-deep K tile, so no tile straddles a tap)
    a.k_per_z = (a.K / 32 + S - 1) / S * 32;
    S = (a.K + a.k_per_z - 1) / a.k_per_z;
    a.C = workspace;
    a.c_zstride = (long)a.M * cout;
    a.bias = nullptr;
    int rc = damc::launch_gemm(a, damc::A_CONV, damc::EPI_STORE, damc::O_DENSE, S, "enc_conv", flops, s);
    if (rc) return rc;
    const long n = (long)a.M * cout;
    hipLaunchKernelGGL(conv_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       (const float*)workspace, S, (long)a.M, cout, bias, y);
    return (int)hipGetLastError();
  }
  return damc::launch_gemm(a, damc::A_CONV, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "enc_conv", flops, s);
}

// ---- the whole encoder forward in one call (damc_q_encoder_fwd): NCHW -> NHWC, then per layer the conv and
// InstanceNorm + LeakyReLU in place; two ping-pong activation buffers, the last conv writes xemb directly.
// Convolutions with cin % 32 == 0 (all but the first 3x3 at the reference's nif) run on the limb engine
// (gemm_x3_kernel, A_CONV gather with stride / pad, bias epilogue; split-K into the sign blocks when the grid would
// not fill the chip): the input activation is split into limbs per call, the weights' limb copy comes from the
// caller (damc_pack_conv2d_x3) or is split into the workspace.  The rest on the fp32 MFMA engine.
namespace {
struct EncShapes {
  int h[DAMC_MAX_ENC_LAYERS + 1], w[DAMC_MAX_ENC_LAYERS + 1];
  size_t act_max = 0, slab_max = 0, in_max = 0;
  size_t a3_max = 0, w3_max = 0, ks_max = 0;  // limb engine: activation limbs, weight limbs, split-K slabs
  size_t wsrc_off[DAMC_MAX_ENC_LAYERS] = {}, wsrc_bytes = 0;  // the limb operands packed from w_src (workspace)
  bool limb[DAMC_MAX_ENC_LAYERS] = {};
  bool first_fused = false;  // layer 0 by enc_first.hip (no stored conv output, no NHWC copy)
  int first_rows = 1, first_strips = 1;
  bool head_geom = false;  // the last conv fits enc_head_x3_kernel (its slabs are in ks_max)
};
size_t round256(size_t b) { return (b + 255) / 256 * 256; }

bool enc_limb_layer(const damc_encoder_t* e, const damc_enc_layer_t& L) {
  return e->engine == DAMC_ENGINE_LIMB && damc::conv_kmajor_ok(L.cin) && L.cout % 8 == 0 && L.k * L.k <= 32;
}
bool enc_shapes(const damc_encoder_t* e, int B, EncShapes* sh) {
  if (!e || B <= 0 || e->n_layers < 1 || e->n_layers > DAMC_MAX_ENC_LAYERS || e->nc <= 0 || e->h <= 0 || e->w <= 0)
    return false;
  if (e->engine != DAMC_ENGINE_LIMB && e->engine != DAMC_ENGINE_FP32) return false;
  sh->h[0] = e->h;
  sh->w[0] = e->w;
  int c = e->nc;
  sh->act_max = (size_t)B * e->h * e->w * e->nc;
  for (int i = 0; i < e->n_layers; ++i) {
    const damc_enc_layer_t& L = e->layers[i];
    if (L.cin != c || L.cout <= 0 || L.k <= 0 || L.stride <= 0 || L.pad < 0) return false;
    if ((L.in_gamma == nullptr) != (L.in_beta == nullptr)) return false;
    const int ho = (sh->h[i] + 2 * L.pad - L.k) / L.stride + 1, wo = (sh->w[i] + 2 * L.pad - L.k) / L.stride + 1;
    if (ho <= 0 || wo <= 0) return false;
    sh->h[i + 1] = ho;
    sh->w[i + 1] = wo;
    if (i + 1 < e->n_layers) sh->act_max = std::max(sh->act_max, (size_t)B * ho * wo * L.cout);
    sh->limb[i] = enc_limb_layer(e, L);
    if (!L.w_packed && !(sh->limb[i] && (L.w_x3 || L.w_src))) return false;  // the engine's weight operand
    if (L.w_src && (!sh->limb[i] || L.w_x3 || (uintptr_t)L.w_src % 16 != 0)) return false;
    if (sh->limb[i]) {
      const long M = (long)B * ho * wo, K = (long)L.k * L.k * L.cin;
      sh->a3_max = std::max(sh->a3_max, (size_t)B * sh->h[i] * sh->w[i] * L.cin * 6);
      if (L.w_src) {
        sh->wsrc_off[i] = sh->wsrc_bytes;
        sh->wsrc_bytes += round256((size_t)L.cout * K * 6);
      } else if (!L.w_x3) {
        sh->w3_max = std::max(sh->w3_max, (size_t)L.cout * K * 6);
      }
      sh->ks_max = std::max(sh->ks_max, (size_t)damc::x3_ksplit_floats((int)M, L.cout, (int)K, 1));
    } else {
      sh->slab_max = std::max(sh->slab_max,
                              damc_conv2d_workspace_floats(B, sh->h[i], sh->w[i], L.cin, L.cout, L.k, L.stride, L.pad));
    }
    if (L.in_gamma)
      sh->in_max = std::max(sh->in_max, damc_instnorm_workspace_floats(B, ho * wo, L.cout) + (size_t)B * L.cout * 2);
    c = L.cout;
  }
  const damc_enc_layer_t& F0 = e->layers[0];
  sh->first_fused = e->n_layers > 1 && sh->limb[1] && F0.k == 3 && F0.stride == 1 && F0.pad == 1 &&
                    (F0.cin == 1 || F0.cin == 3 || F0.cin == 4) && F0.cout % 64 == 0 && F0.cout <= 512 &&
                    F0.in_gamma && F0.w_packed && !damc::conv_kmajor_ok(F0.cin) && e->w <= 1024;
  if (sh->first_fused) {
    // strips per sample from the sample's shape alone, never the batch (each strip's lanes merge their statistics once,
    // a butterfly per channel octet, and in_merge_kernel merges the strips in a fixed tree: the strip partition sets the
    // rounding, so a batch sharded over ranks must keep the whole batch's partition to reproduce its xemb bit for bit;
    // round 5 took ~1024 / B strips, and 8 x B=8 CelebA-HQ shards differed from B=64 in every row,
    // tests/test_gpu_strong_scaling.py): ~512 pixels per strip, at most 64 strips, at least 128 pixels per strip
    const int want = std::max(1, std::min(64, e->h * e->w / 512));
    sh->first_rows = std::max((e->h + want - 1) / want, (128 + e->w - 1) / e->w);
    sh->first_strips = (e->h + sh->first_rows - 1) / sh->first_rows;
    sh->in_max = std::max(sh->in_max, (size_t)B * F0.cout * (sh->first_strips * 3 + 2));
    sh->a3_max = std::max(sh->a3_max, (size_t)B * e->h * e->w * F0.cout * 6);
  }
  // the dense head: the last conv covers its k x k input, reads the PyTorch weight (w_src), and the norm before it is
  // the one-pass kernel (which then writes the head's CHW rows)
  const int nl = e->n_layers - 1;
  const damc_enc_layer_t& LH = e->layers[nl];
  const long KH = (long)LH.cin * LH.k * LH.k;
  sh->head_geom = nl >= 2 && sh->limb[nl] && LH.w_src && LH.stride == 1 && LH.pad == 0 && sh->h[nl] == LH.k &&
                  sh->w[nl] == LH.k && LH.cout % damc::HD_BN == 0 && KH % damc::HD_NEGK == 0 &&
                  e->layers[nl - 1].in_gamma && e->layers[nl - 1].cout % 32 == 0;
  if (sh->head_geom) sh->ks_max = std::max(sh->ks_max, (size_t)(KH / damc::HD_NEGK) * B * LH.cout);
  return true;
}

// y (B, ho, wo, cout) NHWC = conv(x3 limbs of x) + bias on the limb engine
// af32 != NULL: the input as fp32 NHWC, staged as fp32 and split into limbs in registers (X3_F32A; bitwise the limb
// input a3 = the RNE limbs of af32)
int enc_conv_x3(const unsigned short* a3, const float* af32, int B, int hin, int win, const damc_enc_layer_t& L,
                const void* w3, float* y, float* kslab, size_t kslab_floats, int* defer, hipStream_t s,
                float* in_part = nullptr, int* in_done = nullptr) {
  const int hout = (hin + 2 * L.pad - L.k) / L.stride + 1, wout = (win + 2 * L.pad - L.k) / L.stride + 1;
  damc::GemmArgs a;
  if (af32) {
    a.A = af32;
    a.a_f32 = 1;
  } else {
    a.A3 = a3;
  }
  a.Hin = hin;
  a.Win = win;
  a.Cg = L.cin;
  a.Hq = hout;
  a.Wq = wout;
  a.kw = L.k;
  a.stride = L.stride;
  a.pad_y = L.pad;
  a.pad_x = L.pad;
  a.B3 = static_cast<const unsigned short*>(w3);
  a.b_negblk = 1;  // damc::launch_split_x3_conv's layout (sign-alternating blocks)
  a.C = y;
  a.ldc = L.cout;
  a.M = B * hout * wout;
  a.N = L.cout;
  a.K = L.k * L.k * L.cin;
  a.k_per_z = a.K;
  a.bias = L.bias;
  a.bias_mod = L.cout;
  a.act = DAMC_ACT_NONE;
  a.kslab = kslab;
  a.kslab_floats = (long)kslab_floats;
  a.ksplit_deferred = defer;
  a.kwalk = damc::x3_conv_walk(L.k, L.cin);  // the weight operand's K order (every packer of it reads the same rule)
  if (in_part) {  // the norm's statistics in the epilogue where the launch allows (GemmArgs::in_part)
    a.in_part = in_part;
    a.in_hw = hout * wout;
    a.in_S = hout * wout / 256;
    a.in_done = in_done;
  }
  return damc::launch_gemm(a, damc::A_CONV, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "enc_conv",
                           2.0 * a.M * (double)L.cout * a.K, s);
}
}  // namespace

extern "C" int damc_x3_sign_block(void) { return damc::X3_NEGK; }

extern "C" int damc_x3_conv_walk(int k, int cin) { return damc::x3_conv_walk(k, cin); }

extern "C" size_t damc_conv2d_x3_bytes(int cout, int cin, int k) {
  if (cout <= 0 || cin <= 0 || k <= 0 || !damc::conv_kmajor_ok(cin) || cout % 8 != 0 || k * k > 32) return 0;
  return (size_t)cout * k * k * cin * 6;
}

extern "C" int damc_pack_conv2d_x3(const float* w, int cout, int cin, int k, void* w_x3, void* stream) {
  if (!w || !w_x3 || !damc_conv2d_x3_bytes(cout, cin, k)) return DAMC_ERR_ARG;
  return damc::launch_pack_conv_x3(w, cout, cin, k, static_cast<unsigned short*>(w_x3), as_stream(stream));
}

// one Conv2d + bias on the limb engine for the Q update's encoder forward (the training path keeps every conv output,
// so it runs the convs one by one): k4 s2 p1 layers stage their fp32 NHWC input directly (X3_F32A), other shapes split
// it into limbs in the workspace first; split-K slabs in the workspace where the output tiles would not fill the chip
extern "C" size_t damc_conv2d_x3_workspace_bytes(int B, int hin, int win, int cin, int cout, int k, int stride,
                                                 int pad) {
  if (B <= 0 || hin <= 0 || win <= 0 || stride <= 0 || pad < 0 || !damc_conv2d_x3_bytes(cout, cin, k)) return 0;
  const int hout = (hin + 2 * pad - k) / stride + 1, wout = (win + 2 * pad - k) / stride + 1;
  if (hout <= 0 || wout <= 0) return 0;
  const bool f32a = k == 4 && stride == 2 && pad == 1;
  const size_t a3 = f32a ? 0 : round256((size_t)B * hin * win * cin * 6);
  return a3 + round256((size_t)std::max<long>(damc::x3_ksplit_floats(B * hout * wout, cout, k * k * cin, 1), 1) * 4);
}

extern "C" int damc_conv2d_x3_nhwc(const float* x, int B, int hin, int win, int cin, const void* w_x3,
                                   const float* bias, int cout, int k, int stride, int pad, float* y, void* wsp,
                                   size_t wsb, void* stream) {
  const size_t need = damc_conv2d_x3_workspace_bytes(B, hin, win, cin, cout, k, stride, pad);
  if (!x || !w_x3 || !y || !need) return DAMC_ERR_ARG;
  if (!wsp || wsb < need) return DAMC_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  damc_enc_layer_t L{};
  L.cin = cin;
  L.cout = cout;
  L.k = k;
  L.stride = stride;
  L.pad = pad;
  L.bias = bias;
  const bool f32a = k == 4 && stride == 2 && pad == 1;
  char* base = static_cast<char*>(wsp);
  unsigned short* a3 = nullptr;
  size_t off = 0;
  if (!f32a) {
    a3 = reinterpret_cast<unsigned short*>(base);
    off = round256((size_t)B * hin * win * cin * 6);
    const int rc = damc::launch_split_x3(x, (long)B * hin * win * cin, a3, s);
    if (rc) return rc;
  }
  return enc_conv_x3(a3, f32a ? x : nullptr, B, hin, win, L, w_x3, y, reinterpret_cast<float*>(base + off),
                     (wsb - off) / 4, nullptr, s);
}

extern "C" size_t damc_q_encoder_workspace_bytes(const damc_encoder_t* e, int B) {
  EncShapes sh;
  if (!enc_shapes(e, B, &sh)) return 0;
  return 2 * round256(sh.act_max * 4) + round256(std::max<size_t>(sh.slab_max, 1) * 4) +
         round256(std::max<size_t>(sh.in_max, 1) * 4) + round256(sh.a3_max) + round256(sh.w3_max) +
         round256(sh.ks_max * 4) + sh.wsrc_bytes + 256;  // + the packing's status word (DAMC_ENC_PACK_CHECK)
}

// ---- damc_q_encoder_fwd's parts, in the order the call runs them
namespace {

// the call's workspace, in damc_q_encoder_workspace_bytes' order
struct EncWs {
  float* buf[2];       // ping-pong activations, NHWC fp32 (layer i reads buf[i & 1])
  float* slabs;        // the fp32 engine's split-K slabs
  float* inws;         // the norms' statistics partials, then their (scale, shift)
  unsigned short* a3;  // the current limb conv's input as limbs
  unsigned short* w3;  // the limb copy of a w_packed weight
  float* kslab;        // the limb engine's split-K slabs; the dense head's slabs
  char* wsrc;          // the w_src layers' limb operands (null without such a layer)
  int* pack_err;       // the packing's status word (DAMC_ENC_PACK_CHECK)
};
EncWs enc_carve(const EncShapes& sh, void* wsp) {
  char* base = reinterpret_cast<char*>(wsp);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += round256(bytes);
    return p;
  };
  EncWs ws;
  ws.buf[0] = reinterpret_cast<float*>(take(sh.act_max * 4));
  ws.buf[1] = reinterpret_cast<float*>(take(sh.act_max * 4));
  ws.slabs = reinterpret_cast<float*>(take(std::max<size_t>(sh.slab_max, 1) * 4));
  ws.inws = reinterpret_cast<float*>(take(std::max<size_t>(sh.in_max, 1) * 4));
  ws.a3 = reinterpret_cast<unsigned short*>(take(sh.a3_max));
  ws.w3 = reinterpret_cast<unsigned short*>(take(sh.w3_max));
  ws.kslab = reinterpret_cast<float*>(take(sh.ks_max * 4));
  ws.wsrc = sh.wsrc_bytes ? take(sh.wsrc_bytes) : nullptr;
  ws.pack_err = reinterpret_cast<int*>(take(256));
  return ws;
}

// the DAMC_ENC_* switches of one call, each read per call (tests and A/B runs flip them within a process); the stages
// take them as plain bools.  (DAMC_ENC_HEAD_PD and DAMC_ENC_HEAD_XCD are launch_dense_head_x3's own.)
struct EncSwitches {
  // DAMC_ENC_PACK_CHECK=1 (tests, never timed work): the packing workgroups report any workgroup outside their list in
  // a status word the call zeroes first and reads back at its end (one host sync), returning DAMC_ERR_UNSUPPORTED if
  // it was set
  bool pack_check;
  bool in_onepass;  // DAMC_ENC_IN_ONEPASS=0: the three-kernel norm where the one-pass norm would run
  bool head;        // DAMC_ENC_HEAD=0: the last conv on the limb GEMM over its packed weight limbs, not the dense head
  // DAMC_ENC_F32A=0: limbs throughout; else the k4 s2 p1 limb convs stage their input as fp32 (X3_F32A) where the norm
  // before them can write fp32
  bool f32a;
  // DAMC_ENC_IN_SLABS=0: the split-K reduce kernel writes C before a one-pass norm, which else sums the slabs itself
  bool in_slabs;
  // DAMC_ENC_IN_STRIP=0: in_stats_kernel's partition where the three-kernel norm would run on 256-pixel strips, its
  // statistics taken in the conv's epilogue (round 6; GemmArgs::in_part; in_strip_stats_kernel where the conv ran
  // split): the stats pass's read of the conv output is gone (CelebA-HQ B=64: 537 + 268 + 67 MB)
  bool in_strip;
  // layer 0 (read only where enc_first.hip runs it): DAMC_ENC_FIRST_ONEPASS=0 keeps the two recomputing passes,
  // DAMC_ENC_FIRST_MFMA=0 keeps them on the fmaf chain, DAMC_ENC_FIRST_PX=1 one pixel per lane in its statistics pass
  bool first_onepass, first_mfma, first_px1;
};
EncSwitches enc_switches(bool first_fused) {
  auto is = [](const char* name, char v) {
    const char* e = getenv(name);
    return e && e[0] == v;
  };
  EncSwitches sw{};
  sw.pack_check = is("DAMC_ENC_PACK_CHECK", '1');
  sw.in_onepass = !is("DAMC_ENC_IN_ONEPASS", '0');
  sw.head = !is("DAMC_ENC_HEAD", '0');
  sw.f32a = !is("DAMC_ENC_F32A", '0');
  sw.in_slabs = !is("DAMC_ENC_IN_SLABS", '0');
  sw.in_strip = !is("DAMC_ENC_IN_STRIP", '0');
  if (first_fused) {
    sw.first_onepass = !is("DAMC_ENC_FIRST_ONEPASS", '0');
    sw.first_mfma = !is("DAMC_ENC_FIRST_MFMA", '0');
    sw.first_px1 = is("DAMC_ENC_FIRST_PX", '1');
  }
  return sw;
}

// the w_src layers' limb operands as one packing list (it runs as extra workgroups of the one-pass first layer, else
// in a launch of its own); a layer the list cannot take is packed here, in a launch of its own.  With the dense head,
// the last layer is left out (the head reads the fp32 weight itself)
int enc_pack_list(const damc_encoder_t* e, const EncShapes& sh, bool head, char* wsrc, int* err,
                  damc::PackConvList* pl, hipStream_t s) {
  const int n = e->n_layers;
  for (int i = 0; i < n; ++i) {
    const damc_enc_layer_t& L = e->layers[i];
    if (!L.w_src || (head && i == n - 1)) continue;
    unsigned short* y = reinterpret_cast<unsigned short*>(wsrc + sh.wsrc_off[i]);
    if (pl->n < 8 && damc::pack_conv_x3_many_ok(L.w_src, L.cin, L.k)) {
      pl->w[pl->n] = L.w_src;
      pl->y[pl->n] = y;
      pl->cin[pl->n] = L.cin;
      pl->taps[pl->n] = L.k * L.k;
      pl->blk0[++pl->n] = L.cout;
    } else {
      const int rc = damc::launch_pack_conv_x3(L.w_src, L.cout, L.cin, L.k, y, s);
      if (rc) return rc;
    }
  }
  if (pl->n && damc::pack_conv_x3_many_prep(*pl)) return DAMC_ERR_UNSUPPORTED;
  pl->err = err;
  return 0;
}

// where a step left the next conv's input
enum EncFeed {
  FEED_NHWC,   // fp32 NHWC in buf[i & 1]; a limb conv splits it into a3 first
  FEED_LIMBS,  // a3 holds its limbs (written by the previous layer's norm)
  FEED_F32A,   // fp32 NHWC in buf[i & 1], which the limb conv stages itself (X3_F32A)
};

// layer i's conv from its input (feed) to out.  On the limb engine: defer, in_part and in_done as enc_conv_x3 takes
// them; the weight operand is the caller's w_x3, the call's packing of w_src, or a limb copy of w_packed made here
int enc_layer_conv(const damc_encoder_t* e, const EncShapes& sh, int i, int B, EncFeed feed, const EncWs& ws,
                   float* out, int* defer, float* in_part, int* in_done, void* stream) {
  const damc_enc_layer_t& L = e->layers[i];
  hipStream_t s = as_stream(stream);
  float* in = ws.buf[i & 1];
  int rc;
  if (!sh.limb[i]) {
    const size_t nsl = damc_conv2d_workspace_floats(B, sh.h[i], sh.w[i], L.cin, L.cout, L.k, L.stride, L.pad);
    return damc_conv2d_nhwc(in, B, sh.h[i], sh.w[i], L.cin, L.w_packed, L.bias, L.cout, L.k, L.stride, L.pad, out,
                            nsl ? ws.slabs : nullptr, nsl, stream);
  }
  if (feed == FEED_NHWC) {
    const long na = (long)B * sh.h[i] * sh.w[i] * L.cin;
    if ((rc = damc::launch_split_x3(in, na, ws.a3, s))) return rc;
  }
  const void* wl = L.w_x3 ? L.w_x3 : L.w_src ? static_cast<const void*>(ws.wsrc + sh.wsrc_off[i]) : nullptr;
  if (!wl) {  // the limb copy from the fp32 packing
    const int K = L.k * L.k * L.cin;
    if ((rc = damc::x3_conv_walk(L.k, L.cin)
                  ? damc::launch_split_x3_walk(L.w_packed, (long)L.cout * K, K, L.cin, ws.w3, s)
                  : damc::launch_split_x3_conv(L.w_packed, (long)L.cout * K, K, L.cin, ws.w3, s)))
      return rc;
    wl = ws.w3;
  }
  return enc_conv_x3(ws.a3, feed == FEED_F32A ? in : nullptr, B, sh.h[i], sh.w[i], L, wl, out, ws.kslab, sh.ks_max,
                     defer, s, in_part, in_done);
}

}  // namespace

// The steps: carve the workspace, read the switches, pack the w_src operands, layer 0, then per layer its conv and its
// norm, the last conv (the dense head where it fits), the packing's status word.
extern "C" int damc_q_encoder_fwd(const damc_encoder_t* e, const float* x, int B, float* xemb, void* wsp, size_t wsb,
                                  void* stream) {
  EncShapes sh;
  if (!x || !xemb || !enc_shapes(e, B, &sh)) return DAMC_ERR_ARG;
  const int n = e->n_layers;
  if (sh.h[n] != 1 || sh.w[n] != 1) return DAMC_ERR_UNSUPPORTED;  // NHWC flatten == NCHW flatten only at 1 x 1
  if (!wsp || wsb < damc_q_encoder_workspace_bytes(e, B)) return DAMC_ERR_WORKSPACE;
  const EncWs ws = enc_carve(sh, wsp);
  const EncSwitches sw = enc_switches(sh.first_fused);
  hipStream_t s = as_stream(stream);
  int rc;
  if (sw.pack_check && (rc = (int)hipMemsetAsync(ws.pack_err, 0, sizeof(int), s))) return rc;
  // the last conv as the dense head (enc_head_x3_kernel) where it fits; the norm before it is then the one-pass kernel,
  // which writes the head's CHW rows
  const bool head = sh.head_geom && sw.head && sw.in_onepass && (uintptr_t)xemb % 16 == 0;
  auto f32a_layer = [&](int i) {  // layer i is a limb conv that stages an fp32 input
    return sw.f32a && i < n && sh.limb[i] && e->layers[i].k == 4 && e->layers[i].stride == 2 && e->layers[i].pad == 1;
  };

  damc::PackConvList pl{};
  if (ws.wsrc && (rc = enc_pack_list(e, sh, head, ws.wsrc, sw.pack_check ? ws.pack_err : nullptr, &pl, s))) return rc;
  bool pl_done = pl.n == 0;

  EncFeed feed = FEED_NHWC;
  int i0 = 0;
  if (sh.first_fused) {  // layer 0: conv3 + InstanceNorm + LeakyReLU straight to layer 1's input
    float* y32 = f32a_layer(1) ? ws.buf[1] : nullptr;
    if ((rc = damc::launch_enc_first(e->layers[0], x, B, e->h, e->w, sh.first_rows, sh.first_strips, sw.first_onepass,
                                     sw.first_mfma, sw.first_px1, ws.inws, ws.a3, y32, pl, &pl_done, s)))
      return rc;
    feed = y32 ? FEED_F32A : FEED_LIMBS;
    i0 = 1;
  } else if ((rc = damc_nchw_to_nhwc(x, B, e->nc, e->h * e->w, ws.buf[0], stream))) {
    return rc;
  }
  if (!pl_done && (rc = damc::launch_pack_conv_x3_many(pl, s))) return rc;

  for (int i = i0; i < n; ++i) {
    const damc_enc_layer_t& L = e->layers[i];
    float* out = (i + 1 == n) ? xemb : ws.buf[(i + 1) & 1];
    const int hw = sh.h[i + 1] * sh.w[i + 1];
    if (head && i == n - 1) {  // its CHW rows are in buf[(i + 1) & 1] (written by the norm before it)
      if ((rc = damc::launch_dense_head_x3(ws.buf[(i + 1) & 1], L.w_src, L.bias, B, L.cout, L.cin * L.k * L.k,
                                           ws.kslab, sh.ks_max, xemb, s)))
        return rc;
      continue;
    }
    const bool next_limb = i + 1 < n && sh.limb[i + 1];  // the norm writes the next conv's input form
    // the norm after this conv is the one-pass kernel; it then also sums the conv's split-K slabs itself (ks_def)
    const bool in1 = L.in_gamma && next_limb && L.cout % 32 == 0 && hw <= 256 && sw.in_onepass;
    // or the three-kernel norm on 256-pixel strips, its statistics taken in the conv's epilogue (strip_done)
    const bool strip = L.in_gamma && !in1 && next_limb && L.cout % 8 == 0 && sh.limb[i] && hw % 256 == 0 &&
                       hw / 256 <= 64 && sw.in_strip;
    int strip_done = 1, ks_def = 0;
    if ((rc = enc_layer_conv(e, sh, i, B, feed, ws, out, (in1 && sw.in_slabs) ? &ks_def : nullptr,
                             strip ? ws.inws : nullptr, strip ? &strip_done : nullptr, stream)))
      return rc;
    feed = FEED_NHWC;
    if (!L.in_gamma) continue;
    if (in1) {
      // in place: the next conv's fp32 input; before the head: its CHW rows, into this layer's (consumed) input buffer
      const int chw = head && i + 2 == n;
      float* y32 = chw ? ws.buf[i & 1] : f32a_layer(i + 1) ? out : nullptr;
      if ((rc = damc::launch_in_onepass(L, out, B, hw, ws.a3, y32, chw, ws.kslab, ks_def, s))) return rc;
      feed = y32 ? FEED_F32A : FEED_LIMBS;
    } else if (next_limb && L.cout % 8 == 0) {
      const bool f32 = f32a_layer(i + 1);  // in place: the next conv's fp32 input
      if ((rc = damc::launch_in_threepass(L, out, B, hw, strip, strip_done != 0, ws.inws, ws.a3, f32, s))) return rc;
      feed = f32 ? FEED_F32A : FEED_LIMBS;
    } else if ((rc = damc_instnorm_lrelu_nhwc(out, B, hw, L.cout, L.in_gamma, L.in_beta, L.in_eps, L.slope, ws.inws,
                                              stream))) {
      return rc;
    }
  }
  if (sw.pack_check) {
    int flag = 0;
    if ((rc = (int)hipMemcpyAsync(&flag, ws.pack_err, sizeof(int), hipMemcpyDeviceToHost, s))) return rc;
    if ((rc = (int)hipStreamSynchronize(s))) return rc;
    if (flag) return DAMC_ERR_UNSUPPORTED;
  }
  return 0;
}
