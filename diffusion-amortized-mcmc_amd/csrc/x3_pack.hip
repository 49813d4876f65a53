// x3_pack.hip — the limb engine's operand producers: fp32 tensors split into the x3 limb layout (launch_split_x3*)
// and weights packed into the GEMM operands, fp32 and limbs in one pass (launch_pack_*).  The layout and the sign
// blocks are described in gemm_x3.hip; every split is split3_octet's.
#include <algorithm>

#include "gemm_impl.h"

namespace damc {

// fp32 [rows][C] -> x3 [rows][C/8][3][8]; one thread per channel octet
__global__ void split_x3_kernel(const float* __restrict__ x, long n8, unsigned short* __restrict__ y) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const f32x4 v0 = reinterpret_cast<const f32x4*>(x)[2 * i];
  const f32x4 v1 = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
  const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  bf16x8 h, m, l;
  split3_octet(v, h, m, l);
  bf16x8* o = reinterpret_cast<bf16x8*>(y) + 3 * i;
  o[0] = h;
  o[1] = m;
  o[2] = l;
}

// rows of K values; octets in odd negk-blocks of a row negated
__global__ void split_x3_negblk_kernel(const float* __restrict__ x, long n8, int K8, unsigned short* __restrict__ y,
                                       int negk) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const long k8 = i % K8;
  const float sg = ((k8 * 8 / negk) & 1) ? -1.f : 1.f;
  const f32x4 v0 = reinterpret_cast<const f32x4*>(x)[2 * i];
  const f32x4 v1 = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
  const float v[8] = {sg * v0.x, sg * v0.y, sg * v0.z, sg * v0.w, sg * v1.x, sg * v1.y, sg * v1.z, sg * v1.w};
  bf16x8 h, m, l;
  split3_octet(v, h, m, l);
  bf16x8* o = reinterpret_cast<bf16x8*>(y) + 3 * i;
  o[0] = h;
  o[1] = m;
  o[2] = l;
}

int launch_split_x3_negblk(const float* x, long n, int K, unsigned short* y, hipStream_t s, int negk) {
  if (K <= 0 || K % 8 != 0 || n % K != 0 || ((uintptr_t)x | (uintptr_t)y) % 16 != 0) return DAMC_ERR_ARG;
  const long n8 = n / 8;
  if (n8 == 0) return 0;
  hipLaunchKernelGGL(split_x3_negblk_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, n8, K / 8, y, negk);
  return (int)hipGetLastError();
}

// weight rows of K = taps * Cg values in tap-major order [tap][c] -> x3 in slice-major order
// [c / sw][tap][c % sw] (the slice-major K walk, GemmArgs::kwalk, of a ConvT phase's forward weights), odd negk-blocks
// of the new order negated
__global__ void split_x3_cmaj_kernel(const float* __restrict__ x, long n8, int K8, int Cg8, int taps, int sw8,
                                     unsigned short* __restrict__ y, int negk) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // source octet
  if (i >= n8) return;
  const long row = i / K8;
  const int k8 = (int)(i - row * K8);
  const int tp = k8 / Cg8, c8 = k8 - tp * Cg8;  // octet c8 of tap tp
  const int d8 = (c8 / sw8) * taps * sw8 + tp * sw8 + c8 % sw8;  // destination octet within the row
  const float sg = ((d8 * 8 / negk) & 1) ? -1.f : 1.f;
  const f32x4 v0 = reinterpret_cast<const f32x4*>(x)[2 * i];
  const f32x4 v1 = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
  const float v[8] = {sg * v0.x, sg * v0.y, sg * v0.z, sg * v0.w, sg * v1.x, sg * v1.y, sg * v1.z, sg * v1.w};
  bf16x8 h, m, l;
  split3_octet(v, h, m, l);
  bf16x8* o = reinterpret_cast<bf16x8*>(y) + 3 * (row * K8 + d8);
  o[0] = h;
  o[1] = m;
  o[2] = l;
}

int launch_split_x3_cmaj(const float* x, long n, int K, int Cg, int sw, unsigned short* y, hipStream_t s, int negk) {
  if (K <= 0 || Cg <= 0 || sw <= 0 || sw % 8 != 0 || Cg % sw != 0 || K % Cg != 0 || n % K != 0 ||
      ((uintptr_t)x | (uintptr_t)y) % 16 != 0)
    return DAMC_ERR_ARG;
  const long n8 = n / 8;
  if (n8 == 0) return 0;
  hipLaunchKernelGGL(split_x3_cmaj_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, n8, K / 8, Cg / 8,
                     K / Cg, sw / 8, y, negk);
  return (int)hipGetLastError();
}

// rows of K = 16 Cg values in tap-major order [tap][c] -> x3 in the 4 x 4 conv walk (x3_conv_walk: [c / 32][x3_walk_pos
// (tap)][c % 32]), sign blocks counted in the walk order
__global__ void split_x3_walk_kernel(const float* __restrict__ x, long n8, int K8, int Cg8,
                                     unsigned short* __restrict__ y, int negk) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // source octet
  if (i >= n8) return;
  const long row = i / K8;
  const int k8 = (int)(i - row * K8);
  const int tp = k8 / Cg8, c = (k8 - tp * Cg8) * 8;
  const int kk = (c >> 5) * 16 * 32 + x3_walk_pos(tp) * 32 + (c & 31);
  const float sg = ((kk / negk) & 1) ? -1.f : 1.f;
  const f32x4 v0 = reinterpret_cast<const f32x4*>(x)[2 * i];
  const f32x4 v1 = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
  const float v[8] = {sg * v0.x, sg * v0.y, sg * v0.z, sg * v0.w, sg * v1.x, sg * v1.y, sg * v1.z, sg * v1.w};
  bf16x8 h, m, l;
  split3_octet(v, h, m, l);
  bf16x8* o = reinterpret_cast<bf16x8*>(y) + 3 * (row * K8 + (kk >> 3));
  o[0] = h;
  o[1] = m;
  o[2] = l;
}

int launch_split_x3_walk(const float* x, long n, int K, int Cg, unsigned short* y, hipStream_t s, int negk) {
  if (Cg <= 0 || Cg % 32 != 0 || K != 16 * Cg || n % K != 0 || ((uintptr_t)x | (uintptr_t)y) % 16 != 0)
    return DAMC_ERR_ARG;
  const long n8 = n / 8;
  if (n8 == 0) return 0;
  hipLaunchKernelGGL(split_x3_walk_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, n8, K / 8, Cg / 8,
                     y, negk);
  return (int)hipGetLastError();
}

int launch_split_x3_conv(const float* x, long n, int K, int Cg, unsigned short* y, hipStream_t s, int negk) {
  return launch_split_x3_negblk(x, n, K, y, s, negk);
}

// ---- generator-layer weight packing through LDS tiles (damc_pack_generator_layer's hot layouts): a ConvTranspose2d
// weight W[ci][co][tap] (kk <= 16 taps) read in contiguous rows, written as whole octets of the packed matrix, with
// its x3 copy (sign-alternating negk blocks, split_x3_negblk_kernel's values) in the same pass -- the per-call
// packing was scattered 4-byte stores plus a second read for the limb split.
// (flat: fp32 index; the limb octet goes to x3 octet x3_oct, k = its K index within the row in the limb copy's order)
__device__ __forceinline__ void pack_store_octet(const float (&v)[8], long flat, long x3_oct, int k,
                                                 float* __restrict__ out, unsigned short* __restrict__ x3, int negk) {
  f32x4* o = reinterpret_cast<f32x4*>(out + flat);
  o[0] = f32x4{v[0], v[1], v[2], v[3]};
  o[1] = f32x4{v[4], v[5], v[6], v[7]};
  if (x3) {
    const float sg = ((k / negk) & 1) ? -1.f : 1.f;
    const float u[8] = {sg * v[0], sg * v[1], sg * v[2], sg * v[3], sg * v[4], sg * v[5], sg * v[6], sg * v[7]};
    bf16x8 h, m, l;
    split3_octet(u, h, m, l);
    bf16x8* y = reinterpret_cast<bf16x8*>(x3) + 3 * x3_oct;
    y[0] = h;
    y[1] = m;
    y[2] = l;
  }
}

// out[ci][tap][co] = W[ci][co][tap]; x3 rows ci of K = kk * cout. Block: one ci, 128 output channels (kk <= 64).
constexpr int PK_ROW_CO = 128;
__global__ void __launch_bounds__(256) pack_rowT_kernel(const float* __restrict__ w, int cout, int kk,
                                                        float* __restrict__ out, unsigned short* __restrict__ x3,
                                                        int negk, int walk) {
  __shared__ float t[PK_ROW_CO * 65];
  const int ci = blockIdx.y, co0 = blockIdx.x * PK_ROW_CO;
  const int nco = min(PK_ROW_CO, cout - co0), nco8 = nco / 8, ld = kk + 1;
  const float* src = w + ((long)ci * cout + co0) * kk;
  for (int e = threadIdx.x; e < nco * kk; e += 256) t[(e / kk) * ld + e % kk] = src[e];
  __syncthreads();
  for (int o = threadIdx.x; o < kk * nco8; o += 256) {
    const int tap = o / nco8, c8 = o - tap * nco8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t[(c8 * 8 + j) * ld + tap];
    const int co = co0 + c8 * 8, k = tap * cout + co;
    // limb copy in the x3_conv_walk order (walk: the 4 x 4 input gradient, x3_up2_walk): [co / 32][walk pos][co % 32]
    const int k3 = walk ? (co >> 5) * (16 * 32) + x3_walk_pos(tap) * 32 + (co & 31) : k;
    pack_store_octet(v, (long)ci * kk * cout + k, ((long)ci * kk * cout + k3) / 8, k3, out, x3, negk);
  }
}

// out[seg][ci] with seg(co, tap) = the ConvT forward row order: UP2 ((phase * cout + co) * 4 + ty * 2 + tx, x3 rows
// of 4 Cin per (phase, co)), PROJ (tap * cout + co, x3 rows of Cin). Block: 32 input x 128 / kk output channels (each
// input channel's run of 128 contiguous weights).
__global__ void __launch_bounds__(256) pack_colT_kernel(const float* __restrict__ w, int cin, int cout, int kk, int up2,
                                                        float* __restrict__ out, unsigned short* __restrict__ x3,
                                                        int negk, int walk) {
  __shared__ float t[32 * 129];
  const int cot = 128 / kk, ci0 = blockIdx.x * 32, co0 = blockIdx.y * cot, rl = 128, ld = rl + 1;
  for (int e = threadIdx.x; e < 32 * rl; e += 256) {
    const int cl = e / rl, r = e - cl * rl;
    t[cl * ld + r] = w[((long)(ci0 + cl) * cout + co0) * kk + r];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < rl * 4; o += 256) {
    const int c8 = o & 3, r = o >> 2, col = r / kk, tap = r - col * kk, co = co0 + col;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t[(c8 * 8 + j) * ld + r];
    long seg, oct3;
    int k = ci0 + c8 * 8;
    if (up2) {  // ky = 3 - py - 2 ty (the stride-2 phase decomposition, generator.hip pack_up2_kernel)
      const int ky = tap >> 2, kx = tap & 3, py = (3 - ky) & 1, px = (3 - kx) & 1;
      const int tt = ((3 - ky - py) >> 1) * 2 + ((3 - kx - px) >> 1);
      seg = ((long)(py * 2 + px) * cout + co) * 4 + tt;
      // limb copy slice-major (walk, x3_up2_walk): the (phase, co) row's 4 cin values as [c / 32][tap][c % 32]
      // (launch_split_x3_cmaj's order, sw = 32); ci0 is a whole slice
      k = walk ? (ci0 >> 5) * 128 + tt * 32 + c8 * 8 : k + tt * cin;
      oct3 = ((seg - tt) * cin + k) / 8;
    } else {
      seg = (long)tap * cout + co;
      oct3 = (seg * cin + ci0 + c8 * 8) / 8;
    }
    pack_store_octet(v, seg * cin + ci0 + c8 * 8, oct3, k, out, x3, negk);
  }
}

static bool pack_tiled_ok(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) % 16) == 0;
}

// 1 = layout not covered (the caller packs element-wise)
int launch_pack_up2_tiled(const float* w, int cin, int cout, float* wf, unsigned short* wf3, float* wb,
                          unsigned short* wb3, hipStream_t s, int negk_f, int negk_b) {
  if (cin % KM_BK != 0 || cout % KM_BK != 0 || !pack_tiled_ok(wf, wf3, wb, wb3)) return 1;
  hipLaunchKernelGGL(pack_colT_kernel, dim3(cin / 32, cout / 8), dim3(256), 0, s, w, cin, cout, 16, 1, wf, wf3, negk_f,
                     x3_up2_walk(cin));
  hipLaunchKernelGGL(pack_rowT_kernel, dim3((cout + PK_ROW_CO - 1) / PK_ROW_CO, cin), dim3(256), 0, s, w, cout, 16,
                     wb, wb3, negk_b, x3_up2_walk(cout));
  return (int)hipGetLastError();
}

int launch_pack_proj_tiled(const float* w, int cin, int cout, int kk, float* wf, float* wb, unsigned short* wb3,
                           hipStream_t s) {
  if (kk > 64 || 128 % kk != 0 || cin % 32 != 0 || cout % 8 != 0 || cout % (128 / kk) != 0 ||
      !pack_tiled_ok(wf, wb, wb3, nullptr))
    return 1;
  hipLaunchKernelGGL(pack_rowT_kernel, dim3((cout + PK_ROW_CO - 1) / PK_ROW_CO, cin), dim3(256), 0, s, w, cout, kk,
                     wf, (unsigned short*)nullptr, X3_NEGK, 0);
  hipLaunchKernelGGL(pack_colT_kernel, dim3(cin / 32, cout / (128 / kk)), dim3(256), 0, s, w, cin, cout, kk, 0, wb, wb3,
                     X3_NEGK, 0);
  return (int)hipGetLastError();
}

// a PyTorch Conv2d weight (cout, cin, k, k) straight to the limb engine's B operand of the conv, [co][(ky, kx, ci)]
// with sign-alternating blocks (launch_split_x3_negblk of damc_pack_conv2d's K-major packing, in one pass)
__global__ void pack_conv_x3_kernel(const float* __restrict__ w, int cout, int cin, int k, unsigned short* __restrict__ y) {
  const int K = k * k * cin, K8 = K / 8;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)cout * K8) return;
  const int co = (int)(i / K8), k8 = (int)(i - (long)co * K8);
  const int kk = k8 * 8, tap = kk / cin, ci0 = kk - tap * cin;  // cin % 8 == 0: an octet never straddles a tap
  const float sg = ((kk / X3_NEGK) & 1) ? -1.f : 1.f;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = sg * w[((long)co * cin + ci0 + e) * k * k + tap];
  bf16x8 h, m, l;
  split3_octet(v, h, m, l);
  bf16x8* o = reinterpret_cast<bf16x8*>(y) + 3 * i;
  o[0] = h;
  o[1] = m;
  o[2] = l;
}

// the same packing, one thread per (co, input-channel octet): its 8 channels' k*k taps are 8 * k * k contiguous
// floats of the PyTorch layout, read 4 taps at a time as f32x4 (k * k % 4 == 0); adjacent threads write adjacent
// 48-B limb octets of each tap (the thread-per-output-octet kernel above reads 4 B at a 64-B stride, every line 16x)
__global__ void pack_conv_x3_taps_kernel(const float* __restrict__ w, int cout, int cin, int k,
                                         unsigned short* __restrict__ y, int walk) {
  // one thread per (co, 4-tap group, channel octet), octets fastest: 4x the threads of one per (co, octet) walking
  // all its taps (CIFAR encoder: 4 launches 69 -> ~25 us per Q(x) call), same values and stores
  const int cin8 = cin / 8, taps = k * k, K8 = taps * cin8, tq = taps / 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)cout * tq * cin8) return;
  const int c8 = (int)(i % cin8);
  const long r = i / cin8;
  const int t0 = 4 * (int)(r % tq), co = (int)(r / tq);
  const f32x4* src = reinterpret_cast<const f32x4*>(w + ((long)co * cin + c8 * 8) * taps);
  bf16x8* o = reinterpret_cast<bf16x8*>(y) + 3L * co * K8;
  f32x4 q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = src[(e * taps + t0) / 4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = c8 * 8;  // the octet's K index in the GEMM's walk (x3_conv_walk), which also sets its sign block
    const int kk = walk ? (c >> 5) * taps * 32 + x3_walk_pos(t0 + t) * 32 + (c & 31) : (t0 + t) * cin + c;
    const float sg = ((kk / X3_NEGK) & 1) ? -1.f : 1.f;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = sg * q[e][t];
    bf16x8 h, m, l;
    split3_octet(v, h, m, l);
    bf16x8* d = o + 3L * (kk >> 3);
    d[0] = h;
    d[1] = m;
    d[2] = l;
  }
}

// the same packing through LDS, one workgroup per (layer, co, chunk of CC input channels) (pack_conv_x3_block, gemm.h):
// every byte is read and written once, in full lines (the tap-group kernel below reads each 64-B line from 4 waves
// far apart).  Several layers share one launch (the encoder's per-call packing: one dispatch instead of one per layer)
__global__ __launch_bounds__(256) void pack_conv_x3_lds_kernel(PackConvList l) {
  extern __shared__ float pk_t[];  // [CC][taps + 1]
  pack_conv_x3_block(l, blockIdx.x, threadIdx.x, 256, pk_t);
}

bool pack_conv_x3_many_ok(const float* w, int cin, int k) {
  return k > 0 && k * k <= 32 && (uintptr_t)w % 16 == 0 && (cin % 128 == 0 || cin == 64);
}

int pack_conv_x3_many_prep(PackConvList& l) {
  if (l.ready || l.n < 1 || l.n > 8) return 1;
  size_t sm = 0;
  l.blk0[0] = 0;
  for (int i = 0; i < l.n; ++i) {
    if (l.taps[i] <= 0 || l.taps[i] > 32 || (uintptr_t)l.w[i] % 16 || (uintptr_t)l.y[i] % 16 ||
        !(l.cin[i] % 128 == 0 || l.cin[i] == 64) || l.blk0[i + 1] <= 0)
      return 1;
    l.cc[i] = l.cin[i] % 128 == 0 ? 128 : 64;
    l.walk[i] = l.taps[i] == 16 ? x3_conv_walk(4, l.cin[i]) : 0;
    sm = std::max(sm, (size_t)l.cc[i] * (l.taps[i] + 1) * sizeof(float));
  }
  for (int i = 0; i < l.n; ++i) {
    l.cout[i] = l.blk0[i + 1];
    l.blk0[i + 1] = l.blk0[i] + l.blk0[i + 1] * (l.cin[i] / l.cc[i]);
  }
  // the grid is exactly the work list: one workgroup per (layer, co, channel chunk), nothing more
  long total = 0;
  for (int i = 0; i < l.n; ++i) total += (long)l.cout[i] * (l.cin[i] / l.cc[i]);
  if (total != l.blk0[l.n]) return 1;
  l.lds = (int)sm;
  l.ready = 1;
  return 0;
}

int launch_pack_conv_x3_many(PackConvList l, hipStream_t s) {
  if (!l.ready && pack_conv_x3_many_prep(l)) return 1;
  hipLaunchKernelGGL(pack_conv_x3_lds_kernel, dim3((unsigned)l.blk0[l.n]), dim3(256), (size_t)l.lds, s, l);
  return (int)hipGetLastError();
}

int launch_pack_conv_x3(const float* w, int cout, int cin, int k, unsigned short* y, hipStream_t s) {
  if (cout <= 0 || cin % 8 != 0 || k <= 0 || (uintptr_t)y % 16 != 0) return DAMC_ERR_ARG;
  static const bool lds = [] {  // DAMC_PACK_CONV_LDS=0: the tap-group kernel below (A/B)
    const char* e = getenv("DAMC_PACK_CONV_LDS");
    return !(e && e[0] == '0');
  }();
  const int taps = k * k;
  if (lds && pack_conv_x3_many_ok(w, cin, k)) {
    PackConvList l{};
    l.n = 1;
    l.w[0] = w;
    l.y[0] = y;
    l.cin[0] = cin;
    l.taps[0] = taps;
    l.blk0[1] = cout;
    return launch_pack_conv_x3_many(l, s);
  }
  if ((k * k) % 4 == 0 && (uintptr_t)w % 16 == 0) {
    const long nt = (long)cout * (k * k / 4) * (cin / 8);
    hipLaunchKernelGGL(pack_conv_x3_taps_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, w, cout, cin, k,
                       y, x3_conv_walk(k, cin));
    return (int)hipGetLastError();
  }
  if (x3_conv_walk(k, cin)) return DAMC_ERR_UNSUPPORTED;  // (k = 4: the taps kernel above always takes it)
  const long n = (long)cout * k * k * cin / 8;
  hipLaunchKernelGGL(pack_conv_x3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, cout, cin, k, y);
  return (int)hipGetLastError();
}

int launch_split_x3(const float* x, long n, unsigned short* y, hipStream_t s) {
  if (n % 8 != 0 || ((uintptr_t)x | (uintptr_t)y) % 16 != 0) return DAMC_ERR_ARG;
  const long n8 = n / 8;
  if (n8 == 0) return 0;
  hipLaunchKernelGGL(split_x3_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, n8, y);
  return (int)hipGetLastError();
}

}  // namespace damc
