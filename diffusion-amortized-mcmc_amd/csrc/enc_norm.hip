// enc_norm.hip — the encoder's InstanceNorm2d(affine, eps) + LeakyReLU on NHWC activations (encoder.hip has the
// forward that calls it).  Statistics are per (sample, channel) Welford partials merged with Chan's formula (wave
// shuffles + LDS).  Three groups of kernels:
//   - the per-op call (damc_instnorm_lrelu_nhwc): in_stats_pivot_kernel, in_apply_kernel, in place, InstanceNorm's
//     own operation order;
//   - the forward's limb-writing forms, whose output is the next convolution's input (its limbs, or fp32 for an F32A
//     conv): in_fused_x3_kernel in one pass (launch_in_onepass), and in_stats_kernel or in_strip_stats_kernel,
//     in_merge_kernel, in_apply_x3_kernel or in_apply_f32_kernel (launch_in_threepass); in_merge_kernel also serves
//     the first layer's two-pass forms (launch_in_merge, called from enc_first.hip);
//   - the Q update's training forward and backward (damc_instnorm_lrelu_train_nhwc,
//     damc_instnorm_lrelu_backward_nhwc).
// Shares with the other encoder files (enc_impl.h): Wf / wmerge, wave_rsum, in_splits.
#include <algorithm>

#include "enc_impl.h"
#include "wgrad.h"

using damc::in_splits;
using damc::wave_rsum;
using damc::Wf;
using damc::wmerge;

namespace {

// grid: (B * ceil(C/64), S); block 256 = 64 channels x 4 pixel lanes
// PIVOT (the per-op norm calls): the statistics of y - K with K = the (sample, channel)'s first pixel, stored in
// piv[b * C + c]; the partial means are then of the data's spread, not its offset, so neither the running mean of a
// chain nor the difference of two partial means in wmerge rounds at |mean| (rstd 2.3e-6 from fp64 at |mean| = 1000 std
// without it).  The consumer adds K back to the merged mean.  PIVOT = false keeps the absolute frame (piv unused)
template <bool PIVOT>
__device__ __forceinline__ void in_stats_body(const float* y, int B, int HW, int C, int S, float* part, float* piv) {
  const int cg = (C + 63) / 64;
  const int b = blockIdx.x / cg, c = (blockIdx.x % cg) * 64 + (threadIdx.x & 63);
  const int prow = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int p0 = (int)((long)HW * s / S), p1 = (int)((long)HW * (s + 1) / S);
  Wf w{0.f, 0.f, 0.f};
  float K = 0.f;
  if (PIVOT && c < C) {
    K = y[(long)b * HW * C + c];
    if (s == 0 && prow == 0) piv[(long)b * C + c] = K;
  }
  if (c < C) {
    // four loads in flight, then their updates in pixel order (the same Welford chain as one at a time)
    int p = p0 + prow;
    for (; p + 12 < p1; p += 16) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = y[((long)b * HW + p + 4 * u) * C + c];
      if (PIVOT) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __fsub_rn(v[u], K);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        w.n += 1.f;
        const float d = v[u] - w.mean;
        w.mean += d / w.n;
        w.m2 += d * (v[u] - w.mean);
      }
    }
    for (; p < p1; p += 4) {
      float v = y[((long)b * HW + p) * C + c];
      if (PIVOT) v = __fsub_rn(v, K);
      w.n += 1.f;
      const float d = v - w.mean;
      w.mean += d / w.n;
      w.m2 += d * (v - w.mean);
    }
  }
  __shared__ Wf red[4][64];
  red[prow][threadIdx.x & 63] = w;
  __syncthreads();
  if (prow == 0 && c < C) {
    Wf a = red[0][threadIdx.x];
    for (int r = 1; r < 4; ++r) a = wmerge(a, red[r][threadIdx.x]);
    float* o = part + (((long)b * C + c) * S + s) * 3;
    o[0] = a.n;
    o[1] = a.mean;
    o[2] = a.m2;
  }
}
__global__ __launch_bounds__(256) void in_stats_kernel(const float* y, int B, int HW, int C, int S, float* part) {
  in_stats_body<false>(y, B, HW, C, S, part, nullptr);
}
__global__ __launch_bounds__(256) void in_stats_pivot_kernel(const float* y, int B, int HW, int C, int S, float* part,
                                                             float* piv) {
  in_stats_body<true>(y, B, HW, C, S, part, piv);
}

// grid: (B * ceil(C/64), P); merges the S partials of its 64 channels (in_stats_pivot_kernel's, relative to piv),
// then normalises its pixels
__global__ __launch_bounds__(256) void in_apply_kernel(float* y, int B, int HW, int C, int S, const float* part,
                                                       const float* piv, const float* gamma, const float* beta,
                                                       float eps, float slope) {
  const int cg = (C + 63) / 64;
  const int b = blockIdx.x / cg, c = (blockIdx.x % cg) * 64 + (threadIdx.x & 63);
  const int prow = threadIdx.x >> 6;
  __shared__ float sc[64], sh[64];
  if (prow == 0) {
    float scale = 0.f, shift = 0.f;
    if (c < C) {
      const float* pp = part + ((long)b * C + c) * S * 3;
      Wf a{pp[0], pp[1], pp[2]};
      for (int s = 1; s < S; ++s) a = wmerge(a, Wf{pp[3 * s], pp[3 * s + 1], pp[3 * s + 2]});
      const float var = a.m2 / a.n;  // biased, as InstanceNorm2d
      scale = 1.f / sqrtf(var + eps);
      shift = __fadd_rn(piv[(long)b * C + c], a.mean);
    }
    sc[threadIdx.x] = scale;
    sh[threadIdx.x] = shift;
  }
  __syncthreads();
  if (c >= C) return;
  // a = ((y - mean) * rstd) * gamma + beta, InstanceNorm's own order and in_apply_train_kernel's bits: the fused
  // y * (rstd * gamma) + (beta - mean * rstd * gamma) rounds the shift at |mean| * rstd * |gamma|, which is far above
  // the output when |mean| >> std (a constant channel, hw = 1, or data riding on a large offset)
  const float rstd = sc[threadIdx.x & 63], mean = sh[threadIdx.x & 63], g = gamma[c], bt = beta[c];
  const int P = gridDim.y;
  const int p0 = (int)((long)HW * blockIdx.y / P), p1 = (int)((long)HW * (blockIdx.y + 1) / P);
  for (int p = p0 + prow; p < p1; p += 4) {
    float* q = y + ((long)b * HW + p) * C + c;
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(*q, mean), rstd), g), bt);
    *q = v > 0.f ? v : v * slope;
  }
}

// (scale, shift) of every (sample, channel) from the S statistics partials, merged once (in_apply_kernel's merge,
// same order): ss [B][2][C]
// one wave per (sample, channel): lane s loads strip s (one coalesced 12-B record per lane; S <= 64), and the strips
// merge as a fixed pairwise tree over lanes (strides 1, 2, 4, ...; an empty lane is an exact identity of wmerge).
// Round 5's one-thread-per-(sample, channel) left fold issued S dependent merges behind S scattered loads: 22 us per
// CelebA-HQ B=8 layer for 1024 threads (profiles/r06/enc_hq_b8_dispatches.txt).  The tree depends on S alone, which
// depends on the map size alone (in_splits), so a batch sharded over ranks merges exactly as the whole batch.
__global__ __launch_bounds__(256) void in_merge_kernel(const float* __restrict__ part, int B, int C, int S,
                                                       const float* gamma, const float* beta, float eps,
                                                       float* __restrict__ ss) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= B * C) return;  // wave-uniform
  const int b = i / C, c = i - b * C;
  Wf a{0.f, 0.f, 0.f};
  if (lane < S) {
    const float* pp = part + ((long)i * S + lane) * 3;
    a = Wf{pp[0], pp[1], pp[2]};
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const Wf o{__shfl_down(a.n, off), __shfl_down(a.mean, off), __shfl_down(a.m2, off)};
    if ((lane & (2 * off - 1)) == 0) a = wmerge(a, o);
  }
  if (lane != 0) return;
  const float var = a.m2 / a.n;
  const float rstd = 1.f / sqrtf(var + eps);
  const float scale = rstd * gamma[c];
  ss[(long)b * 2 * C + c] = scale;
  ss[(long)b * 2 * C + C + c] = beta[c] - a.mean * scale;
}

// the norm statistics of the 256-pixel strips (GemmArgs::in_part's partition and arithmetic: damc::strip256_stats)
// from the stored conv output, for a conv whose launch could not take them in its epilogue (split-K at a small batch):
// grid (HW / 256 strips, B, ceil(C / 128)), 512 threads; part as in_stats_kernel's with S = HW / 256
__global__ __launch_bounds__(512) void in_strip_stats_kernel(const float* __restrict__ y, int HW, int C, float* part) {
  __shared__ float red[1024];
  const int sp = blockIdx.x, b = blockIdx.y, c0 = blockIdx.z * 128, tid = threadIdx.x;
  const int S = HW >> 8;
  float st[3];
  damc::strip256_stats(y + ((long)b * HW + 256L * sp) * C + c0, C, tid, c0 + (tid & 127) < C, red, st);
  if (tid < 128 && c0 + tid < C) {
    float* o = part + (((long)b * C + c0 + tid) * S + sp) * 3;
    o[0] = st[0];
    o[1] = st[1];
    o[2] = st[2];
  }
}

// in_apply_x3_kernel's fp32 in-place form one channel quad per thread (round 6, late): the same fmaf and LReLU per
// element, and every load / store instruction covers 1 KB without gaps (the octet form's pair of 16-B accesses per
// lane half-covers two 2 KB spans)
__global__ __launch_bounds__(256) void in_apply_f32_kernel(float* y, long n4, int HW, int C,
                                                           const float* __restrict__ ss, float slope) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const int C4 = C / 4;
  const long pix = i / C4;
  const int c0 = (int)(i - pix * C4) * 4;
  const int b = (int)(pix / HW);
  const float* sc = ss + (long)b * 2 * C + c0;
  f32x4 v = *reinterpret_cast<const f32x4*>(y + 4 * i);
  const f32x4 a = *reinterpret_cast<const f32x4*>(sc), h = *reinterpret_cast<const f32x4*>(sc + C);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = fmaf(v[e], a[e], h[e]);
    v[e] = t > 0.f ? t : t * slope;
  }
  *reinterpret_cast<f32x4*>(y + 4 * i) = v;
}

// the normalise + affine + LeakyReLU as one fmaf on in_merge_kernel's (scale, shift) (in_apply_kernel, the per-op call,
// keeps InstanceNorm's own operation order instead), written as the next convolution's limbs (x3
// octets) instead of fp32 in place: the limb engine reads nothing else.  One thread per (pixel, channel octet).
// y32 != NULL: fp32 in place instead (y32 == y; every thread rewrites only the octet it read), for a next conv that
// stages its input as fp32 (gemm_x3.hip X3_F32A)
__global__ __launch_bounds__(256) void in_apply_x3_kernel(const float* y, long n8, int HW, int C,
                                                          const float* __restrict__ ss, float slope,
                                                          unsigned short* __restrict__ y3, float* y32) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const int C8 = C / 8;
  const long pix = i / C8;
  const int c0 = (int)(i - pix * C8) * 8;
  const int b = (int)(pix / HW);
  const float* sc = ss + (long)b * 2 * C + c0;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(y + 8 * i), v1 = *reinterpret_cast<const f32x4*>(y + 8 * i + 4);
  const f32x4 a0 = *reinterpret_cast<const f32x4*>(sc), a1 = *reinterpret_cast<const f32x4*>(sc + 4);
  const f32x4 h0 = *reinterpret_cast<const f32x4*>(sc + C), h1 = *reinterpret_cast<const f32x4*>(sc + C + 4);
  float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  const float sa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const float sb[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = fmaf(v[e], sa[e], sb[e]);
    v[e] = t > 0.f ? t : t * slope;
  }
  if (y32) {
    *reinterpret_cast<f32x4*>(y32 + 8 * i) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(y32 + 8 * i + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    damc::store_x3_octet(v, y3 + 24 * i);
  }
}

// InstanceNorm + LeakyReLU of a stored conv output (NHWC fp32) to the next convolution's limbs in ONE kernel when a
// sample has <= 256 pixels (the encoder's k4 s2 layers at 32x32 input): grid (B, C / 32), 256 threads = 64 pixel slots
// x 4 channel octets, NIT = ceil(HW / 64) pixels per thread held in registers.  Sum, then sum of squared deviations
// (two passes over registers; wave reduce-scatter + fixed-order wave sums), then in_merge_kernel's scale / shift and
// in_apply_x3_kernel's normalise + LReLU + limb store.  Replaces in_stats + in_merge + in_apply_x3 (one read of the
// activation instead of two, one launch instead of three).
template <int NIT>
// y32 != NULL: the result leaves as fp32 NHWC at y32 instead of limbs (the next conv stages it as fp32, gemm_x3.hip
// X3_F32A); y32 may be y itself (every thread writes only the elements it read, after both block sums); chw: fp32 in
// CHW order per sample instead (the dense head's input; y32 must then be another buffer)
// slab != NULL: y was not written; the conv's ks split-K slabs (register layout of the 256 x 128 limb tiles, as
// x3_ksplit_reduce_tile_kernel reads them, sstride4 f32x4 per slab, ntn 128-channel tiles) are summed here in the
// reduce's order from 0, then the conv bias added: the reduce + epilogue's arithmetic, so the values are bitwise C's
__global__ __launch_bounds__(256) void in_fused_x3_kernel(const float* y, int HW, int C,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, float slope, unsigned short* __restrict__ y3,
                                                          float* y32, const float* __restrict__ slab, int ks, int ntn,
                                                          long sstride4, const float* __restrict__ cbias, int chw) {
  __shared__ float red[4][32];
  __shared__ float st[2][32];
  const int b = blockIdx.x, c0 = blockIdx.y * 32, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pr = tid >> 2, q = tid & 3;
  float v[NIT][8];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int p = pr + 64 * it;
    if (p < HW && slab) {
      const long m = (long)b * HW + p;
      const int n = c0 + 8 * q, rm = (int)(m & 255), rn = n & 127;
      const long tile = (m >> 8) * ntn + (n >> 7);
      const int wv = (rm >> 6) * 2 + (rn >> 6), ij = ((rm & 63) >> 4) * 4 + ((rn & 63) >> 4);
      const long base = ((tile * 8 + wv) * 16 + ij) * 64 + ((rm & 15) >> 2) * 16 + (rn & 15);  // f32x4 of element 0
      const int r = rm & 3;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[it][e] = 0.f;
      int sl = 0;
      for (; sl + 2 <= ks; sl += 2) {  // two slabs' 16 loads in flight, then their adds in slab order
        const float* s0 = slab + ((long)sl * sstride4 + base) * 4 + r;
        const float* s1 = s0 + sstride4 * 4;
        float t0[8], t1[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          t0[e] = s0[4 * e];
          t1[e] = s1[4 * e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[it][e] += t0[e];
          v[it][e] += t1[e];
        }
      }
      for (; sl < ks; ++sl) {
        const float* src = slab + ((long)sl * sstride4 + base) * 4 + r;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[it][e] += src[4 * e];
      }
      if (cbias) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[it][e] += cbias[n + e];
      }
    } else if (p < HW) {
      const float* src = y + ((long)b * HW + p) * C + c0 + 8 * q;
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(src), a1 = *reinterpret_cast<const f32x4*>(src + 4);
      v[it][0] = a0.x; v[it][1] = a0.y; v[it][2] = a0.z; v[it][3] = a0.w;
      v[it][4] = a1.x; v[it][5] = a1.y; v[it][6] = a1.z; v[it][7] = a1.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[it][e] = 0.f;
    }
  }
  // per-channel workgroup sum of t[e] (channel c0 + 8 q + e) into st[k]
  auto block_sum = [&](const float (&t)[8], int k) {
    int ch = 0;
    const float w = wave_rsum<8>(t, lane, 32, ch, 4);  // lanes of one octet q differ in bits 2..5
    if ((lane & 4) == 0) red[wave][8 * q + ch] = w;
    __syncthreads();
    if (tid < 32) st[k][tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
  };
  const float inv_n = 1.f / (float)HW;
  float t[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    t[e] = v[0][e];
#pragma unroll
    for (int it = 1; it < NIT; ++it) t[e] += v[it][e];
  }
  block_sum(t, 0);
  float mean[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mean[e] = st[0][8 * q + e] * inv_n;
    t[e] = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const float d = v[it][e] - mean[e];
      t[e] = (pr + 64 * it < HW) ? fmaf(d, d, t[e]) : t[e];
    }
  }
  block_sum(t, 1);
  float scl[8], shf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = c0 + 8 * q + e;
    scl[e] = (1.f / sqrtf(st[1][8 * q + e] * inv_n + eps)) * gamma[c];
    shf[e] = beta[c] - mean[e] * scl[e];
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int p = pr + 64 * it;
    if (p >= HW) continue;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = fmaf(v[it][e], scl[e], shf[e]);
      o[e] = u > 0.f ? u : u * slope;
    }
    const long off = ((long)b * HW + p) * C + c0 + 8 * q;
    if (y32 && chw) {  // fp32 CHW (the dense head's rows, enc_head_x3_kernel); y32 is then not y
#pragma unroll
      for (int e = 0; e < 8; ++e) y32[((long)b * C + c0 + 8 * q + e) * HW + p] = o[e];
    } else if (y32) {
      *reinterpret_cast<f32x4*>(y32 + off) = f32x4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<f32x4*>(y32 + off + 4) = f32x4{o[4], o[5], o[6], o[7]};
    } else {
      damc::store_x3_octet(o, y3 + 3 * off);
    }
  }
}

}  // namespace

namespace damc {

void launch_in_merge(const float* part, int B, int C, int S, const float* gamma, const float* beta, float eps,
                     float* ss, hipStream_t s) {
  hipLaunchKernelGGL(in_merge_kernel, dim3((B * C + 3) / 4), dim3(256), 0, s, part, B, C, S, gamma, beta, eps, ss);
}

int launch_in_onepass(const damc_enc_layer_t& L, const float* y, int B, int hw, unsigned short* a3, float* y32, int chw,
                      const float* kslab, int ks, hipStream_t s) {
  ProfScope ps("instnorm", 0.0, s);
  const int ntn = (L.cout + 127) / 128;
  const long sstride4 = (long)((B * hw + 255) / 256) * ntn * (256 * 128 / 4);
  // NIT = ceil(hw / 64) pixels per thread, rounded up to 1, 2 or 4
  auto* kernel = hw <= 64 ? in_fused_x3_kernel<1> : hw <= 128 ? in_fused_x3_kernel<2> : in_fused_x3_kernel<4>;
  hipLaunchKernelGGL(kernel, dim3(B, L.cout / 32), dim3(256), 0, s, y, hw, L.cout, L.in_gamma, L.in_beta, L.in_eps,
                     L.slope, a3, y32, ks > 0 ? kslab : nullptr, ks, ntn, sstride4, L.bias, chw);
  DAMC_LAUNCH_CHECK();
  return 0;
}

int launch_in_threepass(const damc_enc_layer_t& L, float* y, int B, int hw, bool strip, bool strip_done, float* inws,
                        unsigned short* a3, bool f32_out, hipStream_t s) {
  const int C = L.cout, S = strip ? hw / 256 : in_splits(hw), cg = (C + 63) / 64;
  float* ssb = inws + (size_t)B * C * S * 3;
  ProfScope ps("instnorm", 0.0, s);
  if (!strip)
    hipLaunchKernelGGL(in_stats_kernel, dim3(B * cg, S), dim3(256), 0, s, y, B, hw, C, S, inws);
  else if (!strip_done)
    hipLaunchKernelGGL(in_strip_stats_kernel, dim3(S, B, (C + 127) / 128), dim3(512), 0, s, y, hw, C, inws);
  launch_in_merge(inws, B, C, S, L.in_gamma, L.in_beta, L.in_eps, ssb, s);
  const long n8 = (long)B * hw * (C / 8);
  if (f32_out) {
    const long n4 = 2 * n8;
    hipLaunchKernelGGL(in_apply_f32_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, y, n4, hw, C, ssb,
                       L.slope);
  } else {
    hipLaunchKernelGGL(in_apply_x3_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, y, n8, hw, C, ssb,
                       L.slope, a3, (float*)nullptr);
  }
  DAMC_LAUNCH_CHECK();
  return 0;
}

}  // namespace damc

extern "C" size_t damc_instnorm_workspace_floats(int B, int hw, int c) {
  return (size_t)B * c * in_splits(hw) * 3 + (size_t)B * c;  // the partials, then the pivots (in_stats_pivot_kernel)
}

extern "C" int damc_instnorm_lrelu_nhwc(float* y, int B, int hw, int c, const float* gamma, const float* beta,
                                        float eps, float slope, float* ws, void* stream) {
  if (!y || !gamma || !beta || !ws || B <= 0 || hw <= 0 || c <= 0) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  const int S = in_splits(hw);
  const int cg = (c + 63) / 64;
  ProfScope ps("instnorm", 0.0, s);
  float* piv = ws + (size_t)B * c * S * 3;
  hipLaunchKernelGGL(in_stats_pivot_kernel, dim3(B * cg, S), dim3(256), 0, s, (const float*)y, B, hw, c, S, ws, piv);
  const int P = std::max(1, std::min(64, hw / 256));
  hipLaunchKernelGGL(in_apply_kernel, dim3(B * cg, P), dim3(256), 0, s, y, B, hw, c, S, ws, (const float*)piv, gamma,
                     beta, eps, slope);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ training (Q update)
// InstanceNorm2d(affine) + LeakyReLU for the encoder's training forward/backward: the conv output y is kept,
// h = lrelu(IN(y)) goes to its own buffer and (mean, rstd) per (sample, channel) are saved.  The backward
// of a = gamma * (y - mean) * rstd + beta, h = lrelu(a) (biased variance, as InstanceNorm2d):
//   dA = dh * lrelu'(a);  dy = rstd * gamma * (dA - mean_p(dA) - xhat * mean_p(dA * xhat))
// with per-(sample, channel) sums over pixels taken in S splits and merged in fixed order.
namespace {

__global__ __launch_bounds__(256) void in_apply_train_kernel(const float* y, int B, int HW, int C, int S,
                                                             const float* part, const float* piv,
                                                             const float* gamma, const float* beta, float eps,
                                                             float slope, float* h, float* stats) {
  const int cg = (C + 63) / 64;
  const int b = blockIdx.x / cg, c = (blockIdx.x % cg) * 64 + (threadIdx.x & 63);
  const int prow = threadIdx.x >> 6;
  __shared__ float sc[64], sh[64];
  if (prow == 0) {
    float scale = 0.f, shift = 0.f;
    if (c < C) {
      const float* pp = part + ((long)b * C + c) * S * 3;
      Wf a{pp[0], pp[1], pp[2]};
      for (int s = 1; s < S; ++s) a = wmerge(a, Wf{pp[3 * s], pp[3 * s + 1], pp[3 * s + 2]});
      const float var = a.m2 / a.n;
      const float rstd = 1.f / sqrtf(var + eps);
      scale = rstd;
      shift = __fadd_rn(piv[(long)b * C + c], a.mean);
      if (blockIdx.y == 0) {
        stats[((long)b * C + c) * 2] = shift;
        stats[((long)b * C + c) * 2 + 1] = rstd;
      }
    }
    sc[threadIdx.x] = scale;
    sh[threadIdx.x] = shift;
  }
  __syncthreads();
  if (c >= C) return;
  // a = ((y - mean) * rstd) * gamma + beta, InstanceNorm's own order: the fused y * scale + shift form of
  // the inference pass loses low bits when |mean| >> std, and the backward's LReLU' reads the sign of a
  const float rstd = sc[threadIdx.x & 63], mean = sh[threadIdx.x & 63], g = gamma[c], bt = beta[c];
  const int P = gridDim.y;
  const int p0 = (int)((long)HW * blockIdx.y / P), p1 = (int)((long)HW * (blockIdx.y + 1) / P);
  for (int p = p0 + prow; p < p1; p += 4) {
    const long o = ((long)b * HW + p) * C + c;
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(y[o], mean), rstd), g), bt);
    h[o] = v > 0.f ? v : v * slope;
  }
}

// pass 1: per (b, c, split) partial sums {sum dA, sum dA * xhat}
__global__ __launch_bounds__(256) void in_bwd_sums_kernel(const float* y, const float* stats, const float* dh, int B,
                                                          int HW, int C, int S, const float* gamma, const float* beta,
                                                          float slope, float* part) {
  const int cg = (C + 63) / 64;
  const int b = blockIdx.x / cg, c = (blockIdx.x % cg) * 64 + (threadIdx.x & 63);
  const int prow = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int p0 = (int)((long)HW * s / S), p1 = (int)((long)HW * (s + 1) / S);
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const float mean = stats[((long)b * C + c) * 2], rstd = stats[((long)b * C + c) * 2 + 1];
    const float g = gamma[c], bt = beta[c];
    for (int p = p0 + prow; p < p1; p += 4) {
      const long o = ((long)b * HW + p) * C + c;
      const float xh = __fmul_rn(__fsub_rn(y[o], mean), rstd);
      const float a = __fadd_rn(__fmul_rn(xh, g), bt);  // the forward's a, bit for bit
      const float dA = a > 0.f ? dh[o] : dh[o] * slope;
      s1 += dA;
      s2 += dA * xh;
    }
  }
  __shared__ float r1[4][64], r2[4][64];
  r1[prow][threadIdx.x & 63] = s1;
  r2[prow][threadIdx.x & 63] = s2;
  __syncthreads();
  if (prow == 0 && c < C) {
    const int l = threadIdx.x;
    float* o = part + (((long)b * C + c) * S + s) * 2;
    o[0] = ((r1[0][l] + r1[1][l]) + r1[2][l]) + r1[3][l];
    o[1] = ((r2[0][l] + r2[1][l]) + r2[2][l]) + r2[3][l];
  }
}

// pass 2: merge the S partials (fixed order), write dy; totals per (b, c) go to bc (B x C x 2) for dgamma/dbeta
__global__ __launch_bounds__(256) void in_bwd_apply_kernel(const float* y, const float* stats, const float* dh, int B,
                                                           int HW, int C, int S, const float* gamma,
                                                           const float* beta, float slope, const float* part,
                                                           float* dy, float* bc) {
  const int cg = (C + 63) / 64;
  const int b = blockIdx.x / cg, c = (blockIdx.x % cg) * 64 + (threadIdx.x & 63);
  const int prow = threadIdx.x >> 6;
  if (c >= C) return;
  const float* pp = part + ((long)b * C + c) * S * 2;
  float t1 = 0.f, t2 = 0.f;
  for (int s = 0; s < S; ++s) {
    t1 += pp[2 * s];
    t2 += pp[2 * s + 1];
  }
  if (blockIdx.y == 0 && prow == 0) {  // bc [b][2][C]: dgamma rows (sum dA * xhat), then dbeta rows (sum dA)
    bc[((long)b * 2) * C + c] = t2;
    bc[((long)b * 2 + 1) * C + c] = t1;
  }
  const float mean = stats[((long)b * C + c) * 2], rstd = stats[((long)b * C + c) * 2 + 1];
  const float g = gamma[c], bt = beta[c];
  const float scl = rstd * g;
  const float m1 = t1 / (float)HW, m2 = t2 / (float)HW;
  const int P = gridDim.y;
  const int p0 = (int)((long)HW * blockIdx.y / P), p1 = (int)((long)HW * (blockIdx.y + 1) / P);
  for (int p = p0 + prow; p < p1; p += 4) {
    const long o = ((long)b * HW + p) * C + c;
    const float xh = __fmul_rn(__fsub_rn(y[o], mean), rstd);
    const float a = __fadd_rn(__fmul_rn(xh, g), bt);
    const float dA = a > 0.f ? dh[o] : dh[o] * slope;
    dy[o] = scl * (dA - m1 - xh * m2);
  }
}

}  // namespace

extern "C" int damc_instnorm_lrelu_train_nhwc(const float* y, int B, int hw, int c, const float* gamma,
                                              const float* beta, float eps, float slope, float* h, float* stats,
                                              float* ws, void* stream) {
  if (!y || !h || !stats || !gamma || !beta || !ws || B <= 0 || hw <= 0 || c <= 0) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  const int S = in_splits(hw);
  const int cg = (c + 63) / 64;
  ProfScope ps("instnorm", 0.0, s);
  float* piv = ws + (size_t)B * c * S * 3;
  hipLaunchKernelGGL(in_stats_pivot_kernel, dim3(B * cg, S), dim3(256), 0, s, y, B, hw, c, S, ws, piv);
  const int P = std::max(1, std::min(64, hw / 256));
  hipLaunchKernelGGL(in_apply_train_kernel, dim3(B * cg, P), dim3(256), 0, s, y, B, hw, c, S, (const float*)ws,
                     (const float*)piv, gamma, beta, eps, slope, h, stats);
  return (int)hipGetLastError();
}

extern "C" size_t damc_instnorm_bwd_workspace_floats(int B, int hw, int c) {
  if (B <= 0 || hw <= 0 || c <= 0) return 0;
  return (size_t)B * c * in_splits(hw) * 2 + (size_t)B * c * 2 + damc::colsum_tmp_floats(B, c);
}

extern "C" int damc_instnorm_lrelu_backward_nhwc(const float* y, const float* stats, const float* dh, int B, int hw,
                                                 int c, const float* gamma, const float* beta, float slope, float* dy,
                                                 float* dgamma, float* dbeta, float* ws, void* stream) {
  if (!y || !stats || !dh || !dy || !gamma || !beta || !ws || B <= 0 || hw <= 0 || c <= 0) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  const int S = in_splits(hw);
  const int cg = (c + 63) / 64;
  float* part = ws;
  float* bc = part + (size_t)B * c * S * 2;
  float* tmp = bc + (size_t)B * c * 2;
  ProfScope ps("instnorm_bwd", 0.0, s);
  hipLaunchKernelGGL(in_bwd_sums_kernel, dim3(B * cg, S), dim3(256), 0, s, y, stats, dh, B, hw, c, S, gamma, beta,
                     slope, part);
  const int P = std::max(1, std::min(64, hw / 256));
  hipLaunchKernelGGL(in_bwd_apply_kernel, dim3(B * cg, P), dim3(256), 0, s, y, stats, dh, B, hw, c, S, gamma, beta,
                     slope, (const float*)part, dy, bc);
  DAMC_LAUNCH_CHECK();
  // dgamma = sum_b bc[b][0][c], dbeta = sum_b bc[b][1][c]: fixed-order column sums over the B rows
  if (dgamma && dbeta) return damc::launch_colsum2(bc, B, 2 * c, 2L * c, dgamma, dbeta, c, tmp, s);
  if (dgamma) {
    int rc = damc::launch_colsum(bc, B, c, 2L * c, dgamma, tmp, s);
    if (rc) return rc;
  }
  if (dbeta) {
    int rc = damc::launch_colsum(bc + c, B, c, 2L * c, dbeta, tmp, s);
    if (rc) return rc;
  }
  return 0;
}
