// enc_first.hip — the encoder's first layer (Conv2d k3 s1 p1 on the nc <= 4 image channels, then InstanceNorm +
// LeakyReLU) from the caller's NCHW image straight to layer 1's input, without storing the conv output.  Three
// generations, all kept: the fmaf-chain two passes (conv3_stats_kernel, conv3_apply_x3_kernel), the same two passes on
// the limb MFMA (conv3_mfma_kernel), and one pass for samples of at most 1024 pixels (conv3_in_fused_kernel, which
// also runs the call's weight packing as extra workgroups).  launch_enc_first picks the form; encoder.hip's forward
// calls it.  Shares with the other encoder files (enc_impl.h): Wf / wmerge, wave_rsum; the two-pass forms merge their
// strips with enc_norm.hip's in_merge_kernel (launch_in_merge).
#include <algorithm>

#include "enc_impl.h"

using damc::wave_rsum;
using damc::Wf;
using damc::wmerge;

namespace {

// ---- the first layer (Conv2d k3 s1 p1 on the nc <= 4 image channels, then InstanceNorm + LeakyReLU) in two passes
// that recompute the convolution (9 nc MACs per output) instead of storing it: pass 1 its per-(sample, channel)
// statistics, pass 2 the normalised activation as the next convolution's limbs.  The conv output, the largest
// tensor of the encoder (1 GB at CelebA-HQ B=64), never reaches HBM.  A block = R image rows of one sample, the
// (R+2) x (W+2) x CIN input window staged in LDS (read from the caller's NCHW image).  A wave owns one channel
// octet at a time (its 8 x 9 CIN weights wave-uniform: scalar loads, no LDS traffic) and its lanes own pixels, whose
// 9 CIN window values are read from LDS once for the 8 channels.  Both passes evaluate y with conv3_octet (fixed tap
// order, one fmaf chain per channel), so the statistics describe exactly the values pass 2 normalises.
// PX horizontally adjacent pixels (x .. x + PX - 1 of row r) x one channel octet: the window values of the run are read
// once (3 x (PX + 2) x CIN instead of PX x 9 CIN) and each weight pair once per run; every output keeps the same fmaf
// chain (tap order, from 0, then + bias), so PX changes no value
template <int CIN, int PX>
__device__ __forceinline__ void conv3_octet(const float* __restrict__ win, int ld, int r, int x,
                                            const float* __restrict__ wl, int C, int c0, const float* __restrict__ bl,
                                            float (&y)[PX][8]) {
  float xv[3][PX + 2][CIN];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int cx = 0; cx < PX + 2; ++cx)
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) xv[ky][cx][ci] = win[((r + ky) * ld + x + cx) * CIN + ci];
  float acc[PX][8];
#pragma unroll
  for (int px = 0; px < PX; ++px)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[px][e] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {  // wl: the LDS copy of damc_pack_conv2d's [(ky, kx, ci)][co] (a wave-uniform
        const int t = (ky * 3 + kx) * CIN + ci;  // address: broadcast reads)
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(wl + t * C + c0);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(wl + t * C + c0 + 4);
        const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int px = 0; px < PX; ++px)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[px][e] = fmaf(wv[e], xv[ky][px + kx][ci], acc[px][e]);
      }
  }
#pragma unroll
  for (int px = 0; px < PX; ++px)
#pragma unroll
    for (int e = 0; e < 8; ++e) y[px][e] = acc[px][e] + bl[c0 + e];
}
// the strip's input window: rows r0-1 .. r0+R of sample b, columns -1 .. W, zero outside, [row][col][ci] in LDS
template <int CIN>
__device__ __forceinline__ void conv3_stage(const float* __restrict__ x, int b, int H, int W, int r0, int R, float* win) {
  // element i = (rr CIN + ci) ld + cc: lanes run along one channel row of x (coalesced), 8 unconditional loads (clamped
  // addresses, zeroed by select) in flight per thread before the LDS writes.  Round 5's loop took one element at a
  // time and its load -> ds_write chain paid a full HBM latency per element: with 2 workgroups per CU it was the
  // first layer's cost (40 us of CelebA-HQ B=8's stats pass)
  const int ld = W + 2, n = (R + 2) * ld * CIN;
  const float* xb = x + (long)b * CIN * H * W;
  for (int i0 = threadIdx.x; i0 < n; i0 += 8 * blockDim.x) {
    float v[8];
    int dst[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = min(i0 + j * (int)blockDim.x, n - 1);
      const int q = i / ld, cc = i - q * ld, rr = q / CIN, ci = q - rr * CIN;
      const int iy = r0 - 1 + rr, ix = cc - 1;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float t = xb[((long)ci * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1)];
      v[j] = ok ? t : 0.f;
      dst[j] = (rr * ld + cc) * CIN + ci;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + j * (int)blockDim.x < n) win[dst[j]] = v[j];
  }
}

// pass 1: grid (B, S strips of R rows); wave w takes octets w, w+4, ...; each lane a Welford chain over its pixels per
// channel (runs of PX pixels, W % PX == 0), then the 64 lanes merged (Chan, fixed butterfly order); part [B][C][S][3]
// as in_stats_kernel's
template <int CIN, int PX>
__global__ __launch_bounds__(256) void conv3_stats_kernel(const float* __restrict__ x, int H, int W, int C, int R,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm3[];  // [9 CIN][C] weights, [C] bias, then the window
  const int b = blockIdx.x, s = blockIdx.y, S = gridDim.y, r0 = s * R, rows = min(R, H - r0);
  float* wl = sm3;
  float* bl = wl + 9 * CIN * C;
  float* win = bl + C;
  for (int i = threadIdx.x; i < 9 * CIN * C; i += blockDim.x) wl[i] = w[i];
  for (int i = threadIdx.x; i < C; i += blockDim.x) bl[i] = bias ? bias[i] : 0.f;
  conv3_stage<CIN>(x, b, H, W, r0, R, win);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, npix = rows * W;
  for (int o = wave; o < C / 8; o += 4) {
    const int c0 = __builtin_amdgcn_readfirstlane(o * 8);
    Wf a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = Wf{0.f, 0.f, 0.f};
    float n = 0.f;
#pragma unroll 1
    for (int p = lane * PX; p < npix; p += 64 * PX) {
      // the weights are re-read from LDS per run (broadcast reads); held in registers across the loop they took
      // 216 VGPRs and left one wave per SIMD
      asm volatile("" ::: "memory");
      const int r = p / W, xx = p - r * W;
      float y[PX][8];
      conv3_octet<CIN, PX>(win, W + 2, r, xx, wl, C, c0, bl, y);
#pragma unroll
      for (int px = 0; px < PX; ++px) {
        n += 1.f;
        const float inv = 1.f / n;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = y[px][e] - a[e].mean;
          a[e].mean += d * inv;
          a[e].m2 += d * (y[px][e] - a[e].mean);
          a[e].n = n;
        }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const Wf t{__shfl_xor(a[e].n, off), __shfl_xor(a[e].mean, off), __shfl_xor(a[e].m2, off)};
        a[e] = (lane & off) ? wmerge(t, a[e]) : wmerge(a[e], t);  // both partners form the same (lower, upper) merge
      }
    if (lane < 8) {
      Wf t = a[0];
#pragma unroll
      for (int e = 1; e < 8; ++e)
        if (lane == e) t = a[e];
      float* op = part + (((long)b * C + c0 + lane) * S + s) * 3;
      op[0] = t.n;
      op[1] = t.mean;
      op[2] = t.m2;
    }
  }
}

// pass 2: grid (B, S strips); wave w takes octets w, w+4, ..., lanes pixels; writes the limbs of lrelu(IN(y)), or the
// fp32 values (NHWC) at y32 for an F32A next conv
template <int CIN, int PX>
__global__ __launch_bounds__(256) void conv3_apply_x3_kernel(const float* __restrict__ x, int H, int W, int C, int R,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const float* __restrict__ ss, float slope,
                                                             unsigned short* __restrict__ y3, float* __restrict__ y32) {
  extern __shared__ __attribute__((aligned(16))) float sm3[];  // [9 CIN][C] weights, [C] bias, then the window
  const int b = blockIdx.x, s = blockIdx.y, r0 = s * R, rows = min(R, H - r0);
  float* wl = sm3;
  float* bl = wl + 9 * CIN * C;
  float* win = bl + C;
  for (int i = threadIdx.x; i < 9 * CIN * C; i += blockDim.x) wl[i] = w[i];
  for (int i = threadIdx.x; i < C; i += blockDim.x) bl[i] = bias ? bias[i] : 0.f;
  conv3_stage<CIN>(x, b, H, W, r0, R, win);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, npix = rows * W;
  const float* sb = ss + (long)b * 2 * C;
  for (int o = wave; o < C / 8; o += 4) {
    const int c0 = __builtin_amdgcn_readfirstlane(o * 8);
#pragma unroll 1
    for (int p = lane * PX; p < npix; p += 64 * PX) {
      asm volatile("" ::: "memory");  // weights re-read from LDS per run (see conv3_stats_kernel)
      const int r = p / W, xx = p - r * W;
      float y[PX][8];
      conv3_octet<CIN, PX>(win, W + 2, r, xx, wl, C, c0, bl, y);
#pragma unroll
      for (int px = 0; px < PX; ++px) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = fmaf(y[px][e], sb[c0 + e], sb[C + c0 + e]);
          v[e] = t > 0.f ? t : t * slope;
        }
        const long off = (((long)b * H + r0 + r) * W + xx + px) * C + c0;
        if (y32) {
          *reinterpret_cast<f32x4*>(y32 + off) = f32x4{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(y32 + off + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
          damc::store_x3_octet(v, y3 + 3 * off);
        }
      }
    }
  }
}

// ---- the first layer on the limb MFMA (round 6; DAMC_ENC_FIRST_MFMA=0 keeps the fmaf-chain passes above): the k3 conv
// on CIN <= 3 channels has K = 9 CIN <= 32, one K tile of v_mfma_f32_16x16x32_bf16.  A 16-pixel group's im2col rows
// (k = (ky 3 + kx) CIN + ci, zero past 9 CIN) come from the LDS window, each value split into its three RNE bf16 limbs
// (the GEMM engine's split3), the weights' limbs ([(ky, kx, ci)][co], damc_pack_conv2d's layout) sit in registers, and
// every output is the six limb products summed smallest first into fp32 (the limb engine's arithmetic: error at or
// below the fp32-MFMA engine's), plus the bias.  Pass 1 (STATS) runs a Welford chain per lane
// and channel over the lane's pixels (4 per group), merged over the lanes of a channel (butterfly) and the 4 waves
// (fixed order) into part [B][C][S][3] as conv3_stats_kernel does; pass 2 recomputes y with the same code (so the
// statistics describe exactly the values it normalises), applies lrelu(y scale + shift) and writes the NHWC activation
// as fp32 for an F32A next conv, or as its limbs.  Wave w takes the strip's 16-pixel groups w, w + 4, ...; W % 16 == 0.
typedef __bf16 c3b8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void c3_split8(const float (&v)[8], c3b8& h, c3b8& m, c3b8& l) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 b0 = (__bf16)v[e];
    const float r1 = sub_rn(v[e], (float)b0);
    const __bf16 b1 = (__bf16)r1;
    h[e] = b0;
    m[e] = b1;
    l[e] = (__bf16)sub_rn(r1, (float)b1);
  }
}
// the window as its three RNE bf16 limb planes (c3_split8's split, done once per window value instead of once per
// im2col use: each value feeds 9 CIN taps)
template <int CIN>
__device__ __forceinline__ void conv3_stage_limbs(const float* __restrict__ x, int b, int H, int W, int r0, int R,
                                                  __bf16* wh, __bf16* wm, __bf16* wl) {
  // element (q = rr CIN + ci, cc) of the flattened (R + 2) CIN x (W + 2) window; a thread's elements step by blockDim
  // (q and cc advanced incrementally: no division per element), 8 loads in flight; slots past the end repeat the last
  // element (the same value to the same address), so the loads and LDS stores run unconditionally
  const int ld = W + 2, nq = (R + 2) * CIN, n = nq * ld, dq = blockDim.x / ld, dc = blockDim.x - dq * ld;
  const float* xb = x + (long)b * CIN * H * W;
  int q = threadIdx.x / ld, cc = threadIdx.x - q * ld;
  for (int i0 = 0; i0 < n; i0 += 8 * blockDim.x) {
    float v[8];
    int dst[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int past = q >= nq;
      const int qc = past ? nq - 1 : q, ccc = past ? ld - 1 : cc;
      const int rr = qc / CIN, ci = qc - rr * CIN, iy = r0 - 1 + rr, ix = ccc - 1;
      const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const float t = xb[(unsigned)((ci * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1))];
      v[j] = ok ? t : 0.f;
      dst[j] = (rr * ld + ccc) * CIN + ci;
      cc += dc;
      const int wr = cc >= ld;
      cc -= ld & -wr;
      q += dq + wr;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const __bf16 b0 = (__bf16)v[j];
      const float r1 = sub_rn(v[j], (float)b0);
      const __bf16 b1 = (__bf16)r1;
      wh[dst[j]] = b0;
      wm[dst[j]] = b1;
      wl[dst[j]] = (__bf16)sub_rn(r1, (float)b1);
    }
  }
}
template <int CIN, int NT, bool STATS>
__global__ __launch_bounds__(256) void conv3_mfma_kernel(const float* __restrict__ x, int H, int W, int C, int R,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ part, const float* __restrict__ ss,
                                                         float slope, float* __restrict__ y32,
                                                         unsigned short* __restrict__ y3) {
  static_assert(9 * CIN <= 32 && NT * 16 <= 128, "one K tile, at most 128 channels");
  extern __shared__ __attribute__((aligned(16))) __bf16 c3win[];  // the (R+2) x (W+2) x CIN window's 3 limb planes
  __shared__ Wf c3red[4][NT * 16];
  constexpr int OLD = NT * 16 + 4;  // the output staging tile's row stride (floats)
  __shared__ __attribute__((aligned(16))) float c3out[STATS ? 1 : 4][16][OLD];
  const int b = blockIdx.x, s = blockIdx.y, S = gridDim.y, r0 = s * R, rows = min(R, H - r0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
  const int pst = (R + 2) * (W + 2) * CIN;  // the limb planes' stride (elements)
  conv3_stage_limbs<CIN>(x, b, H, W, r0, R, c3win, c3win + pst, c3win + 2 * pst);
  // the weights' limbs: tile t, lane (channel 16 t + n, k-octet kq)
  c3b8 wb[NT][3];
  float bl[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 8 * kq + e;
      v[e] = k < 9 * CIN ? w[(long)k * C + 16 * t + n] : 0.f;
    }
    c3_split8(v, wb[t][0], wb[t][1], wb[t][2]);
    bl[t] = bias ? bias[16 * t + n] : 0.f;
  }
  // the lane's im2col offsets within the window for its pixel n and k-octet: tap (ky, kx) and ci of k = 8 kq + e; a
  // k >= 9 CIN reads the pixel's own first value (any finite value: its weight limbs are zero, so the products are)
  int koff[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = 8 * kq + e, tap = k / CIN, ci = k - tap * CIN;
    koff[e] = n * CIN + (k < 9 * CIN ? ((tap / 3) * (W + 2) + tap % 3) * CIN + ci : 0);
  }
  __syncthreads();
  const int ngrp = rows * W / 16;
  Wf a[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) a[t] = Wf{0.f, 0.f, 0.f};
  float nn = 0.f;
  float scl[NT], shf[NT];  // lrelu(acc scl + shf): the bias folded into the shift
  if constexpr (!STATS) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      scl[t] = ss[(long)b * 2 * C + 16 * t + n];
      shf[t] = fmaf(bl[t], scl[t], ss[(long)b * 2 * C + C + 16 * t + n]);
    }
  }
  for (int g = wave; g < ngrp; g += 4) {
    // A: pixel m = 16 g + (lane & 15) of the strip (one row: W % 16 == 0, so the group's row and first column are
    // wave-uniform), k-octet kq
    const int p0 = __builtin_amdgcn_readfirstlane(16 * g), r = p0 / W;
    const int base = (r * (W + 2) + p0 - r * W) * CIN;
    c3b8 ah, am, al;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int idx = base + koff[e];
      ah[e] = c3win[idx];
      am[e] = c3win[pst + idx];
      al[e] = c3win[2 * pst + idx];
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wb[t][0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, wb[t][1], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wb[t][2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, wb[t][0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wb[t][1], c, 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wb[t][0], c, 0, 0, 0);
    }
    // lane (n, kq) holds y[pixel 16 g + 4 kq + i][channel 16 t + n], i = 0..3
    if constexpr (STATS) {
      // the lane's 4 values of channel 16 t + n as one chunk (its mean and m2 about it) merged into the lane's chain
      // (Chan's update, one division per group; round 5 ran a Welford step per value).  The chain runs on acc, the
      // bias joins the mean after the loop (y = acc + bias has acc's m2)
      const float nb = nn + 4.f, f = 4.f / nb, cw = nn * f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float mb = ((acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3])) * 0.25f;
        const float d0 = acc[t][0] - mb, d1 = acc[t][1] - mb, d2 = acc[t][2] - mb, d3 = acc[t][3] - mb;
        const float q = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, d0 * d0)));
        const float dl = mb - a[t].mean;
        a[t].mean = fmaf(dl, f, a[t].mean);
        a[t].m2 = fmaf(dl * dl, cw, a[t].m2 + q);
      }
      nn = nb;
    } else {
      // through the wave's LDS tile to whole channel octets per lane: 16-B fp32 stores, or the limbs
      // (damc::store_x3_octet, the F32A conv's in-register split), so both output forms carry the same values
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float tt = fmaf(acc[t][i], scl[t], shf[t]);
          c3out[wave][4 * kq + i][16 * t + n] = fmaxf(tt, tt * slope);  // lrelu for 0 <= slope <= 1 (host-checked)
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const long obase = (((long)b * H + r0 + r) * W + p0 - r * W) * C;  // wave-uniform
      if (y32) {
        // the group's 16 pixels x C channels are one contiguous run of the NHWC output: lane l of store j writes its
        // 16 B at float 4 (l + 64 j), so every store instruction covers 1 KB without gaps (round 6, late: the octet
        // form wrote two half-covered 2 KB spans per pair of stores)
#pragma unroll
        for (int it = 0; it < 16 * NT * 16 / 256; ++it) {
          const int j = lane + 64 * it, pp = j / (4 * NT), c4 = j - pp * (4 * NT);
          *reinterpret_cast<f32x4*>(y32 + obase + 4 * j) = *reinterpret_cast<const f32x4*>(&c3out[wave][pp][4 * c4]);
        }
      } else {
#pragma unroll
        for (int it = 0; it < 2 * NT * 16 / 64; ++it) {  // 16 pixels x NT * 2 octets
          const int id = lane + 64 * it, pp = id / (2 * NT), oc = id - pp * (2 * NT);
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = c3out[wave][pp][8 * oc + e];
          damc::store_x3_octet(v, y3 + 3 * (obase + (pp * (16 * NT) + 8 * oc)));  // C == 16 NT
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the tile is rewritten by the wave's next group
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  if constexpr (STATS) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      a[t].n = nn;
      a[t].mean += bl[t];
    }
    // the four lanes of a channel (kq = 0..3), then the waves in order
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const Wf o{__shfl_xor(a[t].n, off), __shfl_xor(a[t].mean, off), __shfl_xor(a[t].m2, off)};
        a[t] = (lane & off) ? wmerge(o, a[t]) : wmerge(a[t], o);
      }
    if (kq == 0)
#pragma unroll
      for (int t = 0; t < NT; ++t) c3red[wave][16 * t + n] = a[t];
    __syncthreads();
    for (int c = threadIdx.x; c < NT * 16; c += 256) {
      Wf m = c3red[0][c];
#pragma unroll
      for (int v = 1; v < 4; ++v) m = wmerge(m, c3red[v][c]);
      float* op = part + (((long)b * C + c) * S + s) * 3;
      op[0] = m.n;
      op[1] = m.mean;
      op[2] = m.m2;
    }
  }
}

// The same layer in ONE pass when a sample has at most 1024 pixels (32 x 32: CIFAR-10, SVHN) and W % 4 == 0:
// grid (B, C / 16), 512 threads = 2 channel octets (one per group of 4 waves, so weights are wave-uniform) x 256
// 4-pixel row runs (1024 threads capped the kernel at 128 VGPRs and it spilled).  Each thread evaluates its 4 pixels x 8 channels with conv3_octet's arithmetic (same fmaf chain,
// so the same y; each weight read once per 4 pixels, each window value once per run), the workgroup sums them per
// channel (wave reduce-scatter, then the channel's 4 wave sums in a fixed order) for the mean, then sums
// (y - mean)^2 for the variance (two passes over registers), and writes lrelu(IN(y)) as the next convolution's limbs.
// The statistics pass, the Welford partials, the merge kernel and the recomputing second pass all drop out.
// 1-D grid: workgroup (b, C / 16 chunk) for the first nconv = B * C / 16, then the per-call limb packing of the
// limb layers' weights (pk, pack_conv_x3_block) as extra workgroups of the same launch, so the two fill the chip
// together (a separate packing launch, or one on a forked stream, costs its own ramp / the event hand-offs)
template <int CIN>
__global__ __launch_bounds__(512) void conv3_in_fused_kernel(const float* __restrict__ x, int H, int W, int C,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, float slope,
                                                              unsigned short* __restrict__ y3, float* __restrict__ y32,
                                                              int nconv, damc::PackConvList pk) {
  extern __shared__ __attribute__((aligned(16))) float smf[];  // [9 CIN][16] weights, [8][8] sums, [2][16], window
  if ((int)blockIdx.x >= nconv) {  // workgroup-uniform
    damc::pack_conv_x3_block(pk, (int)blockIdx.x - nconv, threadIdx.x, 512, smf);
    return;
  }
  float* wl = smf;
  float* red = wl + 9 * CIN * 16;
  float* st = red + 8 * 8;
  float* win = st + 32;
  const int ncb = C / 16, b = blockIdx.x / ncb, c0 = (blockIdx.x - b * ncb) * 16, tid = threadIdx.x, lane = tid & 63,
            wave = tid >> 6;
  const int HW = H * W, cg = wave >> 2, run = tid & 255;  // channels c0 + 8 cg .. + 7; pixels 4 run .. + 3
  for (int i = tid; i < 9 * CIN * 16; i += 512) wl[i] = w[(i >> 4) * C + c0 + (i & 15)];
  conv3_stage<CIN>(x, b, H, W, 0, H, win);
  __syncthreads();
  const int p0 = 4 * run, r = p0 / W, x0 = p0 - r * W;
  const bool ok = p0 < HW;
  float y[4][8];
  {
    float acc[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {  // rolled: unrolled, the compiler hoisted every window and weight load and spilled
      float xr[CIN][6];  // the window row's 6 columns x0 - 1 .. x0 + 4 (padded coordinates x0 .. x0 + 5)
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
        for (int c = 0; c < 6; ++c) xr[ci][c] = ok ? win[((r + ky) * (W + 2) + x0 + c) * CIN + ci] : 0.f;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          const int t = (ky * 3 + kx) * CIN + ci;  // conv3_octet's tap order
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wl + t * 16 + 8 * cg);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(wl + t * 16 + 8 * cg + 4);
          const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[k][e] = fmaf(wv[e], xr[ci][k + kx], acc[k][e]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) y[k][e] = ok ? acc[k][e] + (bias ? bias[c0 + 8 * cg + e] : 0.f) : 0.f;
  }
  // per-channel workgroup sum of v[e] (channel c0 + 8 cg + e) into st[k * 16 + ...]
  auto block_sum = [&](const float (&v)[8], int k) {
    int ch = 0;
    const float t = wave_rsum<8>(v, lane, 32, ch);
    if ((lane & 7) == 0) red[wave * 8 + ch] = t;
    __syncthreads();
    if (tid < 16) {
      const int g = tid >> 3, e = tid & 7;  // channel 8 g + e: waves 4 g .. 4 g + 3
      st[k * 16 + tid] = ((red[(4 * g) * 8 + e] + red[(4 * g + 1) * 8 + e]) + red[(4 * g + 2) * 8 + e]) +
                         red[(4 * g + 3) * 8 + e];
    }
    __syncthreads();
  };
  const float inv_n = 1.f / (float)HW;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = ((y[0][e] + y[1][e]) + y[2][e]) + y[3][e];
  block_sum(v, 0);
  float mean[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mean[e] = st[8 * cg + e] * inv_n;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = y[k][e] - mean[e];
      q = ok ? fmaf(d, d, q) : q;
    }
    v[e] = q;
  }
  block_sum(v, 1);
  if (!ok) return;
  float scl[8], shf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {  // in_merge_kernel's scale / shift form
    const int c = c0 + 8 * cg + e;
    scl[e] = (1.f / sqrtf(st[16 + 8 * cg + e] * inv_n + eps)) * gamma[c];
    shf[e] = beta[c] - mean[e] * scl[e];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = fmaf(y[k][e], scl[e], shf[e]);
      t[e] = u > 0.f ? u : u * slope;
    }
    const long off = ((long)b * HW + p0 + k) * C + c0 + 8 * cg;
    if (y32) {  // fp32 NHWC for an F32A next conv
      *reinterpret_cast<f32x4*>(y32 + off) = f32x4{t[0], t[1], t[2], t[3]};
      *reinterpret_cast<f32x4*>(y32 + off + 4) = f32x4{t[4], t[5], t[6], t[7]};
    } else {
      damc::store_x3_octet(t, y3 + 3 * off);
    }
  }
}

}  // namespace

namespace damc {

int launch_enc_first(const damc_enc_layer_t& L, const float* x, int B, int H, int W, int R, int S, bool onepass,
                     bool mfma, bool px1, float* inws, unsigned short* a3, float* y32, const PackConvList& pl,
                     bool* pl_done, hipStream_t s) {
  const int C = L.cout, cin = L.cin;
  const size_t sm = ((size_t)(R + 2) * (W + 2) * cin + (size_t)9 * cin * C + C) * sizeof(float);
  if (sm > 65536) return DAMC_ERR_UNSUPPORTED;
  float* ssb = inws + (size_t)B * C * S * 3;
  ProfScope ps("enc_first", 2.0 * B * H * W * (double)C * 9 * cin * 2, s);
  // one pass (conv3_in_fused_kernel) when a sample fits 1024 threads x <= 4 pixels (a sample of at most 1024 pixels;
  // CelebA-64 and larger keep the two passes)
  const size_t sm1 = ((size_t)(H + 2) * (W + 2) * cin + (size_t)9 * cin * 16 + 8 * 8 + 32) * sizeof(float);
  const bool one = onepass && H * W <= 1024 && W % 4 == 0 && C % 16 == 0 && sm1 <= 65536;
  // round 6: both passes on the limb MFMA (conv3_mfma_kernel; CelebA-HQ B=64 first layer 0.87 -> see DESIGN.md) where
  // K = 9 CIN fits one K tile, C is 64 or 128, rows are whole 16-pixel groups and the next conv stages fp32
  const size_t smw = 3 * (size_t)(R + 2) * (W + 2) * cin * sizeof(__bf16);  // + ~11 KB static
  const bool mf = !one && mfma && (cin == 1 || cin == 3) && (C == 64 || C == 128) && W % 16 == 0 && smw <= 49152 &&
                  L.slope >= 0.f && L.slope <= 1.f;
  // runs of 4 pixels per lane in the fmaf statistics pass (the apply pass keeps one: its 2- and 4-pixel forms took 256
  // VGPRs) where the rows allow it
  const int px = (W % 4 == 0 && !px1) ? 4 : 1;
  if (one) {  // with the packing list, if it has not run, as extra workgroups of the same launch
    const int nconv = B * (C / 16), npk = *pl_done ? 0 : pl.blk0[pl.n];
    const size_t smp = std::max(sm1, *pl_done ? (size_t)0 : (size_t)pl.lds);
    auto* fused = cin == 1 ? conv3_in_fused_kernel<1> : cin == 3 ? conv3_in_fused_kernel<3> : conv3_in_fused_kernel<4>;
    hipLaunchKernelGGL(fused, dim3(nconv + npk), dim3(512), smp, s, x, H, W, C, L.w_packed, L.bias, L.in_gamma,
                       L.in_beta, L.in_eps, L.slope, a3, y32, nconv, pl);
    *pl_done = true;
    DAMC_LAUNCH_CHECK();
    return 0;
  }
  if (!*pl_done) {
    const int rc = launch_pack_conv_x3_many(pl, s);
    if (rc) return rc;
    *pl_done = true;
  }
  // two passes over B x S strips of R rows: the strips' statistics, their merge, the recomputed conv normalised
  if (mf) {
    const bool c1 = cin == 1, n4 = C == 64;  // conv3_mfma_kernel<CIN, C / 16, STATS>
    auto* stats = c1 ? (n4 ? conv3_mfma_kernel<1, 4, true> : conv3_mfma_kernel<1, 8, true>)
                     : (n4 ? conv3_mfma_kernel<3, 4, true> : conv3_mfma_kernel<3, 8, true>);
    auto* apply = c1 ? (n4 ? conv3_mfma_kernel<1, 4, false> : conv3_mfma_kernel<1, 8, false>)
                     : (n4 ? conv3_mfma_kernel<3, 4, false> : conv3_mfma_kernel<3, 8, false>);
    hipLaunchKernelGGL(stats, dim3(B, S), dim3(256), smw, s, x, H, W, C, R, L.w_packed, L.bias, inws, nullptr, 0.f,
                       nullptr, nullptr);
    launch_in_merge(inws, B, C, S, L.in_gamma, L.in_beta, L.in_eps, ssb, s);
    hipLaunchKernelGGL(apply, dim3(B, S), dim3(256), smw, s, x, H, W, C, R, L.w_packed, L.bias, nullptr, ssb, L.slope,
                       y32, a3);
  } else {
    auto* stats = px == 4 ? (cin == 1   ? conv3_stats_kernel<1, 4>
                             : cin == 3 ? conv3_stats_kernel<3, 4>
                                        : conv3_stats_kernel<4, 4>)
                          : (cin == 1   ? conv3_stats_kernel<1, 1>
                             : cin == 3 ? conv3_stats_kernel<3, 1>
                                        : conv3_stats_kernel<4, 1>);
    auto* apply = cin == 1   ? conv3_apply_x3_kernel<1, 1>
                  : cin == 3 ? conv3_apply_x3_kernel<3, 1>
                             : conv3_apply_x3_kernel<4, 1>;
    hipLaunchKernelGGL(stats, dim3(B, S), dim3(256), sm, s, x, H, W, C, R, L.w_packed, L.bias, inws);
    launch_in_merge(inws, B, C, S, L.in_gamma, L.in_beta, L.in_eps, ssb, s);
    hipLaunchKernelGGL(apply, dim3(B, S), dim3(256), sm, s, x, H, W, C, R, L.w_packed, L.bias, ssb, L.slope, a3, y32);
  }
  DAMC_LAUNCH_CHECK();
  return 0;
}

}  // namespace damc
