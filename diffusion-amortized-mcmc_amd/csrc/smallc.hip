// smallc.hip — the generator's output layer (DAMC_LAYER_SMALLC): the to-RGB ConvTranspose (Cout <= 4) with tanh
// and the residual delta = (x_hat - x)/s^2 * (1 - x_hat^2), and its input gradient.  h is NHWC fp32, x / x_hat
// NCHW.  Four generations of kernels, each the fallback of the next by shape (output layer: the
// reachability table): generic, register-resident, two-stage projection + gather, proj16 / fused epilogue
// (gemm_x3.hip) with the limb-engine dgrad.  The choices are the functions declared in smallc.h, at the end of
// this file.  The layer's weight gradient is in wgrad.hip.
#include <algorithm>
#include <cstdlib>

#include "gemm.h"
#include "smallc.h"

namespace {

// ---------------------------------------------------------------- generic kernels
// One wave per output pixel, lanes across input channels; weights staged once per
// workgroup in LDS as [tap][ci][co] and the grid strides over pixels.
template <int NC>
__global__ __launch_bounds__(256) void smallc_fwd_kernel(const float* h, int B, int Hin, int Win, int Cin, int k,
                                                         int stride, int pad, int Hout, int Wout, const float* wpk,
                                                         const float* bias, const float* x, float inv_s2,
                                                         float* delta, float* xhat, float* sqerr_sum) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int nw = k * k * Cin * NC;
  for (int i = threadIdx.x; i < nw; i += blockDim.x) wl[i] = wpk[i];
  __shared__ float red[4];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long npix = (long)B * Hout * Wout;
  float sq_local = 0.f;
  for (long pix = (long)blockIdx.x * 4 + wave; pix < npix; pix += (long)gridDim.x * 4) {
    const int b = (int)(pix / ((long)Hout * Wout));
    const int rem = (int)(pix - (long)b * Hout * Wout);
    const int oy = rem / Wout, ox = rem - oy * Wout;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    for (int ky = 0; ky < k; ++ky) {
      const int ty = oy + pad - ky;
      if (ty < 0 || ty % stride) continue;
      const int iy = ty / stride;
      if (iy >= Hin) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int tx = ox + pad - kx;
        if (tx < 0 || tx % stride) continue;
        const int ix = tx / stride;
        if (ix >= Win) continue;
        const float* hp = h + (((long)b * Hin + iy) * Win + ix) * Cin;
        const float* wp = wl + (ky * k + kx) * Cin * NC;
        for (int ci = lane; ci < Cin; ci += 64) {
          const float hv = hp[ci];
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[c] = fmaf(hv, wp[ci * NC + c], acc[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = wave_sum(acc[c]);
    if (lane < NC) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c == lane) a = acc[c];
      a += bias ? bias[lane] : 0.f;
      const float t = tanhf(a);
      const long nchw = (((long)b * NC + lane) * Hout + oy) * Wout + ox;
      if (xhat) xhat[nchw] = t;
      if (delta) {
        const float r = t - x[nchw];
        delta[pix * NC + lane] = r * inv_s2 * (1.f - t * t);
        sq_local += r * r;
      }
    }
  }
  if (sqerr_sum) {
    sq_local = wave_sum(sq_local);
    if (lane == 0) red[wave] = sq_local;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sqerr_sum, (red[0] + red[1] + red[2] + red[3]) * (0.5f * inv_s2));
  }
}

// dh[b,iy,ix,ci] = lrelu'(h) * sum_{ky,kx,co} delta[b, iy*s-p+ky, ix*s-p+kx, co] W[ci][co][ky][kx]
// written in place over h.
template <int NC>
__global__ __launch_bounds__(256) void smallc_dgrad_kernel(float* h, int B, int Hin, int Win, int Cin, int k,
                                                           int stride, int pad, int Hout, int Wout, const float* wpk,
                                                           const float* delta, int mask_act, float mask_slope) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int nw = k * k * Cin * NC;
  for (int i = threadIdx.x; i < nw; i += blockDim.x) wl[i] = wpk[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long npix = (long)B * Hin * Win;
  for (long pix = (long)blockIdx.x * 4 + wave; pix < npix; pix += (long)gridDim.x * 4) {
    const int b = (int)(pix / ((long)Hin * Win));
    const int rem = (int)(pix - (long)b * Hin * Win);
    const int iy = rem / Win, ix = rem - iy * Win;
    float* hp = h + pix * Cin;
    for (int ci0 = 0; ci0 < Cin; ci0 += 64) {
      const int ci = ci0 + lane;
      float acc = 0.f;
      for (int ky = 0; ky < k; ++ky) {
        const int oy = iy * stride - pad + ky;
        if (oy < 0 || oy >= Hout) continue;
        for (int kx = 0; kx < k; ++kx) {
          const int ox = ix * stride - pad + kx;
          if (ox < 0 || ox >= Wout) continue;
          const float* dp = delta + (((long)b * Hout + oy) * Wout + ox) * NC;
          if (ci < Cin) {
            const float* wp = wl + ((ky * k + kx) * Cin + ci) * NC;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc = fmaf(dp[c], wp[c], acc);
          }
        }
      }
      if (ci < Cin) hp[ci] = acc * act_grad_from_out(hp[ci], mask_act, mask_slope);
    }
  }
}

// ---- register-resident variants (the BASELINE shapes): a group of G = Cin/CH lanes owns one pixel,
// lane g holds channels [g*CH, g*CH+CH) and ALL their weights (K*K*CH*NC floats) in VGPRs for the
// whole launch; activations move as float4/float2 channel vectors (one coalesced 16*G-byte row per
// group), the NC partial dots are reduced across the group with xor-shuffles.
template <int CH>
struct VecT;
template <>
struct VecT<4> {
  typedef f32x4 T;
};
template <>
struct VecT<2> {
  typedef float __attribute__((ext_vector_type(2))) T;
};

template <int NC, int K, int S, int CH>
__global__ __launch_bounds__(256) void smallc_fwd_reg_kernel(const float* __restrict__ h, int B, int Hin, int Win,
                                                             int Cin, int pad, int Hout, int Wout,
                                                             const float* __restrict__ wpk,
                                                             const float* __restrict__ bias, const float* x,
                                                             float inv_s2, float* delta, float* xhat,
                                                             float* sqerr_sum) {
  typedef typename VecT<CH>::T V;
  __shared__ float red[4];
  const int G = Cin / CH, P = 64 / G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane % G, sub = lane / G;
  const int ci0 = g * CH;
  float w[K * K][CH][NC];
#pragma unroll
  for (int t = 0; t < K * K; ++t)
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int o = 0; o < NC; ++o) w[t][c][o] = wpk[((long)t * Cin + ci0 + c) * NC + o];
  float bo[NC];
#pragma unroll
  for (int o = 0; o < NC; ++o) bo[o] = bias ? bias[o] : 0.f;
  const long npix = (long)B * Hout * Wout;
  float sq_local = 0.f;
  const long step = (long)gridDim.x * 4 * P;
  for (long pix0 = ((long)blockIdx.x * 4 + wave) * P; pix0 < npix; pix0 += step) {
    const long pix = pix0 + sub;
    const bool live = pix < npix;
    const long pp = live ? pix : 0;
    const int b = (int)(pp / ((long)Hout * Wout));
    const int rem = (int)(pp - (long)b * Hout * Wout);
    const int oy = rem / Wout, ox = rem - oy * Wout;
    static_assert(S == 1, "stride-2 output layers use smallc_fwd_s2_kernel");
    // all K*K taps are loaded unconditionally (border taps clamped + zero-weighted) so the loads
    // issue back to back instead of serialising their latency behind per-tap branches
    V hv[K * K];
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int iy = oy + pad - ky;
      const int iyc = min(max(iy, 0), Hin - 1);
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = ox + pad - kx;
        const int ixc = min(max(ix, 0), Win - 1);
        hv[ky * K + kx] = *reinterpret_cast<const V*>(h + (((long)b * Hin + iyc) * Win + ixc) * Cin + ci0);
        const float m = (iy == iyc && ix == ixc) ? 1.f : 0.f;
        hv[ky * K + kx] *= m;
      }
    }
    float acc[NC];
#pragma unroll
    for (int o = 0; o < NC; ++o) acc[o] = 0.f;
#pragma unroll
    for (int t = 0; t < K * K; ++t)
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int o = 0; o < NC; ++o) acc[o] = fmaf(hv[t][c], w[t][c][o], acc[o]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
      if (off < G)
#pragma unroll
        for (int o = 0; o < NC; ++o) acc[o] += __shfl_xor(acc[o], off, 64);
    if (g == 0 && live) {
#pragma unroll
      for (int o = 0; o < NC; ++o) {
        const float t = tanhf(acc[o] + bo[o]);
        const long nchw = (((long)b * NC + o) * Hout + oy) * Wout + ox;
        if (xhat) xhat[nchw] = t;
        if (delta) {
          const float r = t - x[nchw];
          delta[pix * NC + o] = r * inv_s2 * (1.f - t * t);
          sq_local += r * r;
        }
      }
    }
  }
  if (sqerr_sum) {
    sq_local = wave_sum(sq_local);
    if (lane == 0) red[wave] = sq_local;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sqerr_sum, (red[0] + red[1] + red[2] + red[3]) * (0.5f * inv_s2));
  }
}

// k4 s2 p1 forward: a pixel group owns the output QUAD (2qy+py, 2qx+px), py,px in {0,1}, whose 16
// taps are exactly the 3x3 input neighbourhood (qy+dy, qx+dx) with ky = 1 + py - 2dy (0..3), so each
// input vector is loaded once and every tap index is a compile-time constant.
template <int NC, int CH>
__global__ __launch_bounds__(256) void smallc_fwd_s2_kernel(const float* __restrict__ h, int B, int Hin, int Win,
                                                            int Cin, const float* __restrict__ wpk,
                                                            const float* __restrict__ bias, const float* x,
                                                            float inv_s2, float* delta, float* xhat,
                                                            float* sqerr_sum) {
  typedef typename VecT<CH>::T V;
  constexpr int K = 4;
  __shared__ float red[4];
  const int G = Cin / CH, P = 64 / G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane % G, sub = lane / G;
  const int ci0 = g * CH;
  const int Hout = 2 * Hin, Wout = 2 * Win;
  float w[K * K][CH][NC];
#pragma unroll
  for (int t = 0; t < K * K; ++t)
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int o = 0; o < NC; ++o) w[t][c][o] = wpk[((long)t * Cin + ci0 + c) * NC + o];
  float bo[NC];
#pragma unroll
  for (int o = 0; o < NC; ++o) bo[o] = bias ? bias[o] : 0.f;
  const long nq = (long)B * Hin * Win;
  float sq_local = 0.f;
  const long step = (long)gridDim.x * 4 * P;
  for (long q0 = ((long)blockIdx.x * 4 + wave) * P; q0 < nq; q0 += step) {
    const long q = q0 + sub;
    const bool live = q < nq;
    const long qq = live ? q : 0;
    const int b = (int)(qq / ((long)Hin * Win));
    const int rem = (int)(qq - (long)b * Hin * Win);
    const int qy = rem / Win, qx = rem - qy * Win;
    V hv[3][3];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int iy = qy + dy, iyc = min(max(iy, 0), Hin - 1);
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int ix = qx + dx, ixc = min(max(ix, 0), Win - 1);
        V v = *reinterpret_cast<const V*>(h + (((long)b * Hin + iyc) * Win + ixc) * Cin + ci0);
        v *= (iy == iyc && ix == ixc) ? 1.f : 0.f;
        hv[dy + 1][dx + 1] = v;
      }
    }
    float acc[2][2][NC];
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
#pragma unroll
        for (int o = 0; o < NC; ++o) acc[py][px][o] = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          const int ky = 1 + py - 2 * dy;
          if (ky < 0 || ky > 3) continue;  // compile-time
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int kx = 1 + px - 2 * dx;
            if (kx < 0 || kx > 3) continue;
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
              for (int o = 0; o < NC; ++o)
                acc[py][px][o] = fmaf(hv[dy + 1][dx + 1][c], w[ky * K + kx][c][o], acc[py][px][o]);
          }
        }
      }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
      if (off < G)
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int px = 0; px < 2; ++px)
#pragma unroll
            for (int o = 0; o < NC; ++o) acc[py][px][o] += __shfl_xor(acc[py][px][o], off, 64);
    if (g == 0 && live) {
#pragma unroll
      for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px) {
          const int oy = 2 * qy + py, ox = 2 * qx + px;
          const long pix = ((long)b * Hout + oy) * Wout + ox;
#pragma unroll
          for (int o = 0; o < NC; ++o) {
            const float t = tanhf(acc[py][px][o] + bo[o]);
            const long nchw = (((long)b * NC + o) * Hout + oy) * Wout + ox;
            if (xhat) xhat[nchw] = t;
            if (delta) {
              const float r = t - x[nchw];
              delta[pix * NC + o] = r * inv_s2 * (1.f - t * t);
              sq_local += r * r;
            }
          }
        }
    }
  }
  if (sqerr_sum) {
    sq_local = wave_sum(sq_local);
    if (lane == 0) red[wave] = sq_local;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sqerr_sum, (red[0] + red[1] + red[2] + red[3]) * (0.5f * inv_s2));
  }
}

template <int NC, int K, int S, int CH>
__global__ __launch_bounds__(256) void smallc_dgrad_reg_kernel(float* h, int B, int Hin, int Win, int Cin, int pad,
                                                               int Hout, int Wout, const float* __restrict__ wpk,
                                                               const float* __restrict__ delta, int mask_act,
                                                               float mask_slope, unsigned short* __restrict__ h3) {
  typedef typename VecT<CH>::T V;
  const int G = Cin / CH, P = 64 / G;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane % G, sub = lane / G;
  const int ci0 = g * CH;
  float w[K * K][CH][NC];
#pragma unroll
  for (int t = 0; t < K * K; ++t)
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int o = 0; o < NC; ++o) w[t][c][o] = wpk[((long)t * Cin + ci0 + c) * NC + o];
  const long npix = (long)B * Hin * Win;
  const long step = (long)gridDim.x * 4 * P;
  for (long pix0 = ((long)blockIdx.x * 4 + wave) * P; pix0 < npix; pix0 += step) {
    const long pix = pix0 + sub;
    if (pix >= npix) continue;
    const int b = (int)(pix / ((long)Hin * Win));
    const int rem = (int)(pix - (long)b * Hin * Win);
    const int iy = rem / Win, ix = rem - iy * Win;
    V* hp = reinterpret_cast<V*>(h + pix * Cin + ci0);
    V hv = *hp;  // issued first: its latency overlaps the delta gathers
    float d[K * K][NC];
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int oy = iy * S - pad + ky;
      const int oyc = min(max(oy, 0), Hout - 1);
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ox = ix * S - pad + kx;
        const int oxc = min(max(ox, 0), Wout - 1);
        const float* dp = delta + (((long)b * Hout + oyc) * Wout + oxc) * NC;
        const float m = (oy == oyc && ox == oxc) ? 1.f : 0.f;
#pragma unroll
        for (int o = 0; o < NC; ++o) d[ky * K + kx][o] = dp[o] * m;
      }
    }
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.f;
#pragma unroll
    for (int t = 0; t < K * K; ++t)
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int o = 0; o < NC; ++o) acc[c] = fmaf(d[t][o], w[t][c][o], acc[c]);
#pragma unroll
    for (int c = 0; c < CH; ++c) hv[c] = acc[c] * act_grad_from_out(hv[c], mask_act, mask_slope);
    if (h3) {
      // limbs only (the limb engine reads this gradient); h keeps the activation.  x3 layout:
      // pixel row of 3*Cin bf16, channel octet o at 24 o, limb l at + 8 l
      unsigned short* q = h3 + pix * 3 * Cin + (ci0 >> 3) * 24 + (ci0 & 7);
      typedef unsigned short U __attribute__((ext_vector_type(CH)));
      U lh, lm, ll;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const __bf16 b0 = (__bf16)hv[c];
        const float r1 = sub_rn(hv[c], (float)b0);
        const __bf16 b1 = (__bf16)r1;
        const __bf16 b2 = (__bf16)(sub_rn(r1, (float)b1));
        lh[c] = __builtin_bit_cast(unsigned short, b0);
        lm[c] = __builtin_bit_cast(unsigned short, b1);
        ll[c] = __builtin_bit_cast(unsigned short, b2);
      }
      *reinterpret_cast<U*>(q) = lh;
      *reinterpret_cast<U*>(q + 8) = lm;
      *reinterpret_cast<U*>(q + 16) = ll;
    } else {
      *hp = hv;
    }
  }
}

// k3 s1 p1 output-layer dgrad (CIFAR-10): a block owns R input rows of one image and stages the
// (R+2) x (W+2) x NC delta window (zero border) in LDS once, so the 9 taps read LDS broadcasts instead
// of per-pixel global gathers; lanes own 4 channels of a pixel and each wave walks its pixels UNR at a
// time (UNR activation loads in flight).  Output: the masked gradient as fp32 in place, or (h3) as x3
// limbs only, lane pairs exchanging halves so every store is a whole 16-B limb octet.
template <int NC>
__global__ __launch_bounds__(256) void smallc_dgrad_k3_kernel(float* __restrict__ h, int Hin, int Win, int Cin,
                                                              int R, const float* __restrict__ wpk,
                                                              const float* __restrict__ delta, int mask_act,
                                                              float mask_slope, unsigned short* __restrict__ h3,
                                                              const unsigned char* __restrict__ hbits) {
  // 4 pixels in flight per wave, the next iteration's sign-bit nibbles prefetched (CIFAR B=128, 8 rows: 66.7 us;
  // UNR = 2: 70.8, no prefetch: 67.5; profiles/r03/smallc_bench.txt)
  constexpr int UNR = 4;
  extern __shared__ __attribute__((aligned(16))) float dl[];  // [(R+2)][(Win+2)][4]
  __shared__ __attribute__((aligned(16))) unsigned char stg_all[4][UNR * 1536];  // per-wave x3 staging
  constexpr int K = 3, CH = 4;
  const int G = Cin / CH, P = 64 / G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* stg = stg_all[wave];
  const int g = lane % G, sub = lane / G;
  const int ci0 = g * CH;
  const int b = blockIdx.y, y0 = blockIdx.x * R;
  const int rows = min(R, Hin - y0);
  const int W2 = Win + 2;
  // delta window rows y0-1 .. y0+rows (output pixel (oy, ox) at [oy - y0 + 1][ox + 1])
  // window cells padded to 4 floats: one ds_read_b128 broadcast per tap
  for (int i = threadIdx.x; i < (R + 2) * W2 * 4; i += 256) {
    const int o = i & 3, c = (i >> 2) % W2, r = (i >> 2) / W2;
    const int oy = y0 - 1 + r, ox = c - 1;
    dl[i] = (o < NC && oy >= 0 && oy < Hin && ox >= 0 && ox < Win && r < rows + 2)
                ? delta[(((long)b * Hin + oy) * Win + ox) * NC + o]
                : 0.f;
  }
  float w[K * K][CH][NC];
#pragma unroll
  for (int t = 0; t < K * K; ++t)
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int o = 0; o < NC; ++o) w[t][c][o] = wpk[((long)t * Cin + ci0 + c) * NC + o];
  __syncthreads();
  const int npix = rows * Win;
  const long pbase = ((long)b * Hin + y0) * Win;
  // sign-bit masks: the next iteration's mask nibbles are loaded while this one computes
  unsigned mbn[UNR];
  if (hbits) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int pl = wave * P * UNR + u * P + sub;
      mbn[u] = pl < npix ? (hbits[((pbase + pl) * Cin + ci0) >> 3] >> (ci0 & 4)) & 15u : 0u;
    }
  }
  for (int p0 = wave * P * UNR; p0 < npix; p0 += 4 * P * UNR) {
    // the LReLU' mask source: the fp32 activation, or (hbits) its sign bits (nibble of this lane's 4 channels)
    f32x4 hv[UNR];
    unsigned mb[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int pl = p0 + u * P + sub;
      if (hbits) {
        mb[u] = mbn[u];
        const int pn = pl + 4 * P * UNR;
        mbn[u] = pn < npix ? (hbits[((pbase + pn) * Cin + ci0) >> 3] >> (ci0 & 4)) & 15u : 0u;
        hv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        mb[u] = 0u;
        hv[u] = pl < npix ? *reinterpret_cast<const f32x4*>(h + (pbase + pl) * Cin + ci0) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int pl = p0 + u * P + sub;
      if (p0 + u * P >= npix) break;  // wave-uniform (the flush below stores only the valid pixels)
      const int iy = pl / Win, ix = pl - iy * Win;
      float acc[CH] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          // output pixel (iy - 1 + ky, ix - 1 + kx) -> window [iy + ky][ix + kx]
          const f32x4 dv = *reinterpret_cast<const f32x4*>(dl + ((min(iy, rows - 1) + ky) * W2 + ix + kx) * 4);
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int o = 0; o < NC; ++o) acc[c] = fmaf(dv[o], w[ky * K + kx][c][o], acc[c]);
        }
      float v[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c)
        v[c] = acc[c] * (hbits ? (((mb[u] >> c) & 1u) ? 1.f : mask_slope) : act_grad_from_out(hv[u][c], mask_act, mask_slope));
      const bool live = pl < npix;
      const long pix = pbase + pl;
      if (!h3) {
        if (live) *reinterpret_cast<f32x4*>(h + pix * Cin + ci0) = f32x4{v[0], v[1], v[2], v[3]};
        continue;
      }
      // limbs of the 4 channels (2 per dword) into this wave's LDS image of the iteration's x3 rows
      unsigned lh[2], lm[2], ll[2];
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        unsigned short hh[2], mm[2], lo[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float x = v[2 * c2 + e];
          const __bf16 b0 = (__bf16)x;
          const float r1 = sub_rn(x, (float)b0);
          const __bf16 b1 = (__bf16)r1;
          hh[e] = __builtin_bit_cast(unsigned short, b0);
          mm[e] = __builtin_bit_cast(unsigned short, b1);
          lo[e] = __builtin_bit_cast(unsigned short, (__bf16)(sub_rn(r1, (float)b1)));
        }
        lh[c2] = hh[0] | ((unsigned)hh[1] << 16);
        lm[c2] = mm[0] | ((unsigned)mm[1] << 16);
        ll[c2] = lo[0] | ((unsigned)lo[1] << 16);
      }
      typedef unsigned u2 __attribute__((ext_vector_type(2)));
      unsigned char* q = stg + (u * P + sub) * 6 * Cin + (ci0 >> 3) * 48 + (ci0 & 4) * 2;
      *reinterpret_cast<u2*>(q) = u2{lh[0], lh[1]};
      *reinterpret_cast<u2*>(q + 16) = u2{lm[0], lm[1]};
      *reinterpret_cast<u2*>(q + 32) = u2{ll[0], ll[1]};
    }
    if (h3) {
      // the iteration's UNR*P consecutive pixels are one contiguous x3 span: 16-B chunks, 1 KiB per
      // wave-instruction
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int nv = (int)min((long)UNR * P, (long)npix - p0);
      const int nchunk = nv * 3 * Cin / 8;
      typedef unsigned u4 __attribute__((ext_vector_type(4)));
      u4* dst = reinterpret_cast<u4*>(h3 + (pbase + p0) * 3 * Cin);
      for (int c = lane; c < nchunk; c += 64) dst[c] = reinterpret_cast<const u4*>(stg)[c];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// k3 s1 p1 output-layer dgrad on the limb engine (sign-bit mask in, x3 limbs out).  Per 16 pixels it is the product
// dh^T (Cin x 16) = W^T (Cin x 9 NC) . D (9 NC x 16), D = the pixels' 3x3 delta windows (k = tap NC + o, zero past
// 9 NC <= 32 and outside the image): one 16x16x32 tile per 16 channels, six bf16 limb products each (fp32-accurate,
// as gemm_x3_kernel; the accumulation order differs from the VALU form's fmaf chain, not the accuracy).
// A workgroup's NG waves share a 16-pixel unit, wave w taking channels 64 w .. 64 w + 63 (four tiles): its W^T limb
// fragments (12 registers) are loaded once, the unit's D fragment and sign bits are loaded one unit ahead, and the
// unit's 16 x 384 B of limbs leave through a per-wave LDS image as whole 16-B chunks.  Output lane l holds channels
// 16 i + 4 (l >> 4) + r of pixel l & 15, so the LReLU' nibble of the sign bits applies directly.
// F32O (round 4): the gradient leaves as fp32 NHWC (4 B per element: the next dgrad stages its A operand as fp32,
// gemm_x3.hip X3_F32A) through a per-wave image of 272-B pixel rows (8 rows of a ds_write_b128 group on 8 distinct
// 4-bank groups), 4 wave-instructions of 16-B stores per unit; the values are the limb form's before its split.
// KT x KT taps at stride ST (round 4: also the k4 s2 p1 output layer of the 64x64 / 256x256 generators, whose K =
// 16 NC = 48 runs as two 32-deep k steps per limb product, both in one accumulation chain; pixel y's window is
// delta rows ST y - 1 .. ST y - 1 + KT - 1)
template <int NC, int NG, bool F32O = false, int KT = 3, int ST = 1>
__global__ __launch_bounds__(64 * NG) void smallc_dgrad_k3_mfma_kernel(int npix, int Hin, int Win,
                                                                      const float* __restrict__ wpk,
                                                                      const float* __restrict__ delta,
                                                                      float mask_slope, void* __restrict__ outp,
                                                                      const unsigned char* __restrict__ hbits) {
  constexpr int KK = KT * KT * NC, KS = (KK + 31) / 32;  // k values of a pixel's window, 32-deep k steps
  static_assert(KS <= 2, "at most two k steps");
  const int Hout = ST * Hin, Wout = ST * Win;
  typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
  constexpr int Cin = 64 * NG;
  // per-wave output image, pixel rows padded 384 -> 392 B (98 dwords): the 16 lanes of a ds_write_b64 group (16
  // pixels) then cover all 32 banks (at 384 B they all hit one: 16-way; at 400 B, 2-way); rows are 8-B aligned, so the
  // copy-out reads 8 B at a time
  constexpr int SROW = 392;
  __shared__ __attribute__((aligned(16))) unsigned char stg_all[NG][16 * SROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, m = lane & 15;
  unsigned char* const stg = stg_all[wave];
  // this wave's W^T limb fragments: tile t = channels 64 w + 16 t + m (rows), k = 8 q .. 8 q + 7
  bf16x8_t wa[KS][4][3];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ch = 64 * wave + 16 * t + m;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 32 * ks + 8 * q + e, tp = k / NC, o = k - tp * NC;
        const float v = k < KK ? wpk[((long)tp * Cin + ch) * NC + o] : 0.f;
        const __bf16 b0 = (__bf16)v;
        const float r1 = sub_rn(v, (float)b0);
        const __bf16 b1 = (__bf16)r1;
        wa[ks][t][0][e] = b0;
        wa[ks][t][1][e] = b1;
        wa[ks][t][2][e] = (__bf16)(sub_rn(r1, (float)b1));
      }
    }
  const int hw = Hin * Win;
  const int units = (npix + 15) >> 4;
  // every global access is a buffer access whose out-of-range offset reads zero / drops the store, so no load or store
  // sits in a branch (a store in a divergent branch made the compiler wait vmcnt(0) for it at every unit)
  const __amdgpu_buffer_rsrc_t rd =
      __builtin_amdgcn_make_buffer_rsrc((void*)delta, (short)0, npix * ST * ST * NC * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)hbits, (short)0, npix * (Cin / 8), 0x00020000);
  const __amdgpu_buffer_rsrc_t ro =
      __builtin_amdgcn_make_buffer_rsrc(outp, (short)0, npix * (F32O ? 4 : 6) * Cin, 0x00020000);
  constexpr int OOB = 0x7FFFFFF0;
  // the unit's loads: D's column for this lane's pixel (k = 8 q .. 8 q + 7) and the pixel's 8 sign-bit bytes of this
  // wave's 64 channels
  float dv[KS][8];
  unsigned mw0 = 0u, mw1 = 0u;
  auto load_unit = [&](int un) {
    const int pix = un * 16 + m;
    const bool live = un < units && pix < npix;
    const int b = live ? pix / hw : 0, rem = live ? pix - b * hw : 0;
    const int y = rem / Win, x = rem - y * Win;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 32 * ks + 8 * q + e, tp = k / NC, o = k - tp * NC;
        const int yy = ST * y + tp / KT - 1, xx = ST * x + tp % KT - 1;
        const bool ok = live && k < KK && (unsigned)yy < (unsigned)Hout && (unsigned)xx < (unsigned)Wout;
        dv[ks][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                  rd, ok ? ((((b * Hout + yy) * Wout + xx) * NC + o) * 4) : OOB, 0, 0));
      }
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    const u2 t = __builtin_bit_cast(u2, __builtin_amdgcn_raw_buffer_load_b64(rb, live ? pix * (Cin / 8) + 8 * wave : OOB,
                                                                             0, 0));
    mw0 = t[0];
    mw1 = t[1];
  };
  int un = blockIdx.x;
  load_unit(un);
  const int nsh = 8 * (q >> 1) + 4 * (q & 1);
  for (; un < units; un += gridDim.x) {
    bf16x8_t d0[KS], d1[KS], d2[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const __bf16 b0 = (__bf16)dv[ks][e];
        const float r1 = sub_rn(dv[ks][e], (float)b0);
        const __bf16 b1 = (__bf16)r1;
        d0[ks][e] = b0;
        d1[ks][e] = b1;
        d2[ks][e] = (__bf16)(sub_rn(r1, (float)b1));
      }
    const unsigned m0w = mw0, m1w = mw1;
    load_unit(un + gridDim.x);  // the next unit's loads land under this one's MFMAs and stores
    f32x4 c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the four tiles' six-MFMA chains interleaved (independent accumulators), smallest limb products first, each
    // limb product over the k steps in order
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks][t][2], d0[ks], c[t], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks][t][1], d1[ks], c[t], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks][t][0], d2[ks], c[t], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks][t][1], d0[ks], c[t], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks][t][0], d1[ks], c[t], 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks][t][0], d0[ks], c[t], 0, 0, 0);
    if constexpr (F32O) {
      constexpr int FROW = 272;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned nib = ((t < 2 ? m0w : m1w) >> (16 * (t & 1) + nsh)) & 15u;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = c[t][r] * (((nib >> r) & 1u) ? 1.f : mask_slope);
        *reinterpret_cast<f32x4*>(stg + m * FROW + (16 * t + 4 * q) * 4) = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      typedef unsigned u4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cidx = lane + 64 * j, px = cidx >> 4, w = cidx & 15;
        const u4 v = *reinterpret_cast<const u4*>(stg + px * FROW + w * 16);
        const bool ok = un * 16 + px < npix;
        __builtin_amdgcn_raw_buffer_store_b128(v, ro, ok ? ((un * 16 + px) * Cin + wave * 64) * 4 + w * 16 : OOB, 0, 0);
      }
    } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      // channels 64 w + 16 t + 4 q .. + 3: byte 2 t + (q >> 1) of the wave's 8, nibble q & 1
      const unsigned nib = ((t < 2 ? m0w : m1w) >> (16 * (t & 1) + nsh)) & 15u;
      unsigned short lh[4], lm[4], ll[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = c[t][r] * (((nib >> r) & 1u) ? 1.f : mask_slope);
        const __bf16 b0 = (__bf16)v;
        const float r1 = sub_rn(v, (float)b0);
        const __bf16 b1 = (__bf16)r1;
        lh[r] = __builtin_bit_cast(unsigned short, b0);
        lm[r] = __builtin_bit_cast(unsigned short, b1);
        ll[r] = __builtin_bit_cast(unsigned short, (__bf16)(sub_rn(r1, (float)b1)));
      }
      // image [16 pixels][8 octets x 48 B]: this lane's 4 channels at octet 2 t + (q >> 1), half q & 1
      typedef unsigned u2 __attribute__((ext_vector_type(2)));
      unsigned char* sp = stg + m * SROW + (2 * t + (q >> 1)) * 48 + (q & 1) * 8;
      *reinterpret_cast<u2*>(sp) = u2{lh[0] | ((unsigned)lh[1] << 16), lh[2] | ((unsigned)lh[3] << 16)};
      *reinterpret_cast<u2*>(sp + 16) = u2{lm[0] | ((unsigned)lm[1] << 16), lm[2] | ((unsigned)lm[3] << 16)};
      *reinterpret_cast<u2*>(sp + 32) = u2{ll[0] | ((unsigned)ll[1] << 16), ll[2] | ((unsigned)ll[3] << 16)};
    }
    // the unit's 16 x 384 B of this wave's channels leave as whole 16-B chunks (6 wave-instructions)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int cidx = lane + 64 * j, px = cidx / 24, w = cidx - px * 24;
      const u2 lo = *reinterpret_cast<const u2*>(stg + px * SROW + w * 16);
      const u2 hi = *reinterpret_cast<const u2*>(stg + px * SROW + w * 16 + 8);
      const bool ok = un * 16 + px < npix;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, u4{lo[0], lo[1], hi[0], hi[1]}), ro,
                                             ok ? (un * 16 + px) * 6 * Cin + wave * 384 + w * 16 : OOB, 0, 0);
    }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- two-stage output-layer forward -------------------------------------------------------
// Stage 1 (MFMA): per INPUT pixel p the per-tap projections P[p][n], n = (ky*K + kx)*NC + co,
//   P = h (npix x Cin) . Wp^T,  Wp packed [NTILE*32][Cin] (rows n >= K*K*NC are zero).
// A wave owns 32 pixels x 32 columns per 32-column tile (v_mfma_f32_32x32x2_f32).  Operands come
// straight from L2 as float4: lane (i = l&31, h = l>>5) loads h[p_i][8j + 4h .. +3] and
// Wp[n_i][8j + 4h .. +3]; element t of those feeds k-step 4j + t, i.e. half h covers
// k = 8j + 4h + t — the same bijection of k for A and B, so the sum is unchanged.
template <int NTILE>
__global__ __launch_bounds__(256) void smallc_proj_kernel(const float* __restrict__ h, long npix, int Cin,
                                                          const float* __restrict__ wp, float* __restrict__ P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long p0 = ((long)blockIdx.x * 4 + wave) * 32;
  if (p0 >= npix) return;
  const int i = lane & 31, hh = lane >> 5;
  const long pi = min(p0 + i, npix - 1);
  const float* hrow = h + pi * Cin + 4 * hh;
  f32x16 acc[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* wrow[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) wrow[t] = wp + (long)(32 * t + i) * Cin + 4 * hh;
#pragma unroll 8
  for (int j = 0; j < Cin; j += 8) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(hrow + j);
    f32x4 b[NTILE];
#pragma unroll
    for (int t = 0; t < NTILE; ++t) b[t] = *reinterpret_cast<const f32x4*>(wrow[t] + j);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < NTILE; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[t][e], acc[t], 0, 0, 0);
  }
  // C layout: col = lane & 31, row = (r&3) + 8(r>>2) + 4(lane>>5)
  const int ldp = NTILE * 32;
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long p = p0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (p < npix) P[p * ldp + 32 * t + i] = acc[t][r];
    }
}

// The same products in the same k order, with each wave's 32 pixels (one contiguous NHWC block) staged through LDS
// 64 channels at a time: whole 256-B row spans per load instruction instead of 32 B of 32 rows, the next chunk's
// loads in flight under the current chunk's MFMAs.  Row stride 68 floats: conflict-free ds_read_b128 fragments.
constexpr int PJ_KC = 64, PJ_RS = PJ_KC + 4;
template <int NTILE>
__global__ __launch_bounds__(256) void smallc_proj_lds_kernel(const float* __restrict__ h, long npix, int Cin,
                                                              const float* __restrict__ wp, float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) float st[4][32 * PJ_RS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long p0 = ((long)blockIdx.x * 4 + wave) * 32;
  const int i = lane & 31, hh = lane >> 5;
  float* ls = st[wave];
  f32x16 acc[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* wrow[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) wrow[t] = wp + (long)(32 * t + i) * Cin + 4 * hh;
  // staging: load q of a chunk covers rows 4q + lane/16, float4 lane%16 of the row's 64 channels
  f32x4 g[8];
  auto gload = [&](int c0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int row = 4 * q + (lane >> 4);
      const long pr = min(p0 + row, npix - 1);
      g[q] = *reinterpret_cast<const f32x4*>(h + pr * Cin + c0 + 4 * (lane & 15));
    }
  };
  gload(0);
  for (int c0 = 0; c0 < Cin; c0 += PJ_KC) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q)
      *reinterpret_cast<f32x4*>(ls + (4 * q + (lane >> 4)) * PJ_RS + 4 * (lane & 15)) = g[q];
    __syncthreads();
    if (c0 + PJ_KC < Cin) gload(c0 + PJ_KC);
#pragma unroll
    for (int j = 0; j < PJ_KC; j += 8) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ls + i * PJ_RS + j + 4 * hh);
      f32x4 b[NTILE];
#pragma unroll
      for (int t = 0; t < NTILE; ++t) b[t] = *reinterpret_cast<const f32x4*>(wrow[t] + c0 + j);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NTILE; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[t][e], acc[t], 0, 0, 0);
    }
  }
  const int ldp = NTILE * 32;
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long p = p0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (p < npix) P[p * ldp + 32 * t + i] = acc[t][r];
    }
}

// Stage 2: out[b,oy,ox,co] = bias + sum over the valid taps of P[input pixel][tap*NC + co], then tanh,
// x_hat (NCHW) and the residual delta = (x_hat - x)/s^2 * (1 - x_hat^2) (NHWC).  One thread per output pixel.
template <int NC, int K, int S>
__global__ __launch_bounds__(256) void smallc_gather_kernel(const float* __restrict__ P, const float* __restrict__ P1,
                                                            int ldp, int B, int Hin, int Win, int pad, int Hout, int Wout,
                                                            const float* __restrict__ bias, const float* x,
                                                            float inv_s2, float* delta, float* xhat,
                                                            float* sqerr_sum) {
  __shared__ float red[4];
  const long npix = (long)B * Hout * Wout;
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float sq = 0.f;
  if (pix < npix) {
    const int b = (int)(pix / ((long)Hout * Wout));
    const int rem = (int)(pix - (long)b * Hout * Wout);
    const int oy = rem / Wout, ox = rem - oy * Wout;
    float acc[NC];
#pragma unroll
    for (int o = 0; o < NC; ++o) acc[o] = bias ? bias[o] : 0.f;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int ty = oy + pad - ky;
      if (ty < 0 || (S == 2 && (ty & 1))) continue;
      const int iy = ty / S;
      if (iy >= Hin) continue;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int tx = ox + pad - kx;
        if (tx < 0 || (S == 2 && (tx & 1))) continue;
        const int ix = tx / S;
        if (ix >= Win) continue;
        const long po = (((long)b * Hin + iy) * Win + ix) * ldp + (ky * K + kx) * NC;
#pragma unroll
        for (int o = 0; o < NC; ++o) acc[o] += P1 ? P[po + o] + P1[po + o] : P[po + o];  // chunk partials in order
      }
    }
#pragma unroll
    for (int o = 0; o < NC; ++o) {
      const float t = tanhf(acc[o]);
      const long nchw = (((long)b * NC + o) * Hout + oy) * Wout + ox;
      if (xhat) xhat[nchw] = t;
      if (delta) {
        const float r = t - x[nchw];
        delta[pix * NC + o] = r * inv_s2 * (1.f - t * t);
        sq += r * r;
      }
    }
  }
  if (sqerr_sum) {
    sq = wave_sum(sq);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = red[0];
      for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t += red[w];
      atomicAdd(sqerr_sum, t * (0.5f * inv_s2));
    }
  }
}

// The k3 s1 gather through LDS: a workgroup takes R output rows of one sample, stages the R + 2 input rows' projection
// rows (9 NC taps each, the two chunk partials already added in order) with coalesced loads, then gathers from LDS with
// smallc_gather_kernel's arithmetic (same tap order, same adds), so the result is bitwise that kernel's.  The
// direct gather issued 27 (x 2 partials) scattered 4-B loads per output pixel: 36 us at CIFAR B=128.
template <int NC>
__global__ __launch_bounds__(256) void smallc_gather_lds_kernel(const float* __restrict__ P, const float* __restrict__ P1,
                                                                int ldp, int H, int W, int R,
                                                                const float* __restrict__ bias, const float* x,
                                                                float inv_s2, float* delta, float* xhat,
                                                                float* sqerr_sum) {
  constexpr int T = 9 * NC;
  extern __shared__ float pr[];  // [(R + 2) rows][W][T]
  __shared__ float red[4];
  const int b = blockIdx.x, r0 = blockIdx.y * R, rows = min(R, H - r0);
  const int n = (rows + 2) * W * T;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int rr = i / (W * T), rem = i - rr * (W * T), px = rem / T, t = rem - px * T;
    const int iy = r0 - 1 + rr;
    if (iy < 0 || iy >= H) continue;
    const long po = (((long)b * H + iy) * W + px) * ldp + t;
    pr[i] = P1 ? P[po] + P1[po] : P[po];
  }
  __syncthreads();
  float sq = 0.f;
  for (int p = threadIdx.x; p < rows * W; p += 256) {
    const int oy = r0 + p / W, ox = p - (p / W) * W;
    float acc[NC];
#pragma unroll
    for (int o = 0; o < NC; ++o) acc[o] = bias ? bias[o] : 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy + 1 - ky;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox + 1 - kx;
        if (ix < 0 || ix >= W) continue;
        const float* q = pr + ((iy - r0 + 1) * W + ix) * T + (ky * 3 + kx) * NC;
#pragma unroll
        for (int o = 0; o < NC; ++o) acc[o] += q[o];
      }
    }
    const long pix = ((long)b * H + oy) * W + ox;
#pragma unroll
    for (int o = 0; o < NC; ++o) {
      const float t = tanhf(acc[o]);
      const long nchw = (((long)b * NC + o) * H + oy) * W + ox;
      if (xhat) xhat[nchw] = t;
      if (delta) {
        const float rd = t - x[nchw];
        delta[pix * NC + o] = rd * inv_s2 * (1.f - t * t);
        sq += rd * rd;
      }
    }
  }
  if (sqerr_sum) {
    sq = wave_sum(sq);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sqerr_sum, (red[0] + red[1] + red[2] + red[3]) * (0.5f * inv_s2));
  }
}

// The k4 s2 p1 gather through LDS (round 4): a workgroup takes an R x CW tile of output pixels (R, CW even) of one
// sample; the R/2 + 2 x CW/2 + 2 input pixels its taps reach have their 16 NC projection values staged in LDS (the
// chunk partials already added in order), then smallc_gather_kernel's loops and adds run over LDS: bitwise that kernel.
template <int NC>
__global__ __launch_bounds__(256) void smallc_gather_s2_lds_kernel(const float* __restrict__ P,
                                                                   const float* __restrict__ P1, int ldp, int Hin,
                                                                   int Win, int R, int CW,
                                                                   const float* __restrict__ bias, const float* x,
                                                                   float inv_s2, float* delta, float* xhat,
                                                                   float* sqerr_sum) {
  constexpr int T = 16 * NC;
  extern __shared__ float pr[];  // [R/2 + 2][CW/2 + 2][T]
  __shared__ float red[4];
  const int Hout = 2 * Hin, Wout = 2 * Win;
  const int b = blockIdx.z, oy0 = blockIdx.y * R, ox0 = blockIdx.x * CW;
  const int IR = R / 2 + 2, IC = CW / 2 + 2, iy0 = oy0 / 2 - 1, ix0 = ox0 / 2 - 1;
  for (int i = threadIdx.x; i < IR * IC * T; i += 256) {
    const int rc = i / T, t = i - rc * T, r = rc / IC, c = rc - r * IC;
    const int iy = iy0 + r, ix = ix0 + c;
    if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;
    const long po = (((long)b * Hin + iy) * Win + ix) * ldp + t;
    pr[i] = P1 ? P[po] + P1[po] : P[po];
  }
  __syncthreads();
  float sq = 0.f;
  for (int p = threadIdx.x; p < R * CW; p += 256) {
    const int oy = oy0 + p / CW, ox = ox0 + p % CW;
    if (oy >= Hout || ox >= Wout) continue;
    float acc[NC];
#pragma unroll
    for (int o = 0; o < NC; ++o) acc[o] = bias ? bias[o] : 0.f;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      const int ty = oy + 1 - ky;
      if (ty < 0 || (ty & 1)) continue;
      const int iy = ty / 2;
      if (iy >= Hin) continue;
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const int tx = ox + 1 - kx;
        if (tx < 0 || (tx & 1)) continue;
        const int ix = tx / 2;
        if (ix >= Win) continue;
        const float* q = pr + ((iy - iy0) * IC + (ix - ix0)) * T + (ky * 4 + kx) * NC;
#pragma unroll
        for (int o = 0; o < NC; ++o) acc[o] += q[o];
      }
    }
    const long pix = ((long)b * Hout + oy) * Wout + ox;
#pragma unroll
    for (int o = 0; o < NC; ++o) {
      const float t = tanhf(acc[o]);
      const long nchw = (((long)b * NC + o) * Hout + oy) * Wout + ox;
      if (xhat) xhat[nchw] = t;
      if (delta) {
        const float rd = t - x[nchw];
        delta[pix * NC + o] = rd * inv_s2 * (1.f - t * t);
        sq += rd * rd;
      }
    }
  }
  if (sqerr_sum) {
    sq = wave_sum(sq);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sqerr_sum, (red[0] + red[1] + red[2] + red[3]) * (0.5f * inv_s2));
  }
}

// ------------------------------------------------------------------------------- shapes
// the two geometries the specialised kernels know: k3 s1 (CIFAR-10, MNIST) and k4 s2 (SVHN, CelebA), 1 or 3 colours
bool known_taps(const damc_layer_t& L) {
  return (L.cout == 1 || L.cout == 3) && ((L.k == 3 && L.stride == 1) || (L.k == 4 && L.stride == 2));
}
// register-resident kernels: the pixel's channels split over a power-of-two lane group (4 channels per lane at k3, 2 at k4)
bool smallc_reg_ok(const damc_layer_t& L) {
  if (!known_taps(L)) return false;
  const int CH = L.k == 3 ? 4 : 2;
  if (L.cin % CH) return false;
  const int G = L.cin / CH;
  return G <= 64 && (64 % G) == 0;
}
// the register-resident dgrad can write its gradient as x3 limbs (channel groups never straddle an octet)
bool smallc_x3_ok(const damc_layer_t& L) { return smallc_reg_ok(L) && L.cin % 8 == 0; }
// k3 s1 p1 output layer handled by smallc_dgrad_k3_kernel (reads sign bits / writes limbs)
bool smallc_k3(const damc_layer_t& L) {
  return L.kind == DAMC_LAYER_SMALLC && L.k == 3 && L.pad == 1 && L.hout == L.hin && L.wout == L.win &&
         smallc_x3_ok(L);
}
// k4 s2 p1 output layer with the limb-engine dgrad (Cin = 64, 128 or 256): the layer before it writes sign bits for it
// (against the register-resident VALU dgrad with the fp32 activation as mask: profiles/r04/smallc_s2_mfma_ab.txt)
bool smallc_s2_mfma(const damc_layer_t& L) {
  return L.kind == DAMC_LAYER_SMALLC && known_taps(L) && L.k == 4 && L.pad == 1 && L.hout == 2 * L.hin &&
         L.wout == 2 * L.win && (L.cin == 64 || L.cin == 128 || L.cin == 256);
}
// the limb-engine dgrad (sign bits in; limbs or fp32 out) has an instantiation: k3 at Cin = 128 or 256, k4 s2 as above
bool smallc_mfma_ok(const damc_layer_t& L) {
  return (smallc_k3(L) && (L.cin == 128 || L.cin == 256)) || smallc_s2_mfma(L);
}
// rows per workgroup of the k3 LDS-staged gather: at most what 60 KB of LDS holds (with the 2 halo rows), spread evenly
// over the strips
int gather_rows(const damc_layer_t& L) {
  const int gRmax = L.wout > 0 ? std::min(L.hout, 15360 / (L.wout * 9 * L.cout) - 2) : 0;
  return gRmax > 0 ? (L.hout + (L.hout + gRmax - 1) / gRmax - 1) / ((L.hout + gRmax - 1) / gRmax) : 0;
}
double smallc_flops(const damc_layer_t& L, int B) {
  return 2.0 * B * L.hout * L.wout * L.cout * L.cin * L.k * L.k / (L.stride * L.stride);
}

// ----------------------------------------------------------------------------- launchers
// out32: the fp32 gradient (in place of the activation) instead of limbs into h3
int launch_smallc_dgrad_k3_mfma(const damc_layer_t& L, int B, const float* delta, float mask_slope,
                                unsigned short* h3, const unsigned char* hbits, hipStream_t s, float* out32) {
  // the kernel addresses its operands through 32-bit buffer offsets: batches whose gradient image would reach 2^31
  // bytes (CelebA-HQ from B = 342 with limbs out, CIFAR from B = 2731) run in per-sample-aligned chunks (pixels never
  // interact across samples, so the chunking changes no result)
  const long hw = (long)L.hin * L.win;
  const long per_sample = hw * L.cin * (out32 ? 4 : 6);
  if (per_sample >= 2147483647L - 16) return DAMC_ERR_UNSUPPORTED;
  const int bc = (int)std::min<long>(B, (2147483647L - 16) / per_sample);
  // persistent grid: 1024 workgroups (CelebA-HQ B=64 step 8.03 / 8.06 -> 7.77 / 7.89 ms against 512, CIFAR B=128 within
  // noise; profiles/r04/smallc_dgrad_grid_ab.txt)
  constexpr int gmax = 1024;
  const int ng = L.cin / 64;
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int npix = (int)(std::min(bc, B - b0) * hw);
    const int units = (npix + 15) / 16;
    const int grid = std::max(1, std::min(units, gmax));
    const float* dl = delta + (long)b0 * L.hout * L.wout * L.cout;
    const unsigned char* hb = hbits + (long)b0 * hw * (L.cin / 8);
    float* o32 = out32 ? out32 + (long)b0 * hw * L.cin : nullptr;
    unsigned short* o3 = h3 ? h3 + (long)b0 * hw * L.cin * 3 : nullptr;
#define SDM(NC_, NG_, KT_, ST_)                                                                                    \
  if (o32)                                                                                                         \
    hipLaunchKernelGGL((smallc_dgrad_k3_mfma_kernel<NC_, NG_, true, KT_, ST_>), dim3(grid), dim3(64 * NG_), 0, s,    \
                       npix, L.hin, L.win, L.w_fwd, dl, mask_slope, (void*)o32, hb);                                \
  else                                                                                                             \
    hipLaunchKernelGGL((smallc_dgrad_k3_mfma_kernel<NC_, NG_, false, KT_, ST_>), dim3(grid), dim3(64 * NG_), 0, s,   \
                       npix, L.hin, L.win, L.w_fwd, dl, mask_slope, (void*)o3, hb)
    if (L.k == 4) {
      if (L.cout == 3 && ng == 4) SDM(3, 4, 4, 2);
      else if (L.cout == 3 && ng == 2) SDM(3, 2, 4, 2);
      else if (L.cout == 3) SDM(3, 1, 4, 2);
      else if (ng == 4) SDM(1, 4, 4, 2);
      else if (ng == 2) SDM(1, 2, 4, 2);
      else SDM(1, 1, 4, 2);
    } else {
      if (L.cout == 3 && ng == 4) SDM(3, 4, 3, 1);
      else if (L.cout == 3) SDM(3, 2, 3, 1);
      else if (ng == 4) SDM(1, 4, 3, 1);
      else SDM(1, 2, 3, 1);
    }
#undef SDM
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

// a register-resident instantiation (smallc_reg_ok(L)): the forward (h_in -> x_hat / delta / sqerr) or the dgrad
// (delta_in -> over h_out, or limbs into h3)
template <int NC>
void smallc_reg_dispatch(bool fwd, const damc_layer_t& L, const float* h_in, float* h_out, int B, const float* x,
                         float inv_s2, float* delta, const float* delta_in, float* xhat, float* sqerr, int mask_act,
                         float mask_slope, hipStream_t s, unsigned short* h3 = nullptr) {
  const int P = 64 / (L.cin / (L.k == 3 ? 4 : 2));  // pixels per wave
  const long npix = (fwd && L.k == 3) ? (long)B * L.hout * L.wout : (long)B * L.hin * L.win;
  const int grid = (int)std::max<long>(1, std::min<long>((npix + 4L * P - 1) / (4L * P), 1024));
  if (fwd) {
    if (L.k == 3)
      hipLaunchKernelGGL((smallc_fwd_reg_kernel<NC, 3, 1, 4>), dim3(grid), dim3(256), 0, s, h_in, B, L.hin, L.win,
                         L.cin, L.pad, L.hout, L.wout, L.w_fwd, L.bias, x, inv_s2, delta, xhat, sqerr);
    else
      hipLaunchKernelGGL((smallc_fwd_s2_kernel<NC, 2>), dim3(grid), dim3(256), 0, s, h_in, B, L.hin, L.win, L.cin,
                         L.w_fwd, L.bias, x, inv_s2, delta, xhat, sqerr);
  } else {
    if (L.k == 3)
      hipLaunchKernelGGL((smallc_dgrad_reg_kernel<NC, 3, 1, 4>), dim3(grid), dim3(256), 0, s, h_out, B, L.hin,
                         L.win, L.cin, L.pad, L.hout, L.wout, L.w_fwd, delta_in, mask_act, mask_slope, h3);
    else
      hipLaunchKernelGGL((smallc_dgrad_reg_kernel<NC, 4, 2, 2>), dim3(grid), dim3(256), 0, s, h_out, B, L.hin,
                         L.win, L.cin, L.pad, L.hout, L.wout, L.w_fwd, delta_in, mask_act, mask_slope, h3);
  }
}

// stage 1 of the two-stage forward: the per-tap projections of every input pixel into pbuf
int smallc_project(damc::SmallcFwd path, const damc_layer_t& L, const float* h, long npin, float* pbuf, hipStream_t s) {
  const int nt = damc::smallc_ntile(L);
  if (path == damc::SMALLC_FWD_PROJ16)
    return damc::launch_proj_rows(h, npin, L.cin, L.w_bwd, L.cin, 32 * nt, pbuf, npin * 32 * nt, s);
  // the round-3 projection kernels: LDS-staged when Cin is whole 64-channel chunks (CIFAR B=128: 63.5 -> 51.3 us for
  // projection + gather), else direct loads
  const int g1 = (int)((npin + 127) / 128);
  const bool lds = path == damc::SMALLC_FWD_PROJ_LDS;
  if (lds && nt == 1)
    hipLaunchKernelGGL((smallc_proj_lds_kernel<1>), dim3(g1), dim3(256), 0, s, h, npin, L.cin, L.w_bwd, pbuf);
  else if (lds)
    hipLaunchKernelGGL((smallc_proj_lds_kernel<2>), dim3(g1), dim3(256), 0, s, h, npin, L.cin, L.w_bwd, pbuf);
  else if (nt == 1)
    hipLaunchKernelGGL((smallc_proj_kernel<1>), dim3(g1), dim3(256), 0, s, h, npin, L.cin, L.w_bwd, pbuf);
  else
    hipLaunchKernelGGL((smallc_proj_kernel<2>), dim3(g1), dim3(256), 0, s, h, npin, L.cin, L.w_bwd, pbuf);
  return 0;
}

// stage 2: taps gathered from pbuf (P1: the second 128-channel chunk's partials, or nullptr), bias, tanh, residual
int smallc_gather(const damc_layer_t& L, int B, const float* pbuf, const float* P1, const float* x, float inv_s2,
                  float* delta, float* xhat, float* sqerr, hipStream_t s) {
  const int ldp = damc::smallc_ntile(L) * 32;
  switch (damc::smallc_gather_path(L, B)) {
    case damc::SMALLC_GATHER_K3_LDS: {
      const int gR = gather_rows(L);
      const size_t sm = (size_t)(gR + 2) * L.wout * 9 * L.cout * sizeof(float);
      const dim3 g(B, (L.hout + gR - 1) / gR);
      if (L.cout == 3)
        hipLaunchKernelGGL(smallc_gather_lds_kernel<3>, g, dim3(256), sm, s, pbuf, P1, ldp, L.hout, L.wout, gR, L.bias,
                           x, inv_s2, delta, xhat, sqerr);
      else
        hipLaunchKernelGGL(smallc_gather_lds_kernel<1>, g, dim3(256), sm, s, pbuf, P1, ldp, L.hout, L.wout, gR, L.bias,
                           x, inv_s2, delta, xhat, sqerr);
      break;
    }
    case damc::SMALLC_GATHER_S2_LDS: {
      const int R2 = 16, CW2 = 32;
      const size_t sm = (size_t)(R2 / 2 + 2) * (CW2 / 2 + 2) * 16 * L.cout * sizeof(float);
      const dim3 g((L.wout + CW2 - 1) / CW2, (L.hout + R2 - 1) / R2, B);
      if (L.cout == 3)
        hipLaunchKernelGGL(smallc_gather_s2_lds_kernel<3>, g, dim3(256), sm, s, pbuf, P1, ldp, L.hin, L.win, R2, CW2,
                           L.bias, x, inv_s2, delta, xhat, sqerr);
      else
        hipLaunchKernelGGL(smallc_gather_s2_lds_kernel<1>, g, dim3(256), sm, s, pbuf, P1, ldp, L.hin, L.win, R2, CW2,
                           L.bias, x, inv_s2, delta, xhat, sqerr);
      break;
    }
    case damc::SMALLC_GATHER_DIRECT: {
      // one wave per workgroup where 256-thread workgroups would leave CUs idle (CIFAR B=16: 256 workgroups of 64
      // instead of 64 of 256 -- a pixel's 54 scattered loads are latency-bound, so the CU count carries it); pixels are
      // independent
      const long npout = (long)B * L.hout * L.wout;
      const int tpb = (int)((npout + 255) / 256) < 512 ? 64 : 256;
      const int g2t = (int)((npout + tpb - 1) / tpb);
#define SG(NC_, K_, S_)                                                                                         \
  hipLaunchKernelGGL((smallc_gather_kernel<NC_, K_, S_>), dim3(g2t), dim3(tpb), 0, s, pbuf, P1, ldp, B, L.hin,  \
                     L.win, L.pad, L.hout, L.wout, L.bias, x, inv_s2, delta, xhat, sqerr)
      if (L.cout == 3) {
        if (L.k == 3) SG(3, 3, 1); else SG(3, 4, 2);
      } else {
        if (L.k == 3) SG(1, 3, 1); else SG(1, 4, 2);
      }
#undef SG
      break;
    }
  }
  return (int)hipGetLastError();
}

}  // namespace

namespace damc {

int smallc_ntile(const damc_layer_t& L) { return (L.k * L.k * L.cout + 31) / 32; }

// ------------------------------------------------------------------------------ the choices
SmallcFwd smallc_fwd_path(const damc_layer_t& L, bool have_pbuf, bool by_shape) {
  // two stages where the projection's MFMA kernels apply: they walk 8 channels a step over the packed w_bwd and hold
  // at most 2 column tiles (every known_taps layer has that few)
  if (!(have_pbuf && known_taps(L) && L.cin % 8 == 0 && smallc_ntile(L) <= 2 && L.w_bwd))
    return smallc_reg_ok(L) ? SMALLC_FWD_REG : SMALLC_FWD_GENERIC;
  // proj16 (gemm_x3.hip launch_proj_rows; the arithmetic of the fused ConvT epilogue) up to 256 channels
  const char* p16 = by_shape ? nullptr : getenv("DAMC_SMALLC_PROJ16");
  if (L.cin <= 256 && L.cin % 16 == 0 && !(p16 && p16[0] == '0')) return SMALLC_FWD_PROJ16;
  // the round-3 kernels: LDS-staged when Cin is whole 64-channel chunks, else direct loads
  const char* pe = by_shape ? nullptr : getenv("DAMC_SMALLC_PROJ_LDS");
  if (L.cin % PJ_KC == 0 && !(pe && atoi(pe) == 0)) return SMALLC_FWD_PROJ_LDS;
  return SMALLC_FWD_PROJ;
}

SmallcGather smallc_gather_path(const damc_layer_t& L, int B) {
  const char* gl = getenv("DAMC_SMALLC_GATHER_LDS");
  if (gl && gl[0] == '0') return SMALLC_GATHER_DIRECT;
  // k3 s1 p1, the same grid in and out: the LDS-staged gather (bitwise the direct one), only where the strips fill the
  // chip (at CIFAR B=16, 48 workgroups, it measured 10 us slower than the direct gather; at B=128, 384 workgroups,
  // 13 us faster; profiles/r04/gather_lds_ab.txt)
  const int gR = gather_rows(L);
  if (L.k == 3 && L.stride == 1 && L.pad == 1 && L.hin == L.hout && L.win == L.wout && gR >= 4 &&
      (long)B * ((L.hout + gR - 1) / gR) >= 256)
    return SMALLC_GATHER_K3_LDS;
  // k4 s2 p1: the LDS-staged gather over 16 x 32 output tiles (bitwise), where the tiles fill the chip
  if (L.k == 4 && L.stride == 2 && L.pad == 1 && L.hout == 2 * L.hin && L.wout == 2 * L.win && B <= 65535 &&
      (long)B * ((L.hout + 15) / 16) * ((L.wout + 31) / 32) >= 256)
    return SMALLC_GATHER_S2_LDS;
  return SMALLC_GATHER_DIRECT;
}

bool smallc_dgrad_reads_bits(const damc_layer_t& L) { return smallc_k3(L) || smallc_s2_mfma(L); }

SmallcGrad smallc_grad_form(const damc_layer_t& L, bool bits, bool limbs, bool f32a) {
  if (!limbs) return SMALLC_GRAD_F32;
  if (f32a && bits && smallc_mfma_ok(L)) return SMALLC_GRAD_F32A;
  return smallc_x3_ok(L) ? SMALLC_GRAD_LIMBS : SMALLC_GRAD_F32;  // F32: the caller splits it into limbs
}

SmallcDgrad smallc_dgrad_kernel_of(const damc_layer_t& L, bool bits, SmallcGrad form) {
  // the limb-engine form wherever sign bits come in (any batch: it runs in batch chunks below 2^31 bytes), except a k3
  // layer asked for the plain fp32 gradient (its producer is the first layer): the VALU kernel reads the bits too
  if (bits && smallc_mfma_ok(L) && (L.k == 4 || form != SMALLC_GRAD_F32)) return SMALLC_DGRAD_MFMA;
  if (smallc_k3(L)) return SMALLC_DGRAD_K3;
  return smallc_reg_ok(L) ? SMALLC_DGRAD_REG : SMALLC_DGRAD_GENERIC;
}

// ----------------------------------------------------------------------------- entry points
int smallc_fwd(const damc_layer_t& L, const float* h, int B, const float* x, float inv_s2, float* delta, float* xhat,
               float* sqerr, float* pbuf, hipStream_t s, bool p_ready) {
  const SmallcFwd path = smallc_fwd_path(L, pbuf != nullptr);
  if (p_ready && smallc_fwd_path(L, pbuf != nullptr, true) != SMALLC_FWD_PROJ16) return DAMC_ERR_ARG;
  if (path == SMALLC_FWD_GENERIC && (L.cout < 1 || L.cout > 4)) return DAMC_ERR_UNSUPPORTED;
  ProfScope ps("smallc_fwd", smallc_flops(L, B), s);
  switch (path) {
    case SMALLC_FWD_PROJ16:
    case SMALLC_FWD_PROJ_LDS:
    case SMALLC_FWD_PROJ: {
      const long npin = (long)B * L.hin * L.win;
      int rc;
      if (!p_ready && (rc = smallc_project(path, L, h, npin, pbuf, s))) return rc;
      // the proj16 forms (proj_rows_kernel and the fused epilogues) leave one partial per 128-channel chunk
      const bool chunks = (p_ready || path == SMALLC_FWD_PROJ16) && L.cin > PROJ_CHUNK;
      return smallc_gather(L, B, pbuf, chunks ? pbuf + npin * 32 * smallc_ntile(L) : nullptr, x, inv_s2, delta, xhat,
                           sqerr, s);
    }
    case SMALLC_FWD_REG:
      if (L.cout == 3)
        smallc_reg_dispatch<3>(true, L, h, nullptr, B, x, inv_s2, delta, nullptr, xhat, sqerr, 0, 0.f, s);
      else
        smallc_reg_dispatch<1>(true, L, h, nullptr, B, x, inv_s2, delta, nullptr, xhat, sqerr, 0, 0.f, s);
      break;
    case SMALLC_FWD_GENERIC: {
      const size_t sm = (size_t)L.k * L.k * L.cin * L.cout * sizeof(float);
      const long npix = (long)B * L.hout * L.wout;
      const int grid = (int)std::min<long>((npix + 3) / 4, 2048);
#define SC(NC_)                                                                                              \
  hipLaunchKernelGGL((smallc_fwd_kernel<NC_>), dim3(grid), dim3(256), sm, s, h, B, L.hin, L.win, L.cin, L.k, \
                     L.stride, L.pad, L.hout, L.wout, L.w_fwd, L.bias, x, inv_s2, delta, xhat, sqerr)
      switch (L.cout) {
        case 1: SC(1); break;
        case 2: SC(2); break;
        case 3: SC(3); break;
        default: SC(4); break;
      }
#undef SC
      break;
    }
  }
  return (int)hipGetLastError();
}

int smallc_dgrad(const damc_layer_t& L, float* h, int B, const float* delta, int mask_act, float mask_slope,
                 unsigned short* h3, const unsigned char* hbits, SmallcGrad form, hipStream_t s) {
  const SmallcDgrad kernel = smallc_dgrad_kernel_of(L, hbits != nullptr, form);
  unsigned short* const o3 = form == SMALLC_GRAD_LIMBS ? h3 : nullptr;  // else the fp32 gradient over h
  if (form == SMALLC_GRAD_LIMBS && !(h3 && smallc_x3_ok(L))) return DAMC_ERR_ARG;
  if (hbits && (!smallc_dgrad_reads_bits(L) || mask_act != DAMC_ACT_LRELU)) return DAMC_ERR_ARG;
  if (kernel == SMALLC_DGRAD_GENERIC && (L.cout < 1 || L.cout > 4)) return DAMC_ERR_UNSUPPORTED;
  ProfScope ps("smallc_dgrad", smallc_flops(L, B), s);
  switch (kernel) {
    case SMALLC_DGRAD_MFMA:
      return launch_smallc_dgrad_k3_mfma(L, B, delta, mask_slope, o3, hbits, s, o3 ? nullptr : h);
    case SMALLC_DGRAD_K3: {
      // 8 rows per block: 66.4 us vs 69.9 (4 rows, no prefetch) at the CIFAR B=128 shape; 16 rows leave CUs idle: 115 us
      // (profiles/r03/smallc_bench.txt holds a recorded run of that A/B); fewer rows per block when the batch would
      // leave fewer than 256 blocks (B=16: 60 us at 8 rows, 64 blocks).  Pixels are independent, so the row blocking
      // never changes a result
      int R = 8;
      while (R > 1 && (long)((L.hin + R - 1) / R) * B < 256) R >>= 1;
      const dim3 grid((unsigned)((L.hin + R - 1) / R), (unsigned)B);
      const size_t sm = sizeof(float) * (R + 2) * (L.win + 2) * 4;
      if (L.cout == 3)
        hipLaunchKernelGGL((smallc_dgrad_k3_kernel<3>), grid, dim3(256), sm, s, h, L.hin, L.win, L.cin, R, L.w_fwd,
                           delta, mask_act, mask_slope, o3, hbits);
      else
        hipLaunchKernelGGL((smallc_dgrad_k3_kernel<1>), grid, dim3(256), sm, s, h, L.hin, L.win, L.cin, R, L.w_fwd,
                           delta, mask_act, mask_slope, o3, hbits);
      break;
    }
    case SMALLC_DGRAD_REG:
      if (L.cout == 3)
        smallc_reg_dispatch<3>(false, L, nullptr, h, B, nullptr, 0.f, nullptr, delta, nullptr, nullptr, mask_act,
                               mask_slope, s, o3);
      else
        smallc_reg_dispatch<1>(false, L, nullptr, h, B, nullptr, 0.f, nullptr, delta, nullptr, nullptr, mask_act,
                               mask_slope, s, o3);
      break;
    case SMALLC_DGRAD_GENERIC: {
      const size_t sm = (size_t)L.k * L.k * L.cin * L.cout * sizeof(float);
      const long npix = (long)B * L.hin * L.win;
      const int grid = (int)std::min<long>((npix + 3) / 4, 2048);
#define SD(NC_)                                                                                                \
  hipLaunchKernelGGL((smallc_dgrad_kernel<NC_>), dim3(grid), dim3(256), sm, s, h, B, L.hin, L.win, L.cin, L.k, \
                     L.stride, L.pad, L.hout, L.wout, L.w_fwd, delta, mask_act, mask_slope)
      switch (L.cout) {
        case 1: SD(1); break;
        case 2: SD(2); break;
        case 3: SD(3); break;
        default: SD(4); break;
      }
#undef SD
      break;
    }
  }
  return (int)hipGetLastError();
}

}  // namespace damc
