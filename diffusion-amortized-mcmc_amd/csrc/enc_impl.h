// enc_impl.h — what more than one of the encoder's files shares: the Welford record and its merge, the wave
// reduce-scatter, the statistics partition, the dense head's two tile constants that the workspace layout reads, and
// the host launchers that damc_q_encoder_fwd (encoder.hip) calls in enc_norm.hip and enc_first.hip.  Included only by
// encoder.hip, enc_norm.hip, enc_first.hip and enc_head.hip; everything else goes through include/damc.h
// (launch_dense_head_x3, which encoder_train.hip calls too, is declared in gemm.h).  It defines no variable and no
// function that is not inline.
#pragma once
#include "gemm.h"

namespace damc {

// ---- per-(sample, channel) statistics: Welford partials merged with Chan's formula (enc_norm.hip, enc_first.hip)
struct Wf {
  float n, mean, m2;
};
__device__ __forceinline__ Wf wmerge(Wf a, Wf b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float d = b.mean - a.mean;
  const float fb = b.n / n;
  Wf r;
  r.n = n;
  r.mean = a.mean + d * fb;
  r.m2 = a.m2 + b.m2 + d * d * a.n * fb;
  return r;
}

// wave reduce-scatter of N per-lane values: halving exchanges (N/2 + N/4 + ... shuffles instead of 6 N), then a plain
// butterfly over the lanes left sharing a channel; every lane returns the wave total of channel ch (fixed order)
// (conv3_in_fused_kernel in enc_first.hip, in_fused_x3_kernel in enc_norm.hip)
template <int N>
__device__ __forceinline__ float wave_rsum(const float (&v)[N], int lane, int off, int& ch, int stop = 1) {
  if constexpr (N == 1) {
    float s = v[0];
    for (; off >= stop; off >>= 1) s += __shfl_xor(s, off);
    return s;
  } else {
    constexpr int H = N / 2;
    const bool hi = (lane & off) != 0;
    float nv[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const float keep = hi ? v[H + i] : v[i], send = hi ? v[i] : v[H + i];
      nv[i] = keep + __shfl_xor(send, off);
    }
    ch = 2 * ch + (hi ? 1 : 0);
    return wave_rsum<H>(nv, lane, off >> 1, ch, stop);
  }
}

// pixel splits of the statistics pass: <= 64 pixels per split (the Welford chain of a thread is serial),
// merged with Chan's formula
inline int in_splits(int hw) {
  int s = hw / 64;
  return s < 1 ? 1 : (s > 64 ? 64 : s);
}

// the dense head's column tile and sign block (enc_head.hip; enc_shapes sizes the head's slabs with them)
constexpr int HD_BN = 64, HD_NEGK = 512;

// ---- the forward's steps outside encoder.hip.  Each returns 0 or an error code; every DAMC_ENC_* switch is read by
// damc_q_encoder_fwd and arrives here as a plain bool.

// enc_first.hip: layer 0 (Conv2d k3 s1 p1 on nc = 1, 3 or 4 channels + InstanceNorm + LeakyReLU) from the caller's NCHW
// image straight to layer 1's input: its limbs at a3, or fp32 NHWC at y32 where y32 != NULL.  rows / strips: the
// two-pass forms' partition of a sample (EncShapes::first_rows, first_strips); inws: strips * 3 + 2 floats per
// (sample, channel).  onepass / mfma allow conv3_in_fused_kernel / conv3_mfma_kernel where the shape fits them, px1
// keeps the fmaf statistics pass at one pixel per lane.  The packing list pl runs here unless *pl_done: as extra
// workgroups of the one-pass kernel, or in a launch of its own before the two passes; *pl_done is then set.
int launch_enc_first(const damc_enc_layer_t& L, const float* x, int B, int H, int W, int rows, int strips, bool onepass,
                     bool mfma, bool px1, float* inws, unsigned short* a3, float* y32, const PackConvList& pl,
                     bool* pl_done, hipStream_t s);

// enc_norm.hip: InstanceNorm + LeakyReLU of layer L's stored conv output y (B, hw, cout) NHWC to the next conv's input
// in one kernel (in_fused_x3_kernel; hw <= 256, cout % 32 == 0): limbs at a3, or fp32 at y32 (NHWC, may be y itself;
// chw: CHW rows for the dense head, y32 then another buffer).  ks > 0: y was not written, the kernel sums the conv's
// ks split-K slabs at kslab itself
int launch_in_onepass(const damc_enc_layer_t& L, const float* y, int B, int hw, unsigned short* a3, float* y32, int chw,
                      const float* kslab, int ks, hipStream_t s);
// the same norm as statistics, merge and apply kernels (cout % 8 == 0): limbs at a3, or fp32 in place (f32_out).
// strip: the 256-pixel strip partition (hw % 256 == 0), whose partials the conv's epilogue left in inws (strip_done) or
// in_strip_stats_kernel takes here; else in_stats_kernel's in_splits(hw).  inws: S * 3 + 2 floats per (sample, channel)
int launch_in_threepass(const damc_enc_layer_t& L, float* y, int B, int hw, bool strip, bool strip_done, float* inws,
                        unsigned short* a3, bool f32_out, hipStream_t s);
// its middle kernel alone (in_merge_kernel), which the first layer's two-pass forms run between their passes: the S
// partials [B][C][S][3] at part to (scale, shift) [B][2][C] at ss.  Launches only; the caller checks the launch
void launch_in_merge(const float* part, int B, int C, int S, const float* gamma, const float* beta, float eps,
                     float* ss, hipStream_t s);

}  // namespace damc
