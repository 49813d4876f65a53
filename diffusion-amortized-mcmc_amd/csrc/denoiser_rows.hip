// denoiser_rows.hip — the row-resident form of the amortizer's reverse sweep (_netQ_U.forward,
// workspace/src/diffusion_net.py:585-622; the toy's _netQ_U_toy, workspace/toy_example/src/diffusion_net.py:188-239).
//
// The seven ConcatSquash blocks never mix rows, so one 256-thread workgroup owns 16 rows and runs all n steps x 7
// blocks for them by itself: z, the block activations and the three skip outputs stay in LDS (one image row per
// latent row, below), and nothing is handed between workgroups: no flags, no sentinels, no wait, no rescue path.
// The weights are read from the workspace in the layout pack_denoiser_kernel writes for the launch chain
// ([ntn][16][kp], rows 0-7 Wl, 8-15 Ws of 8 output columns) as f32x4 B fragments of v_mfma_f32_16x16x4_f32, through
// the k-permutation of sweep_chain.hip (MFMA step s of k-group g reads k = 16 g + 4 (lane >> 4) + s on both operands);
// they stream from L2 once per step and workgroup, double-buffered 64 k ahead of the MFMAs.  Wave w takes the column
// tiles w, w + 4, ... two at a time over the whole K, each tile on two accumulator chains (even and odd k-groups):
// four independent chains per wave where a block has eight tiles or more, against the instruction's 40-cycle
// dependent latency (32 to issue).
//
// LDS image of a row (floats):  [ X0: sin cos z 0.. | U | o2 | T | o1 | P | o0 ]  kp0 + 10 w (o0 up to in1's padded K),
// + 4 of padding so the 16 rows of a ds_read_b128 fall on distinct banks.  in0 reads X0 and writes o0, in1 o0 -> o1, in2 o1 -> o2,
// mid o2 -> U, out0 [U | o2] -> T, out1 [T | o1] -> P, out2 [P | o0] -> z (inside X0): every cat() is one K range.
//
// The guided sweep (classifier-free guidance, diffusion_net.py:595-620) is the same kernel with GUIDED set: a workgroup
// owns 8 latent rows and holds each twice, image rows 0-7 on the conditional gates and 8-15 on the unconditional ones,
// so every weight fragment serves both evaluations of a step; the twins exchange eps in the last block's epilogue.
#include "denoiser_rows.h"

namespace damc {
namespace {

constexpr int RW_WAVES = 4, RW_THREADS = 64 * RW_WAVES;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// block j of step k for the workgroup's 16 rows: out = (x Wl^T + bl) gate + hb + (x Ws^T + bs), x = lrelu(src) (in0: src)
// GUIDED (classifier-free guidance, diffusion_net.py:603-606): image rows lr and lr + 8 are the conditional and the
// unconditional evaluation of latent row r0 + (lr & 7); they differ in the plane their gates come from, and meet in
// the FINAL epilogue
template <bool EMB, bool FINAL, bool GUIDED>
__device__ __forceinline__ void rows_block(const RowsArgs& a, const RowsBlock& b, float* lds, int k, int r0,
                                           const float* tb, uint64_t seed, uint64_t step_offset) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int LD = a.ld, niter = b.kp >> 6;
  const float* xrow = lds + m * LD + b.src + 4 * q;
  const int peer = (lane & 48) | ((m + 8) & 15);  // the lane holding the skip product of this lane's column
  for (int t = wave; t < b.ntn; t += 2 * RW_WAVES) {
    const bool two = t + RW_WAVES < b.ntn;
    const float* w0 = b.w + ((long)t * 16 + m) * b.kp + 4 * q;
    const float* w1 = two ? w0 + (long)RW_WAVES * 16 * b.kp : w0;
    f32x4 wa[4], wb[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      wa[g] = ld4(w0 + 16 * g);
      wb[g] = ld4(w1 + 16 * g);
    }
    // epilogue operands (independent of the products): lane (m < 8, q) owns column 8 t + m of rows 4 q + r
    float gate[2][4], hb[2][4], bias[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ti = t + i * RW_WAVES, c = 8 * ti + m;
      const bool cok = (i == 0 || two) && m < 8 && c < b.dout;
      bias[i] = (i == 0 || two) ? b.bls[ti * 16 + m] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = GUIDED ? r0 + ((4 * q + r) & 7) : r0 + 4 * q + r;
        gate[i][r] = hb[i][r] = 0.f;
        if (cok && row < a.B) {
          const float* plane = (GUIDED && 4 * q + r >= 8) ? a.gh_u : a.gh;
          const float* ghr = plane + ((long)k * a.B + row) * a.ldgh + b.ghoff + c;
          gate[i][r] = ghr[0];
          hb[i][r] = ghr[b.dout];
        }
      }
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[i][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < niter; ++it) {
      f32x4 ca[4], cb[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        ca[g] = wa[g];
        cb[g] = wb[g];
      }
      if (it + 1 < niter) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          wa[g] = ld4(w0 + 64 * (it + 1) + 16 * g);
          wb[g] = ld4(w1 + 64 * (it + 1) + 16 * g);
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int kk = 64 * it + 16 * g + 4 * q;
        f32x4 x = ld4(xrow + 64 * it + 16 * g);
        if (kk >= b.din) x = f32x4{0.f, 0.f, 0.f, 0.f};  // past K the image holds other data (the weights there are 0)
        if (!EMB) {
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = x[e] > 0.f ? x[e] : 0.01f * x[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[0][g & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[e], ca[g][e], acc[0][g & 1], 0, 0, 0);
          if (two) acc[1][g & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[e], cb[g][e], acc[1][g & 1], 0, 0, 0);
        }
      }
    }
    // C layout 16x16x4: column = lane & 15 (0-7 Wl, 8-15 Ws), rows 4 (lane >> 4) + r
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ti = t + i * RW_WAVES, c = 8 * ti + m;
      const f32x4 s = acc[i][0] + acc[i][1];
      const float bs = __shfl(bias[i], peer, 64), bl = bias[i];
      float sk[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) sk[r] = __shfl(s[r], peer, 64);
      if (!((i == 0 || two) && m < 8 && c < b.dout)) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 4 * q + r, row = GUIDED ? r0 + (lr & 7) : r0 + lr;
        // ConcatSquashLinearSkipCtx.forward, the fma spelled out as in chain_kernel: every sweep form rounds alike
        const float o = __builtin_fmaf(s[r] + bl, gate[i][r], hb[i][r]) + (sk[r] + bs);
        float* dst = lds + lr * LD + b.dst + c;
        if (!FINAL) {
          *dst = o;
          continue;
        }
        // reverse step (diffusion_net.py:601-620): eps = z + out; pred = c0 (z - eps c1)
        const float zv = *dst;
        float eps = a.residual ? zv + o : o;
        if (GUIDED) {
          // the twin's eps of this column sits in lane ^ 32 (rows 4 (lane >> 4) + r; the pair shares m and c, so both
          // lanes are here); (1 + cond_w) * eps_pred - cond_w * eps_pred_unc, each op rounded, in both twins
          const float other = __shfl_xor(eps, 32, 64);
          const float ec = lr < 8 ? eps : other, eu = lr < 8 ? other : eps;
          eps = sub_rn(mul_rn(a.gw1, ec), mul_rn(a.gw, eu));
        }
        const bool last = tb[5] != 0.f;
        if ((!GUIDED || lr < 8) && row < a.B && a.eps_log && k < a.eps_log_steps)
          a.eps_log[((long)k * a.B + row) * a.nz + c] = eps;
        const float pred = mul_rn(tb[0], sub_rn(zv, mul_rn(eps, tb[1])));
        float zn = pred;
        if (!last) {
          zn = add_rn(mul_rn(tb[2], zv), mul_rn(tb[3], pred));
          if (a.with_noise && row < a.B) {
            const int noisy_k = (int)tb[6];
            float xi;
            if (a.noise) {
              xi = a.noise[((long)noisy_k * a.B + row) * a.nz + c];
            } else {
              float n4[4];
              philox_normal4(seed, a.chain_base + row, step_offset + noisy_k, (uint32_t)(c >> 2), DAMC_STREAM_SWEEP,
                             n4);
              xi = pick4(n4, c);
            }
            zn = add_rn(zn, mul_rn(tb[4], xi));
          }
        }
        *dst = zn;
      }
    }
  }
  __syncthreads();
}

// GUIDED: the workgroup's 16 image rows are its 8 latent rows twice (rows_block); both twins start every step from
// the same z, so the embedding below is evaluated per image row like everything else
template <bool GUIDED>
__global__ __launch_bounds__(RW_THREADS) void sweep_rows_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [16][a.ld]
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * (GUIDED ? ROWS_GTM : ROWS_TM);
  const int nz = a.nz, half = nz >> 1, LD = a.ld;
  const int zoff = 2 * half;  // z within X0
  uint64_t seed = a.seed, step_offset = a.step_offset;
  draw_key(a.draws, seed, step_offset);
  for (int i = tid; i < ROWS_TM * nz; i += RW_THREADS) {
    const int r = i / nz, c = i - r * nz;
    const int row = GUIDED ? r0 + (r & 7) : r0 + r;
    lds[r * LD + zoff + c] = row < a.B ? a.zt[(long)row * nz + c] : 0.f;
  }
  __syncthreads();
  // in0's Fourier embedding: up to four (row, column) outputs of zB per thread, their k loops interleaved
  constexpr int EPT = 4;  // 16 rows x 64 columns (nz <= 128) over 256 threads
  for (int k = 0; k < a.n; ++k) {
    float tb[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) tb[i] = a.tab[8 * k + i];
    {
      float acc[EPT];
      const float *zr[EPT], *br[EPT];
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const int idx = tid + i * RW_THREADS;
        const bool ok = idx < ROWS_TM * half;
        const int r = ok ? idx / half : 0, c = ok ? idx - r * half : 0;
        zr[i] = lds + r * LD + zoff;
        br[i] = a.bmat + (long)c * nz;
        acc[i] = 0.f;
      }
      for (int kk = 0; kk < nz; kk += 2)
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          acc[i] = __builtin_fmaf(zr[i][kk], br[i][kk], acc[i]);
          acc[i] = __builtin_fmaf(zr[i][kk + 1], br[i][kk + 1], acc[i]);
        }
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const int idx = tid + i * RW_THREADS;
        if (idx < ROWS_TM * half) {
          const int r = idx / half, c = idx - r * half;
          // the reference's argument, 2 pi (zB) rounded to fp32, and the full-precision functions (input_emb)
          const float arg = mul_rn(6.283185307179586f, acc[i]);
          lds[r * LD + c] = sinf(arg);
          lds[r * LD + half + c] = cosf(arg);
        }
      }
    }
    __syncthreads();
    rows_block<true, false, GUIDED>(a, a.b[0], lds, k, r0, tb, seed, step_offset);
#pragma unroll 1
    for (int j = 1; j < 6; ++j) rows_block<false, false, GUIDED>(a, a.b[j], lds, k, r0, tb, seed, step_offset);
    rows_block<false, true, GUIDED>(a, a.b[6], lds, k, r0, tb, seed, step_offset);
  }
  for (int i = tid; i < (GUIDED ? ROWS_GTM : ROWS_TM) * nz; i += RW_THREADS) {
    const int r = i / nz, c = i - r * nz;
    if (r0 + r < a.B) a.zt[(long)(r0 + r) * nz + c] = lds[r * LD + zoff + c];
  }
}

__global__ void narrow_linear_kernel(const float* A, long lda, int M, int K, int silu_a, const float* W, long ldw,
                                     const float* bias, int N, int npad, float* Y, long ldy) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * npad) return;
  const long mrow = i / npad;
  const int c = (int)(i - mrow * npad);
  float v = 0.f;
  if (c < N) {
    for (int k = 0; k < K; ++k) {
      float x = A[mrow * lda + k];
      if (silu_a) x = x / (1.f + expf(-x));
      v = __builtin_fmaf(x, W[(long)c * ldw + k], v);
    }
    if (bias) v += bias[c];
  }
  Y[mrow * ldy + c] = v;
}

__global__ void narrow_hyper_kernel(const float* cx, long ldc, long M, int dout, const float* wg, const float* bg,
                                    const float* wb, float* gh, long ldgh) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * dout) return;
  const long r = i / dout;
  const int c = (int)(i - r * dout);
  float g = 0.f, h = 0.f;
  for (int k = 0; k < dout; ++k) {
    const float x = cx[r * ldc + k];
    g = __builtin_fmaf(x, wg[(long)c * dout + k], g);
    h = __builtin_fmaf(x, wb[(long)c * dout + k], h);
  }
  g += bg[c];
  gh[r * ldgh + c] = 1.f / (1.f + expf(-g));
  gh[r * ldgh + dout + c] = h;
}

}  // namespace

int rows_layout(int nz, int w, int kp0, RowsBlock* b) {
  const int U = kp0, o2 = U + 2 * w, T = o2 + 2 * w, o1 = T + 2 * w, P = o1 + 2 * w, o0 = P + w;
  const int src[7] = {0, o0, o1, o2, U, T, P};
  const int dst[7] = {o0, o1, o2, U, T, P, 2 * (nz / 2)};
  for (int j = 0; j < 7; ++j) {
    b[j].src = src[j];
    b[j].dst = dst[j];
  }
  // in1 reads o0 over its padded K, and out2 reads [P | o0] over its own: at 32 < w % 64 < 64 (48, 112, 176, 240 of
  // the multiples of 16) pad64(2 w) reaches past o0's pad64(w), and launch_rows refuses an image a block reads beyond
  const int p64 = (w + 63) / 64 * 64, p2 = (2 * w + 63) / 64 * 64;
  return (o0 + p64 > P + p2 ? o0 + p64 : P + p2) + 4;
}

namespace {

template <bool GUIDED>
int launch_rows(const RowsArgs& a, hipStream_t s) {
  const size_t smem = (size_t)ROWS_TM * a.ld * sizeof(float);
  if (smem > ROWS_LDS_MAX || (a.ld & 3) || a.nz > 128 || (a.nz & 1)) return DAMC_ERR_UNSUPPORTED;
  for (int j = 0; j < 7; ++j)
    if ((a.b[j].kp & 63) || (a.b[j].din & 3) || a.b[j].din > a.b[j].kp || ((a.b[j].src | (j < 6 ? a.b[j].dst : 0)) & 3) ||
        a.b[j].src + a.b[j].kp > a.ld)
      return DAMC_ERR_UNSUPPORTED;
  static const bool lds_ok = hipFuncSetAttribute((const void*)sweep_rows_kernel<GUIDED>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)ROWS_LDS_MAX) == hipSuccess;
  if (!lds_ok) return DAMC_ERR_UNSUPPORTED;
  const int tm = GUIDED ? ROWS_GTM : ROWS_TM;
  hipLaunchKernelGGL(sweep_rows_kernel<GUIDED>, dim3((unsigned)((a.B + tm - 1) / tm)), dim3(RW_THREADS), smem, s, a);
  return (int)hipGetLastError();
}

}  // namespace

int launch_sweep_rows(const RowsArgs& a, hipStream_t s) { return launch_rows<false>(a, s); }

int launch_sweep_rows_guided(const RowsArgs& a, hipStream_t s) {
  if (!a.gh_u) return DAMC_ERR_ARG;
  return launch_rows<true>(a, s);
}

int launch_narrow_linear(const float* A, long lda, int M, int K, int silu_a, const float* W, long ldw, const float* bias,
                         int N, int npad, float* Y, long ldy, hipStream_t s) {
  const long tot = (long)M * npad;
  hipLaunchKernelGGL(narrow_linear_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, A, lda, M, K, silu_a, W,
                     ldw, bias, N, npad, Y, ldy);
  return (int)hipGetLastError();
}

int launch_narrow_hyper(const float* cx, long ldc, long M, int dout, const float* wg, const float* bg, const float* wb,
                        float* gh, long ldgh, hipStream_t s) {
  const long tot = M * dout;
  hipLaunchKernelGGL(narrow_hyper_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, cx, ldc, M, dout, wg, bg,
                     wb, gh, ldgh);
  return (int)hipGetLastError();
}

}  // namespace damc
