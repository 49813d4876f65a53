// sweep_stages.hip — the per-call stages of the reverse sweep and the guided sweep (denoiser.hip): everything that
// does not depend on zt, computed once per call for all n * B (step, row) pairs before the dependent chain runs.
//   1. stage_pack  : every weight from the caller's PyTorch layouts into the workspace (pack_denoiser_kernel,
//                    transpose_kernel; the nets train between calls);
//   2. stage_time  : the time MLP on the n sinusoidal embeddings and its part of every block's ctx Linear, qt (n, S);
//      stage_px    : the xemb part, px = SiLU(xemb) Wx^T; both on skinny_gemm_kernel where the widths allow it,
//                    on the fp32 GEMM engine (gemm.hip) otherwise;
//      launch_ctx  : c[k][b] = SiLU(px[b] + qt[k]) (ctx4_kernel / ctx_kernel);
//   3. stage_hyper : per block [gate | hyper bias] = [sigmoid(c Wg^T + bg) | c Wb^T] over the n * B rows, on the
//                    limb product (hyper_x3_kernel) or the fp32 engine's EPI_GATE.
// out2 of a denoiser with nz % 4 != 0 takes the narrow kernels of denoiser_rows.hip in stages 2 and 3.
// Process-wide host state defined here: hyper_x3_kernel's LDS attribute, set once (stage_hyper).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "denoiser_rows.h"
#include "sweep_impl.h"

using namespace damc;

namespace {

// ------------------------------------------------------------------------------ skinny GEMMs of the precompute
// Y[m][n] = act(sum_k f(A[m][k]) W[n][k] + bias[n]) for the sweep's short-M products (the time MLP and qt over
// n steps, px over B rows): the chain kernel's tile (16 rows x 16 columns, K split over 4 waves, every lane's
// f32x4 loads of a chunk in flight together) so a product of a few hundred rows fills the chip with one memory
// round trip per chunk, where 128 x 128 tiles would give it 9 workgroups walking K serially.  W is read in its
// PyTorch (out, in) layout; the N columns are up to 7 segments with their own weight rows and bias (the 7
// blocks' ctx Linears side by side).
struct SkSeg {
  const float* w;     // row n - n0 of the segment at w + (n - n0) * ldw
  const float* bias;  // or null
  long ldw;
  int n0;
};
struct SkArgs {
  const float* A;
  long lda;
  int M, N, K;
  SkSeg seg[7];
  int nseg;
  int silu_a, silu_y;
  float* Y;
  long ldy;
};

__global__ __launch_bounds__(256) void skinny_gemm_kernel(SkArgs a) {
  __shared__ __attribute__((aligned(16))) float red[4][16][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int ntn = a.N >> 4;
  const int tn = blockIdx.x % ntn, tm = blockIdx.x / ntn;
  const int r0 = tm * 16, n0 = tn * 16;
  int sg = 0;
  while (sg + 1 < a.nseg && a.seg[sg + 1].n0 <= n0) ++sg;
  const SkSeg& S = a.seg[sg];
  const int kq = ((a.K + 63) >> 6) << 4;  // per-wave K span, whole 16-deep k-groups
  const int kbase = wave * kq;
  const int row = r0 + m, col = n0 + m;
  const bool rok = row < a.M;
  const float* arow = a.A + (long)row * a.lda;
  const float* wrow = S.w + (long)(col - S.n0) * S.ldw;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int g0 = 0; g0 < kq; g0 += 16 * CH_CHUNK) {
    f32x4 xa[CH_CHUNK], wb[CH_CHUNK];
#pragma unroll
    for (int c = 0; c < CH_CHUNK; ++c) {
      const int k = kbase + g0 + 16 * c + 4 * q;
      const bool ok = g0 + 16 * c < kq && k < a.K;
      xa[c] = (ok && rok) ? *reinterpret_cast<const f32x4*>(arow + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      wb[c] = ok ? *reinterpret_cast<const f32x4*>(wrow + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < CH_CHUNK; ++c) {
      f32x4 x = xa[c];
      if (a.silu_a) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] / (1.f + expf(-x[e]));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[e], wb[c][e], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * q + r][m] = acc[r];
  __syncthreads();
  const int er = tid >> 4, ec = tid & 15;
  const int orow = r0 + er, ocol = n0 + ec;
  if (orow >= a.M) return;
  float v = ((red[0][er][ec] + red[1][er][ec]) + red[2][er][ec]) + red[3][er][ec];
  if (S.bias) v += S.bias[ocol - S.n0];
  if (a.silu_y) v = v / (1.f + expf(-v));
  a.Y[(long)orow * a.ldy + ocol] = v;
}

int launch_skinny(const SkArgs& a, const char* prof, hipStream_t s) {
  if (a.M <= 0 || (a.N & 15) || (a.K & 3) || (a.lda & 3) || a.nseg < 1 || a.nseg > 7) return DAMC_ERR_UNSUPPORTED;
  for (int i = 0; i < a.nseg; ++i)
    if ((a.seg[i].ldw & 3) || (a.seg[i].n0 & 15)) return DAMC_ERR_UNSUPPORTED;
  ProfScope ps(prof, 2.0 * a.M * a.N * a.K, s);
  const unsigned grid = (unsigned)(((a.M + 15) / 16) * (a.N / 16));
  hipLaunchKernelGGL(skinny_gemm_kernel, dim3(grid), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------- per-call helpers
__global__ void silu_kernel(const float* x, long n, float* y) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    y[i] = v / (1.f + expf(-v));
  }
}

// c[k][b][s] = SiLU(px[k * pxstep + b * S + s] + qt[k][s]): pxstep 0 for the one px of a sweep's xemb, B S for a px
// per step (the guided sweep's unconditional embeddings)
__global__ void ctx_kernel(const float* __restrict__ px, long pxstep, const float* __restrict__ qt, int B, int S,
                           long total, float* __restrict__ c) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long per = (long)B * S;
  const long k = i / per;
  const long r = i - k * per;
  const int s = (int)(r % S);
  const float u = px[k * pxstep + r] + qt[k * S + s];
  c[i] = u / (1.f + expf(-u));
}

// the same, 4 columns per thread (S % 4 == 0), grid.y = step: no 64-bit division per element, and SiLU on the
// transcendental unit (exp2 and reciprocal, ~1 ulp each) unless exact (DAMC_SWEEP_HYPER_SIGMOID=exact: ctx_kernel's
// expf and IEEE division); 16 M SiLUs per CIFAR sweep
__global__ __launch_bounds__(256) void ctx4_kernel(const float* __restrict__ px, long pxstep,
                                                   const float* __restrict__ qt, int BS, int S, int exact,
                                                   float* __restrict__ c) {
  const int r4 = 4 * (blockIdx.x * 256 + threadIdx.x), k = blockIdx.y;
  if (r4 >= BS) return;
  const int s = r4 % S;
  const f32x4 a = *reinterpret_cast<const f32x4*>(px + k * pxstep + r4),
              b = *reinterpret_cast<const f32x4*>(qt + (long)k * S + s);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float u = a[e] + b[e];
    o[e] = exact ? u / (1.f + expf(-u)) : u * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-u * 1.4426950408889634f));
  }
  *reinterpret_cast<f32x4*>(c + (long)k * BS + r4) = o;
}

struct PackBlock {
  const float *wl, *bl, *ws, *bs, *wg, *bg, *wb, *wctx, *bctx;
  int din, dout, kp, coloff;
  float *w, *bls, *wgb, *bg2;
};
struct PackArgs {
  PackBlock b[7];
  int ntemb, nxemb, S;
  float *wctx_t, *wctx_x, *bctx;
};

// grid.y = block, grid.z = part: 0 chain weights [tile][16][kp] + biases, 1 [Wg^T | Wb^T] (dout, 2 dout) + [bg | 0],
// 2 the block's columns of Wctx_t (ntemb, S), Wctx_x (nxemb, S) and bctx (S)
__global__ void pack_denoiser_kernel(PackArgs pa) {
  const PackBlock& b = pa.b[blockIdx.y];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.z == 0) {
    const int ntn = (b.dout + TC - 1) / TC;
    const long n = (long)ntn * 16 * b.kp;
    if (i < n) {
      const int k = (int)(i % b.kp);
      const long rr = i / b.kp;
      const int r = (int)(rr % 16), t = (int)(rr / 16);
      const int col = t * TC + (r & 7);
      float v = 0.f;
      if (col < b.dout && k < b.din) v = (r < 8 ? b.wl : b.ws)[(long)col * b.din + k];
      b.w[i] = v;
    }
    if (i < (long)ntn * 16) {
      const int r = (int)(i % 16), t = (int)(i / 16);
      const int col = t * TC + (r & 7);
      b.bls[i] = col < b.dout ? (r < 8 ? b.bl : b.bs)[col] : 0.f;
    }
  } else if (blockIdx.z == 1) {
    const long n = (long)b.dout * 2 * b.dout;
    if (i < n) {
      const int k = (int)(i / (2 * b.dout)), c = (int)(i % (2 * b.dout));
      b.wgb[i] = c < b.dout ? b.wg[(long)c * b.dout + k] : b.wb[(long)(c - b.dout) * b.dout + k];
    }
    if (i < 2 * b.dout) b.bg2[i] = i < b.dout ? b.bg[i] : 0.f;
  } else {
    const int kc = pa.ntemb + pa.nxemb;
    const long n = (long)kc * b.dout;
    if (i < n) {
      const int k = (int)(i / b.dout), c = (int)(i % b.dout);
      const float v = b.wctx[(long)c * kc + k];
      if (k < pa.ntemb) pa.wctx_t[(long)k * pa.S + b.coloff + c] = v;
      else pa.wctx_x[(long)(k - pa.ntemb) * pa.S + b.coloff + c] = v;
    }
    if (i < b.dout) pa.bctx[b.coloff + i] = b.bctx[i];
  }
}

// (rows, cols) -> (cols, rows)
__global__ void transpose_kernel(const float* in, int rows, int cols, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * cols) return;
  const long r = i / cols, c = i - r * cols;
  out[c * rows + r] = in[i];
}

// ---- the hyper GEMMs on the limb product (round 5): per block j, [gate | hyper bias] = [sigmoid(c Wg^T + bg) | c Wb^T]
// over all n * B (step, row) pairs, K = dout <= 512: one limb-engine sign block, so no sign alternation.  The weights
// are read as the PyTorch Linear rows themselves ([dout][dout], k contiguous; row n < dout of the [2 dout][dout] operand
// is Wg's, the rest Wb's) and split into limbs on their way into LDS, with c's rows; one workgroup = 128 rows x 64
// columns, 8 waves of 32 x 32, the limb engine's six-MFMA product (enc_head.hip enc_head_x3_kernel has the same tile).
// The 7 blocks in one launch (tile table); the epilogue adds bg and applies the gate's sigmoid as gemm.hip's EPI_GATE.
typedef __bf16 hy8 __attribute__((ext_vector_type(8)));
typedef __bf16 hy4 __attribute__((ext_vector_type(4)));
constexpr int HY_BM = 128, HY_BN = 64, HY_KT = 32, HY_THREADS = 512, HY_ROWS = HY_BM + HY_BN, HY_NTMAX = 16;
constexpr size_t HY_LDS = 2 * 3 * HY_ROWS * 4 * sizeof(hy8);

struct HyperBlock {
  const float *a, *wg, *wb, *bg;
  float* c;
  long lda, ldc;
  int M, dout, ntn, tile0;
};
struct HyperGroup {
  HyperBlock b[7];
  int n, tiles;
  int exact_sig;  // 1: the gate's sigmoid as 1 / (1 + expf(-v)) with IEEE division (DAMC_SWEEP_HYPER_SIGMOID=exact)
};

__device__ __forceinline__ int hy_slot(int row, int q) {  // (enc_head.hip hd_slot: conflict-free fragment reads)
  return row * 4 + (q ^ ((0x1320 >> (4 * ((row >> 2) & 3))) & 3));
}
template <int N>
__device__ __forceinline__ void hy_split(const float* x, __bf16 (&h)[N], __bf16 (&m)[N], __bf16 (&l)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const __bf16 b0 = (__bf16)x[e];
    const float r1 = sub_rn(x[e], (float)b0);
    const __bf16 b1 = (__bf16)r1;
    h[e] = b0;
    m[e] = b1;
    l[e] = (__bf16)sub_rn(r1, (float)b1);
  }
}

template <int PD>
__global__ __launch_bounds__(HY_THREADS) void hyper_x3_kernel(HyperGroup g) {
  extern __shared__ __attribute__((aligned(16))) hy8 hyl[];  // [2 K tiles][3 limbs][HY_ROWS][4 slots]
  int j = 0;
  while (j + 1 < g.n && (int)blockIdx.x >= g.b[j + 1].tile0) ++j;
  const HyperBlock& hb = g.b[j];
  const int u = blockIdx.x - hb.tile0, m0 = (u / hb.ntn) * HY_BM, n0 = (u % hb.ntn) * HY_BN;
  const int K = hb.dout, nt = K / HY_KT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // staging: A row fr octet fq (rows past M load row M - 1 again, never stored); B row br (of the [2 dout][dout]
  // operand) half octet bh -- every thread the same loads, no branch
  const int fr = tid >> 2, fq = tid & 3, br = tid >> 3, bh = tid & 7;
  const float* ap = hb.a + (long)min(m0 + fr, hb.M - 1) * hb.lda + 8 * fq;
  const int nrow = n0 + br;
  const float* bp = (nrow < hb.dout ? hb.wg + (long)nrow * K : hb.wb + (long)(nrow - hb.dout) * K) + 4 * bh;
  f32x4 pa[PD][2], pb[PD];
  auto gload = [&](int t, int st) {
    pa[st][0] = *reinterpret_cast<const f32x4*>(ap + t * HY_KT);
    pa[st][1] = *reinterpret_cast<const f32x4*>(ap + t * HY_KT + 4);
    pb[st] = *reinterpret_cast<const f32x4*>(bp + t * HY_KT);
  };
  auto lstore = [&](int buf, int st) {
    hy8* p = hyl + buf * 3 * HY_ROWS * 4;
    const float va[8] = {pa[st][0][0], pa[st][0][1], pa[st][0][2], pa[st][0][3],
                         pa[st][1][0], pa[st][1][1], pa[st][1][2], pa[st][1][3]};
    __bf16 h[8], m[8], l[8];
    hy_split<8>(va, h, m, l);
    const int s = hy_slot(fr, fq);
    p[s] = hy8{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
    p[HY_ROWS * 4 + s] = hy8{m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]};
    p[2 * HY_ROWS * 4 + s] = hy8{l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7]};
    const float vb[4] = {pb[st][0], pb[st][1], pb[st][2], pb[st][3]};
    __bf16 h4[4], m4[4], l4[4];
    hy_split<4>(vb, h4, m4, l4);
    hy4* p4 = reinterpret_cast<hy4*>(p);
    const int s4 = 2 * hy_slot(HY_BM + br, bh >> 1) + (bh & 1);
    p4[s4] = hy4{h4[0], h4[1], h4[2], h4[3]};
    p4[2 * HY_ROWS * 4 + s4] = hy4{m4[0], m4[1], m4[2], m4[3]};
    p4[4 * HY_ROWS * 4 + s4] = hy4{l4[0], l4[1], l4[2], l4[3]};
  };
  const int wr = wave & 3, wc = wave >> 2, m = lane & 15, q = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < PD; ++st)
    if (st < nt) gload(st, st);
  lstore(0, 0);
  __syncthreads();
#pragma unroll
  for (int t = 0; t < HY_NTMAX; ++t) {
    if (t >= nt) break;  // (workgroup-uniform)
    if (t + PD < nt) gload(t + PD, t % PD);
    const hy8* p = hyl + (t & 1) * 3 * HY_ROWS * 4;
    hy8 fa[2][3], fb[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        fa[i][l] = p[l * HY_ROWS * 4 + hy_slot(32 * wr + 16 * i + m, q)];
        fb[i][l] = p[l * HY_ROWS * 4 + hy_slot(HY_BM + 32 * wc + 16 * i + m, q)];
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        f32x4 c = acc[i][jj];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][2], fb[jj][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[jj][1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[jj][2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[jj][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[jj][1], c, 0, 0, 0);
        acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[jj][0], c, 0, 0, 0);
      }
    if (t + 1 < nt) lstore((t + 1) & 1, (t + 1) % PD);
    __syncthreads();
  }
  // epilogue through LDS (free after the loop's last barrier): the tile's rows leave as 256-B runs of 16-B stores
  // instead of 64-B runs of 4-B stores (144 MB of gate / hyper-bias output per CIFAR sweep)
  constexpr int LD = HY_BN + 4;
  float* ot = reinterpret_cast<float*>(hyl);  // [HY_BM][LD]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 32 * wr + 16 * i + 4 * q + r, lc = 32 * wc + 16 * jj + m, col = n0 + lc;
        float v = acc[i][jj][r];
        if (col < hb.dout) {  // the gate: sigmoid(v + bg)
          if (hb.bg) v += hb.bg[col];
          // exp2 and reciprocal on the transcendental unit (~1 ulp each, both saturate to 0 / 1 correctly): 16 M
          // sigmoids per CIFAR sweep, where expf plus the IEEE division took a sixth of this kernel
          v = g.exact_sig ? 1.f / (1.f + expf(-v))
                          : __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-v * 1.4426950408889634f));
        }
        ot[lr * LD + lc] = v;
      }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < HY_BM * HY_BN / 4 / HY_THREADS; ++k) {
    const int f = tid + k * HY_THREADS, lr = f / (HY_BN / 4), c4 = f % (HY_BN / 4), row = m0 + lr;
    if (row < hb.M)
      *reinterpret_cast<f32x4*>(hb.c + (long)row * hb.ldc + n0 + 4 * c4) =
          *reinterpret_cast<const f32x4*>(ot + lr * LD + 4 * c4);
  }
}

}  // namespace

namespace damc {

// the ctx launch of a sweep: ctx4_kernel where the rows allow float4 access
int launch_ctx(const float* px, long pxstep, const float* qt, int n, int B, int S, float* cx, hipStream_t s) {
  const char* hs = getenv("DAMC_SWEEP_HYPER_SIGMOID");  // (read per call)
  const int exact = hs && strcmp(hs, "exact") == 0;
  const long BS = (long)B * S;
  if (S % 4 == 0 && pxstep % 4 == 0 && BS < (1L << 31) && (uintptr_t)px % 16 == 0 && (uintptr_t)qt % 16 == 0 && (uintptr_t)cx % 16 == 0) {
    hipLaunchKernelGGL(ctx4_kernel, dim3((unsigned)((BS / 4 + 255) / 256), (unsigned)n), dim3(256), 0, s, px, pxstep,
                       qt, (int)BS, S, exact, cx);
  } else {
    const long tot = (long)n * BS;
    hipLaunchKernelGGL(ctx_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, px, pxstep, qt, B, S,
                       tot, cx);
  }
  return (int)hipGetLastError();
}

// the shape predicates the stages and the dispatch branch on; damc_sweep_stages / damc_sweep_form report the same calls
bool stages_skinny(const damc_denoiser_t* d) {
  bool skinny = (d->ntemb & 15) == 0 && (d->nxemb & 3) == 0;
  for (int j = 0; j < (narrow_out2(d) ? 6 : 7); ++j) skinny = skinny && (d->blocks[j].dout & 15) == 0;
  return skinny;
}

// blocks whose hyper GEMM runs on hyper_x3_kernel (bit j), by shape: the stage's one grouped launch takes blocks
// 0 .. nb - 1 together, so every one of them has to fit it (K = dout in whole 32-deep tiles, at most HY_NTMAX of
// them), or the stage runs on the fp32 engine whole
int hyper_limb_blocks(const damc_denoiser_t* d, int nb, const int* coloff) {
  for (int j = 0; j < nb; ++j) {
    const int dout = d->blocks[j].dout;
    if (!(dout % 32 == 0 && dout <= HY_NTMAX * HY_KT && coloff[j] % 4 == 0)) return 0;
  }
  return (1 << nb) - 1;
}

void stages_init(Stages& st, const damc_denoiser_t* d, int B, int n, void* wsp, hipStream_t s) {
  st.d = d;
  carve(d, B, n, reinterpret_cast<char*>(wsp), &st.w);
  st.s = s;
  st.S = sum_dout(d);
  st.nt = d->ntemb;
  st.nx = d->nxemb;
  for (int j = 0, o = 0; j < 7; ++j) {
    st.coloff[j] = o;
    o += lay_dout(d->blocks[j].dout);
  }
  st.narrow = narrow_out2(d);
  st.nb = st.narrow ? 6 : 7;
  st.skinny = stages_skinny(d);
}

// ---- 1. pack the live weights
int stage_pack(const Stages& st) {
  const damc_denoiser_t* d = st.d;
  const SweepWs& w = st.w;
  hipStream_t s = st.s;
  const int nt = st.nt, nx = st.nx;
  PackArgs pa;
  long maxn = 0;
  for (int j = 0; j < 7; ++j) {
    const damc_csq_block_t& b = d->blocks[j];
    PackBlock& p = pa.b[j];
    p.wl = b.wl;
    p.bl = b.bl;
    p.ws = b.ws;
    p.bs = b.bs;
    p.wg = b.wg;
    p.bg = b.bg;
    p.wb = b.wb;
    p.wctx = d->wctx[j];
    p.bctx = d->bctx[j];
    p.din = b.din;
    p.dout = b.dout;
    p.kp = kpad(b.din);
    p.coloff = st.coloff[j];
    p.w = w.w[j];
    p.bls = w.bls[j];
    p.wgb = w.wgb[j];
    p.bg2 = w.bg2[j];
    const long ntn = (b.dout + TC - 1) / TC;
    maxn = std::max({maxn, ntn * 16 * p.kp, 2L * b.dout * b.dout, (long)(nt + nx) * b.dout});
  }
  pa.ntemb = nt;
  pa.nxemb = nx;
  pa.S = st.S;
  pa.wctx_t = w.wctx_t;
  pa.wctx_x = w.wctx_x;
  pa.bctx = w.bctx;
  hipLaunchKernelGGL(pack_denoiser_kernel, dim3((unsigned)((maxn + 255) / 256), 7, st.skinny ? 2 : 3), dim3(256), 0, s,
                     pa);
  const long ntt = (long)nt * nt;
  if (!st.skinny) {
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((ntt + 255) / 256)), dim3(256), 0, s, d->tw1, nt, nt, w.tw1t);
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((ntt + 255) / 256)), dim3(256), 0, s, d->tw2, nt, nt, w.tw2t);
  }
  const long nbm = (long)d->nz * (d->nz / 2);
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((nbm + 255) / 256)), dim3(256), 0, s, d->bmat, d->nz, d->nz / 2,
                     w.bmat);
  DAMC_LAUNCH_CHECK();
  return 0;
}

// ---- 2a. the time MLP (n rows) and its part of every block's ctx Linear: qt (n, S)
int stage_time(const Stages& st, const float* temb_in, int n) {
  const damc_denoiser_t* d = st.d;
  const SweepWs& w = st.w;
  hipStream_t s = st.s;
  const int nt = st.nt, nx = st.nx, S = st.S, nb = st.nb;
  int rc;
  if (st.narrow && !st.skinny) return DAMC_ERR_UNSUPPORTED;  // (validate() has checked)
  if (st.skinny) {
    SkArgs g;
    memset(&g, 0, sizeof(g));
    g.M = n;
    g.N = nt;
    g.K = nt;
    g.A = temb_in;
    g.lda = nt;
    g.nseg = 1;
    g.seg[0] = SkSeg{d->tw1, d->tb1, nt, 0};
    g.silu_y = 1;
    g.Y = w.t1;
    g.ldy = nt;
    if ((rc = launch_skinny(g, "sweep_pre", s))) return rc;
    g.A = w.t1;
    g.seg[0] = SkSeg{d->tw2, d->tb2, nt, 0};
    g.Y = w.t2;  // the ctx Linear consumes SiLU(temb)
    if ((rc = launch_skinny(g, "sweep_pre", s))) return rc;
    g.A = w.t2;
    g.N = st.narrow ? st.coloff[6] : S;
    g.nseg = nb;
    for (int j = 0; j < nb; ++j) g.seg[j] = SkSeg{d->wctx[j], d->bctx[j], (long)nt + nx, st.coloff[j]};
    g.silu_y = 0;
    g.Y = w.qt;
    g.ldy = S;
    if ((rc = launch_skinny(g, "sweep_pre", s))) return rc;
    if (st.narrow) {  // out2's columns of qt (its padding columns zero)
      const int d6 = d->blocks[6].dout, p6 = lay_dout(d6);
      if ((rc = damc::launch_narrow_linear(w.t2, nt, n, nt, 0, d->wctx[6], (long)nt + nx, d->bctx[6], d6, p6,
                                           w.qt + st.coloff[6], S, s)))
        return rc;
    }
    return 0;
  }
  damc::GemmArgs g;
  g.M = n;
  g.N = nt;
  g.K = nt;
  g.k_per_z = nt;
  g.A = temb_in;
  g.lda = nt;
  g.B = w.tw1t;
  g.ldb = nt;
  g.C = w.t1;
  g.ldc = nt;
  g.bias = d->tb1;
  g.bias_mod = nt;
  g.act = DAMC_ACT_SILU;
  if ((rc = damc::launch_gemm(g, damc::A_DENSE, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "sweep_pre", 2.0 * n * nt * nt, s)))
    return rc;
  g.A = w.t1;
  g.B = w.tw2t;
  g.C = w.t2;
  g.bias = d->tb2;
  g.act = DAMC_ACT_SILU;  // the ctx Linear consumes SiLU(temb)
  if ((rc = damc::launch_gemm(g, damc::A_DENSE, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "sweep_pre", 2.0 * n * nt * nt, s)))
    return rc;
  g.A = w.t2;
  g.B = w.wctx_t;
  g.ldb = S;
  g.N = S;
  g.C = w.qt;
  g.ldc = S;
  g.bias = w.bctx;
  g.bias_mod = S;
  g.act = DAMC_ACT_NONE;
  return damc::launch_gemm(g, damc::A_DENSE, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "sweep_pre", 2.0 * n * nt * S, s);
}

// ---- 2b. the xemb part of every block's ctx Linear: px (M, S) = SiLU(xemb) Wx^T of M embedding rows (xs: M x nxemb
// of scratch where the skinny GEMM does not apply)
int stage_px(const Stages& st, const float* xemb, int M, float* xs, float* px) {
  const damc_denoiser_t* d = st.d;
  const SweepWs& w = st.w;
  hipStream_t s = st.s;
  const int nt = st.nt, nx = st.nx, S = st.S, nb = st.nb;
  int rc;
  if (st.skinny) {
    SkArgs g;
    memset(&g, 0, sizeof(g));
    g.A = xemb;
    g.lda = nx;
    g.M = M;
    g.K = nx;
    g.N = st.narrow ? st.coloff[6] : S;
    g.nseg = nb;
    for (int j = 0; j < nb; ++j) g.seg[j] = SkSeg{d->wctx[j] + nt, nullptr, (long)nt + nx, st.coloff[j]};
    g.silu_a = 1;
    g.Y = px;
    g.ldy = S;
    if ((rc = launch_skinny(g, "sweep_pre", s))) return rc;
    if (st.narrow) {  // out2's columns of px (its padding columns zero)
      const int d6 = d->blocks[6].dout, p6 = lay_dout(d6);
      if ((rc = damc::launch_narrow_linear(xemb, nx, M, nx, 1, d->wctx[6] + nt, (long)nt + nx, nullptr, d6, p6,
                                           px + st.coloff[6], S, s)))
        return rc;
    }
    return 0;
  }
  const long nxe = (long)M * nx;
  hipLaunchKernelGGL(silu_kernel, dim3((unsigned)((nxe + 255) / 256)), dim3(256), 0, s, xemb, nxe, xs);
  damc::GemmArgs h;
  h.M = M;
  h.N = S;
  h.K = nx;
  h.k_per_z = nx;
  h.A = xs;
  h.lda = nx;
  h.B = w.wctx_x;
  h.ldb = S;
  h.C = px;
  h.ldc = S;
  return damc::launch_gemm(h, damc::A_DENSE, damc::EPI_STORE, damc::O_DENSE, 1, "sweep_pre", 2.0 * M * nx * S, s);
}

// ---- 3. every block's gate and hyper bias for M (step, row) pairs: gh (M, 2S) = [sigmoid(c Wg^T + bg) | c Wb^T] of
// cx (M, S).  Every engine below computes a row by itself, whatever M it runs with.
int stage_hyper(const Stages& st, const float* cx, float* gh, long M) {
  const damc_denoiser_t* d = st.d;
  const SweepWs& w = st.w;
  hipStream_t s = st.s;
  const int S = st.S, nb = st.nb;
  const int* coloff = st.coloff;
  int rc;
  damc::GemmArgs hg[7];
  double hflops = 0.0;
  for (int j = 0; j < nb; ++j) {
    const int dout = d->blocks[j].dout;
    damc::GemmArgs& g = hg[j];
    g.M = (int)M;
    g.N = 2 * dout;
    g.K = dout;
    g.k_per_z = dout;
    g.A = cx + coloff[j];
    g.lda = S;
    g.B = w.wgb[j];
    g.ldb = 2 * dout;
    g.C = gh + 2 * coloff[j];
    g.ldc = 2L * S;
    g.bias = w.bg2[j];
    g.bias_mod = 2 * dout;
    g.gate_cols = dout;
    hflops += 2.0 * M * dout * 2.0 * dout;
  }
  // round 5: on the limb product (hyper_x3_kernel) where every block fits it; DAMC_SWEEP_HYPER=fp32 (read per call)
  // keeps the fp32-MFMA engine below
  const char* hye = getenv("DAMC_SWEEP_HYPER");
  bool hy_ok = !(hye && strcmp(hye, "fp32") == 0) && (S % 4 == 0) && ((uintptr_t)cx % 16 == 0) &&
               ((uintptr_t)gh % 16 == 0) && hyper_limb_blocks(d, nb, coloff) != 0;
  HyperGroup hgp{};
  hgp.n = nb;
  {
    const char* hs = getenv("DAMC_SWEEP_HYPER_SIGMOID");  // (read per call) exact: IEEE expf and division
    hgp.exact_sig = hs && strcmp(hs, "exact") == 0;
  }
  for (int j = 0; j < nb && hy_ok; ++j) {
    const damc_csq_block_t& bk = d->blocks[j];
    const int dout = bk.dout;
    hy_ok = bk.wg && bk.wb && (uintptr_t)bk.wg % 16 == 0 && (uintptr_t)bk.wb % 16 == 0;
    HyperBlock& h = hgp.b[j];
    h.a = cx + coloff[j];
    h.lda = S;
    h.wg = bk.wg;
    h.wb = bk.wb;
    h.bg = bk.bg;
    h.c = gh + 2 * coloff[j];
    h.ldc = 2L * S;
    h.M = (int)M;
    h.dout = dout;
    h.ntn = 2 * dout / HY_BN;
    h.tile0 = hgp.tiles;
    hgp.tiles += ((h.M + HY_BM - 1) / HY_BM) * h.ntn;
  }
  if (hy_ok) {
    static const bool lds_ok = [] {
      return hipFuncSetAttribute((const void*)hyper_x3_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)HY_LDS) == hipSuccess;
    }();
    hy_ok = lds_ok;
  }
  // one grouped launch (its tiles fill the chip; seven launches of 200-400 tiles each left half of it idle in their
  // last round); the general path when a block's rows are not float4-aligned
  // DAMC_SWEEP_HYPER_GROUP=0 (read per call): seven launches (tests/test_gpu_amortizer.py checks both are bitwise equal)
  const char* hge = getenv("DAMC_SWEEP_HYPER_GROUP");
  if (hy_ok) {
    ProfScope ps("sweep_hyper", hflops, s);
    hipLaunchKernelGGL(hyper_x3_kernel<4>, dim3(hgp.tiles), dim3(HY_THREADS), HY_LDS, s, hgp);
    rc = (int)hipGetLastError();
  } else {
    rc = (hge && atoi(hge) == 0) ? DAMC_ERR_UNSUPPORTED
                                 : damc::launch_gemm_group(hg, nb, damc::EPI_GATE, "sweep_hyper", hflops, s);
  }
  if (rc == DAMC_ERR_UNSUPPORTED) {
    for (int j = 0; j < nb; ++j) {
      const int dout = d->blocks[j].dout;
      if ((rc = damc::launch_gemm(hg[j], damc::A_DENSE, damc::EPI_GATE, damc::O_DENSE, 1, "sweep_hyper",
                                  2.0 * M * dout * 2.0 * dout, s)))
        return rc;
    }
  } else if (rc) {
    return rc;
  }
  if (st.narrow) {  // out2's gate and hyper bias (K = N = nz), with the exact sigmoid
    const damc_csq_block_t& bk = d->blocks[6];
    if ((rc = damc::launch_narrow_hyper(cx + coloff[6], S, M, bk.dout, bk.wg, bk.bg, bk.wb, gh + 2 * coloff[6], 2L * S,
                                        s)))
      return rc;
  }
  return 0;
}

}  // namespace damc
