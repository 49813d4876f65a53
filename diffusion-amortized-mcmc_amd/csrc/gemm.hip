// gemm.hip — fp32 MFMA implicit-GEMM engine for the generator / encoder convolutions.
//
// Block tile (64*MT) x 128 x BK, 256 threads = 4 waves in a 2x2 grid; a wave owns (32*MT) x 64 =
// MT x 2 tiles of v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain per output; gfx950
// has no xf32).  Operands are staged global -> registers -> LDS (k-major images: every MFMA operand
// read is one conflict-free ds_read_b32 of 32 consecutive floats per half-wave), double-buffered
// with one barrier per K-tile.  Schedule per tile: all fragments of the tile -> registers, store the
// next tile into the other LDS buffer, issue the global loads of the tile after that, then the
// tile's MFMAs back to back (the loads land under them).  Gather addresses are 32-bit element
// offsets off the tensor base (every tensor here has < 2^31 elements).  Blocks are remapped so each
// XCD owns a contiguous run of tiles (shared A rows stay in its L2).
//
// Config (BK, OCC, MT): K-tile depth, workgroups per CU for the launch bounds, MFMA tiles per wave
// along M.  tools/gemm_bench.hip A/B-tests them on the generator's convolutions.
//
// This file: the generic engine, the small and grouped fp32 GEMMs, and launch_gemm / launch_gemm_group, which
// dispatch to the three engines.  The other engines behind gemm.h:
//   gemm_km.hip   the K-major convolution engine (gemm_km_kernel, km_skinny_kernel, launch_gemm_km)
//   gemm_x3.hip   the bf16 limb ("x3") engine: gemm_x3_kernel and its variants (X3_F32A, X3_TAPSHARE, ...), the
//                 split-K plan and reduces (x3_ksplit), x3_skinny_kernel, the output-layer projection (PROJ_CHUNK,
//                 launch_proj_rows), launch_gemm_x3, launch_wgrad_x3, the clock probe
//   x3_pack.hip   the limb split and weight-pack kernels (launch_split_x3*, launch_pack_*)
//   gemm_impl.h   what they share (epilogue helpers, rasters, the limb engine's constants, split3_octet)
#include "gemm_impl.h"

namespace damc {

template <int BK, int MT>
struct TileCfg {
  static constexpr int BM = 64 * MT;
  // A is written transposed with ds_write_b32: lanes (a_kq, m) of a half-wave must hit 32 banks
  static constexpr int LDA = (BK == 16) ? BM + 2 : BM + 1;
  static constexpr int LDB = BN;
  static constexpr int AQ = BK / 4;              // float4 slots per A row
  static constexpr int AROWS_V = BM * BK / 1024; // A float4 loads per thread (vector path)
  static constexpr int AROWS_S = BM * BK / 256;  // A scalar loads per thread
  static constexpr int BROWS_V = BK / 8;         // B float4 loads per thread
  static constexpr int BROWS_S = BK / 2;         // B scalar loads per thread
};

// Not called.  hipcc inlines the always-inline helpers in the order the module first references them, and the four
// O_PHASE A_CONV(_SCALAR) instantiations of gemm_f32_kernel allocate their registers differently (two of them 1-2 VGPRs
// more) unless gemm_row_offset<O_PHASE> and then gemm_epilogue<EPI_BIAS_ACT, O_PHASE, 2> are referenced ahead of
// gemm_f32_tile, so that each is inlined into the next.  While gemm_km_kernel shared this translation unit, its
// row table and epilogue call gave that order; this function keeps it, so every kernel here is the code it was
// (profiles/r22/isa_identity.txt).  Drop it only with a measurement of those four kernels.
__device__ __attribute__((used)) void gemm_epilogue_order(const GemmArgs& p, f32x16 (&acc)[2][2]) {
  const long rowoff = gemm_row_offset<O_PHASE>(p, 0, 0, 0);
  gemm_epilogue<EPI_BIAS_ACT, O_PHASE, 2>(p, acc, 0, 0, 0, 0, 0, 0, 0, 0, &rowoff);
}

// one block tile of the generic engine: tile wgid (already XCD-remapped) of the (M, N) grid, z = blockIdx.z
template <int AM, int EPI, int OM, bool BVEC, int BK, int MT, int SCHED>
__device__ __forceinline__ void gemm_f32_tile(const GemmArgs& p, const int wgid, const int z) {
  typedef TileCfg<BK, MT> C;
  constexpr int BM = C::BM;
  __shared__ float As[2][BK * C::LDA];
  __shared__ float Bs[2][BK * C::LDB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  const int ntn = (p.N + BN - 1) / BN;
  const int tm = wgid / ntn, tn = wgid - tm * ntn;
  const int m0 = tm * BM, n0 = tn * BN;

  int pad_y = p.pad_y, pad_x = p.pad_x;
  const float* Bg = p.B;
  int kbeg = 0, kend = p.K;
  int py = 0, px = 0;
  if (OM == O_PHASE) {
    py = z >> 1;
    px = z & 1;
    pad_y = 1 - py;
    pad_x = 1 - px;
    Bg += (long)z * p.b_zstride;
  } else {
    kbeg = z * p.k_per_z;
    kend = min(p.K, kbeg + p.k_per_z);
  }
  const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;

  // ---- per-thread A rows
  const int a_kq = tid % C::AQ;  // float4 slot within the k tile (vector paths)
  const int a_ml = tid / C::AQ;  // rows a_ml + AVSTEP*j
  constexpr int AVSTEP = 256 / C::AQ;
  const int s_kk = tid % BK;     // scalar path k
  const int s_ml = tid / BK;     // rows s_ml + ASSTEP*j
  constexpr int ASSTEP = 256 / BK;
  constexpr int AROWS = (AM == A_CONV_SCALAR) ? C::AROWS_S : C::AROWS_V;
  int a_pix[AROWS], a_iy[AROWS], a_ix[AROWS];  // first pixel of the sample / top-left input tap
  const int hwq = p.Hq * p.Wq;
  const int hwin = p.Hin * p.Win;
#pragma unroll
  for (int j = 0; j < AROWS; ++j) {
    const int m = m0 + ((AM == A_CONV_SCALAR) ? (s_ml + ASSTEP * j) : (a_ml + AVSTEP * j));
    const bool ok = m < p.M;
    if (AM == A_DENSE) {
      a_pix[j] = m * (int)p.lda;
      a_iy[j] = ok ? 0 : -0x40000000;  // poisons the row bound check
      a_ix[j] = 0;
    } else {
      const int mm = ok ? m : 0;
      const int b = mm / hwq;
      const int r = mm - b * hwq;
      const int qy = r / p.Wq, qx = r - qy * p.Wq;
      a_pix[j] = b * hwin;
      a_iy[j] = ok ? qy * p.stride - pad_y : -0x40000000;
      a_ix[j] = qx * p.stride - pad_x;
    }
  }
  // when Cg is a multiple of BK a whole K-tile sits inside one filter tap: the tap decomposition
  // is then tile-uniform (scalar) instead of a per-lane division
  const bool tap_uniform = (AM == A_CONV) && (p.Cg % BK == 0);
  const unsigned Hin = (unsigned)p.Hin, Win = (unsigned)p.Win;

  f32x4 ra[C::AROWS_V];
  float rs[C::AROWS_S];
  f32x4 rb[C::BROWS_V];
  float rbs[C::BROWS_S];

  auto load_a = [&](int k0) {
    if (AM == A_CONV_SCALAR) {
      const int k = k0 + s_kk;
      int ky = 0, kx = 0, ci = 0;
      const bool kin = k < kend;
      if (kin) {
        const int tap = k / p.Cg;
        ci = k - tap * p.Cg;
        ky = tap / p.kw;
        kx = tap - ky * p.kw;
      }
#pragma unroll
      for (int j = 0; j < C::AROWS_S; ++j) {
        const int iy = a_iy[j] + ky, ix = a_ix[j] + kx;
        const bool ok = kin && (unsigned)iy < Hin && (unsigned)ix < Win;
        rs[j] = ok ? p.A[(a_pix[j] + iy * p.Win + ix) * p.Cg + ci] : 0.f;
      }
    } else {
      const int k = k0 + 4 * a_kq;
      const bool kin = k < kend;
      if (AM == A_DENSE) {
#pragma unroll
        for (int j = 0; j < C::AROWS_V; ++j) {
          ra[j] = (kin && a_iy[j] == 0) ? *reinterpret_cast<const f32x4*>(p.A + (a_pix[j] + k))
                                        : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      } else {
        int ky = 0, kx = 0, ci = 0;
        if (tap_uniform) {
          const int tap = k0 / p.Cg;
          ci = k0 - tap * p.Cg + 4 * a_kq;
          ky = tap / p.kw;
          kx = tap - ky * p.kw;
        } else if (kin) {
          const int tap = k / p.Cg;
          ci = k - tap * p.Cg;
          ky = tap / p.kw;
          kx = tap - ky * p.kw;
        }
#pragma unroll
        for (int j = 0; j < C::AROWS_V; ++j) {
          const int iy = a_iy[j] + ky, ix = a_ix[j] + kx;
          const bool ok = kin && (unsigned)iy < Hin && (unsigned)ix < Win;
          ra[j] = ok ? *reinterpret_cast<const f32x4*>(p.A + ((a_pix[j] + iy * p.Win + ix) * p.Cg + ci))
                     : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  };
  auto store_a = [&](int buf) {
    float* as = As[buf];
    if (AM == A_CONV_SCALAR) {
#pragma unroll
      for (int j = 0; j < C::AROWS_S; ++j) as[s_kk * C::LDA + s_ml + ASSTEP * j] = rs[j];
    } else {
#pragma unroll
      for (int j = 0; j < C::AROWS_V; ++j) {
        const int ml = a_ml + AVSTEP * j;
        as[(4 * a_kq + 0) * C::LDA + ml] = ra[j].x;
        as[(4 * a_kq + 1) * C::LDA + ml] = ra[j].y;
        as[(4 * a_kq + 2) * C::LDA + ml] = ra[j].z;
        as[(4 * a_kq + 3) * C::LDA + ml] = ra[j].w;
      }
    }
  };
  // B tile: BK k-rows x 128 n
  const int b_row = tid >> 5, b_c4 = tid & 31;    // vector path: 8 rows per pass
  const int bs_n = tid & 127, bs_row = tid >> 7;  // scalar path: 2 rows per pass
  const int ldb = (int)p.ldb;
  auto load_b = [&](int k0) {
    if (BVEC) {
      const int n = n0 + 4 * b_c4;
#pragma unroll
      for (int j = 0; j < C::BROWS_V; ++j) {
        const int k = k0 + b_row + 8 * j;
        rb[j] = (k < kend && n < p.N) ? *reinterpret_cast<const f32x4*>(Bg + (k * ldb + n))
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
      const int n = n0 + bs_n;
#pragma unroll
      for (int j = 0; j < C::BROWS_S; ++j) {
        const int k = k0 + bs_row + 2 * j;
        rbs[j] = (k < kend && n < p.N) ? Bg[k * ldb + n] : 0.f;
      }
    }
  };
  auto store_b = [&](int buf) {
    float* bs = Bs[buf];
    if (BVEC) {
#pragma unroll
      for (int j = 0; j < C::BROWS_V; ++j)
        *reinterpret_cast<f32x4*>(bs + (b_row + 8 * j) * C::LDB + 4 * b_c4) = rb[j];
    } else {
#pragma unroll
      for (int j = 0; j < C::BROWS_S; ++j) bs[(bs_row + 2 * j) * C::LDB + bs_n] = rbs[j];
    }
  };

  f32x16 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    load_a(kbeg);
    load_b(kbeg);
    store_a(0);
    store_b(0);
    if (nk > 1) {
      load_a(kbeg + BK);
      load_b(kbeg + BK);
    }
  }
  __syncthreads();

  const int lrow = lane & 31, lk = lane >> 5;
  const int am0 = wm * (32 * MT) + lrow, bn0 = wn * 64 + lrow;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const float* as = As[cur];
    const float* bs = Bs[cur];
    float fa[BK / 2][MT], fb[BK / 2][2];
#pragma unroll
    for (int s2 = 0; s2 < BK / 2; ++s2) {
      const int kk = 2 * s2 + lk;
#pragma unroll
      for (int i = 0; i < MT; ++i) fa[s2][i] = as[kk * C::LDA + am0 + 32 * i];
      fb[s2][0] = bs[kk * C::LDB + bn0];
      fb[s2][1] = bs[kk * C::LDB + bn0 + 32];
    }
    auto mfma_steps = [&](int s_lo, int s_hi) {
#pragma unroll
      for (int s2 = 0; s2 < BK / 2; ++s2) {
        if (s2 < s_lo || s2 >= s_hi) continue;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s2][i], fb[s2][0], acc[i][0], 0, 0, 0);
          acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s2][i], fb[s2][1], acc[i][1], 0, 0, 0);
        }
      }
    };
    auto stage_next = [&]() {
      if (kt + 1 < nk) {
        store_a(cur ^ 1);
        store_b(cur ^ 1);
        if (kt + 2 < nk) {
          load_a(kbeg + (kt + 2) * BK);
          load_b(kbeg + (kt + 2) * BK);
        }
      }
    };
    if (SCHED == 0) {
      stage_next();
      mfma_steps(0, BK / 2);
    } else if (SCHED == 1) {
      // keep the MFMA block before the barrier (hipcc otherwise hoists the barrier and its
      // lgkmcnt(0) above the MFMAs, serialising the LDS writes in front of them)
      stage_next();
      mfma_steps(0, BK / 2);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      // first half of the MFMAs, then the LDS writes + next global loads, then the second half
      mfma_steps(0, BK / 4);
      __builtin_amdgcn_sched_barrier(0);
      stage_next();
      __builtin_amdgcn_sched_barrier(0);
      mfma_steps(BK / 4, BK / 2);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  }

  gemm_epilogue<EPI, OM, MT>(p, acc, m0, n0, wm, wn, lane, z, py, px);
}

template <int AM, int EPI, int OM, bool BVEC, int BK, int OCC, int MT, int SCHED>
__global__ __launch_bounds__(256, OCC) void gemm_f32_kernel(GemmArgs p) {
  // XCD-aware tile remap (bijective for any grid size)
  gemm_f32_tile<AM, EPI, OM, BVEC, BK, MT, SCHED>(p, xcd_remap(blockIdx.x, gridDim.x), blockIdx.z);
}

// independent GEMMs of one shape class in one launch: group g owns the remapped tile ids [start[g], start[g+1]), so
// the tiles of all of them share the chip instead of each launch's last partial round idling half of it
template <int AM, int EPI, int OM, bool BVEC, int BK, int OCC, int MT, int SCHED>
__global__ __launch_bounds__(256, OCC) void gemm_f32_group_kernel(GemmGroup g) {
  const int wgid = xcd_remap(blockIdx.x, gridDim.x);
  int j = 0;
#pragma unroll
  for (int t = 1; t < GEMM_GROUP_MAX; ++t) j += (t < g.n && wgid >= g.start[t]) ? 1 : 0;
  gemm_f32_tile<AM, EPI, OM, BVEC, BK, MT, SCHED>(g.a[j], wgid - g.start[j], 0);
}

// ================================================================================================
// Small fp32 GEMMs (the Q update's denoiser: B = 128-row activations times weights, and the weight gradients with
// K = B): C (M x N, ldc) = A (M x K row-major, lda) . B (K x N row-major, ldb) (+ bias[n]), exact fp32 products on
// v_mfma_f32_16x16x4f32 with fp32 accumulation.  One 16 x 16 output tile per wave, the whole K in one chain, operands
// straight from memory into registers (KU 16-k steps of loads in flight), so a 128 x 512 product is 256 waves in ONE
// launch -- the tiled engine gave it 4 workgroups, or split K into slabs plus a reduce launch.  Lane (m, q) supplies
// A[row m][k0 + 4 q + e] and B[k0 + 4 q + e][col m] to MFMA step e (proj16's k bijection).
template <int KU>
__global__ __launch_bounds__(256) void small_gemm_kernel(const float* __restrict__ A, long lda, const float* __restrict__ B,
                                                         long ldb, const float* __restrict__ bias, float* __restrict__ C,
                                                         long ldc, int M, int N, int K, int bias_mod, int act,
                                                         float slope) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntn = (N + 15) >> 4;
  const long tile = (long)blockIdx.x * 4 + wave;
  const int tm = (int)(tile / ntn), tn = (int)(tile - (long)tm * ntn);
  if (tm * 16 >= M) return;  // wave-uniform
  const int m = lane & 15, q = lane >> 4;
  const int row = tm * 16 + m, col = tn * 16 + m;
  const bool rok = row < M, cok = col < N;
  const float* Ar = A + (long)(rok ? row : 0) * lda;
  const float* Bc = B + (cok ? col : 0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 16 * KU) {
    f32x4 a[KU], b[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {  // K % 4 == 0: a lane's 4 k are all in range or all out; loads from clamped
      const int k = k0 + 16 * u + 4 * q;  // (valid) addresses, then zeroed, so no load sits in a branch
      const bool kin = k < K;
      const int kk = kin ? k : 0;
      a[u] = *reinterpret_cast<const f32x4*>(Ar + kk);
#pragma unroll
      for (int e = 0; e < 4; ++e) b[u][e] = Bc[(long)(kk + e) * ldb];
      if (!(rok && kin)) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (!(cok && kin)) b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __builtin_amdgcn_sched_barrier(0);  // the KU steps' loads all in flight before the first MFMA waits
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], b[u][e], acc, 0, 0, 0);
  }
  if (!cok) return;
  const float bv = bias ? bias[bias_mod > 0 ? col % bias_mod : col] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = tm * 16 + 4 * q + r;
    if (rr < M) C[(long)rr * ldc + col] = act_apply(acc[r] + bv, act, slope);
  }
}

int launch_small_gemm(const float* A, long lda, const float* B, long ldb, const float* bias, float* C, long ldc, int M,
                      int N, int K, hipStream_t s, int bias_mod, int act, float slope) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || lda < K || ldb < N || ldc < N) return DAMC_ERR_ARG;
  if (K % 4 != 0 || lda % 4 != 0 || (reinterpret_cast<uintptr_t>(A) & 15) != 0) return DAMC_ERR_UNSUPPORTED;  // f32x4 A
  ProfScope ps("small_gemm", 2.0 * M * N * K, s);
  const long tiles = (long)((M + 15) / 16) * ((N + 15) / 16);
  hipLaunchKernelGGL(small_gemm_kernel<4>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, A, lda, B, ldb, bias, C,
                     ldc, M, N, K, bias_mod, act, slope);
  return (int)hipGetLastError();
}

// Up to SG_GROUP_MAX independent small GEMMs (SmallGemm, gemm.h) in ONE launch, one 16 x 16 output tile per 4-wave
// workgroup with K split over the waves in four contiguous runs of 16-k steps (a quarter of the single-wave kernel's
// dependent load rounds), the wave partials summed in LDS in a fixed order ((w0 + w1) + w2) + w3.  a_ones: A is a row of
// ones (M = 1): C = the column sums of B, the bias gradients of the denoiser's Linears as one more member of the group.
template <int KU>
__global__ __launch_bounds__(256) void small_gemm_group_kernel(SmallGemmGroup g) {
  __shared__ f32x4 red[3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blk = blockIdx.x;
  int gi = 0;
  while (gi + 1 < g.n && blk >= g.tile_end[gi]) ++gi;  // workgroup-uniform
  const SmallGemm& D = g.d[gi];
  const int tile = blk - (gi ? g.tile_end[gi - 1] : 0);
  const int M = D.M, N = D.N, K = D.K;
  const int ntn = (N + 15) >> 4;
  const int tm = tile / ntn, tn = tile - tm * ntn;
  const int m = lane & 15, q = lane >> 4;
  const int row = tm * 16 + m, col = tn * 16 + m;
  const bool rok = row < M, cok = col < N;
  const float* Ar = D.A + (long)(rok && !D.a_ones ? row : 0) * D.lda;
  const long ldb = D.ldb;
  const float* Bc = D.b_t ? D.B + (long)(cok ? col : 0) * ldb : D.B + (cok ? col : 0);
  const int k16 = (K + 15) >> 4, per = (k16 + 3) >> 2;
  const int kb = wave * per * 16, ke = min(K, kb + per * 16);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += 16 * KU) {
    f32x4 a[KU], b[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {  // K % 4 == 0: a lane's 4 k are all in range or all out
      const int k = k0 + 16 * u + 4 * q;
      const bool kin = k < ke;
      const int kk = kin ? k : 0;
      a[u] = D.a_ones ? f32x4{1.f, 1.f, 1.f, 1.f} : *reinterpret_cast<const f32x4*>(Ar + kk);
      if (D.b_t) {
        b[u] = *reinterpret_cast<const f32x4*>(Bc + kk);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) b[u][e] = Bc[(long)(kk + e) * ldb];
      }
      if (!(rok && kin)) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (!(cok && kin)) b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], b[u][e], acc, 0, 0, 0);
  }
  if (wave) red[wave - 1][lane] = acc;
  __syncthreads();
  if (wave || !cok) return;
  acc = ((acc + red[0][lane]) + red[1][lane]) + red[2][lane];
  const float bv = D.bias ? D.bias[D.bias_mod > 0 ? col % D.bias_mod : col] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = tm * 16 + 4 * q + r;
    if (rr < M) D.C[(long)rr * D.ldc + col] = act_apply(acc[r] + bv, D.act, D.slope);
  }
}

int launch_small_gemm_group(const SmallGemm* g, int n, hipStream_t s) {
  if (n < 1 || n > SG_GROUP_MAX) return DAMC_ERR_ARG;
  SmallGemmGroup grp{};
  long tot = 0;
  double flops = 0.0;
  for (int i = 0; i < n; ++i) {
    const SmallGemm& d = g[i];
    if ((!d.A && !d.a_ones) || !d.B || !d.C || d.M <= 0 || d.N <= 0 || d.K <= 0 || d.ldb < (d.b_t ? d.K : d.N) ||
        d.ldc < d.N || (d.a_ones && d.M != 1) || (!d.a_ones && d.lda < d.K))
      return DAMC_ERR_ARG;
    if (d.K % 4 != 0 || (!d.a_ones && (d.lda % 4 != 0 || (reinterpret_cast<uintptr_t>(d.A) & 15) != 0)))
      return DAMC_ERR_UNSUPPORTED;  // f32x4 A
    if (d.b_t && (d.ldb % 4 != 0 || (reinterpret_cast<uintptr_t>(d.B) & 15) != 0)) return DAMC_ERR_UNSUPPORTED;
    grp.d[i] = d;
    tot += (long)((d.M + 15) / 16) * ((d.N + 15) / 16);
    if (tot >= (1L << 31)) return DAMC_ERR_UNSUPPORTED;
    grp.tile_end[i] = (int)tot;
    flops += 2.0 * d.M * d.N * d.K;
  }
  grp.n = n;
  ProfScope ps("small_gemm_group", flops, s);
  hipLaunchKernelGGL(small_gemm_group_kernel<4>, dim3((unsigned)tot), dim3(256), 0, s, grp);
  return (int)hipGetLastError();
}

#ifndef DAMC_GEMM_SCHED
#define DAMC_GEMM_SCHED 0  // hipcc's own placement measured best (profiles/r01/gemm_bench.txt)
#endif
template <int AM, int EPI, int OM, bool BV, int BK, int OCC, int MT, int SCHED = DAMC_GEMM_SCHED>
static void launch_t(const GemmArgs& a, int zdim, hipStream_t s) {
  const int bm = 64 * MT;
  const int ntm = (a.M + bm - 1) / bm, ntn = (a.N + BN - 1) / BN;
  dim3 grid(ntm * ntn, 1, zdim);
  hipLaunchKernelGGL((gemm_f32_kernel<AM, EPI, OM, BV, BK, OCC, MT, SCHED>), grid, dim3(256), 0, s, a);
}

// tile configuration used by the library (tools/gemm_bench.hip A/B-tests alternatives)
#ifndef DAMC_GEMM_BK
#define DAMC_GEMM_BK 32  // measured best on the B=128 generator convs (profiles/r01/gemm_bench.txt)
#endif
#ifndef DAMC_GEMM_OCC
#define DAMC_GEMM_OCC 2
#endif
#ifndef DAMC_GEMM_MT
#define DAMC_GEMM_MT 2
#endif

int launch_gemm_group(const GemmArgs* a, int n, Epi epi, const char* prof_name, double flops, hipStream_t s) {
  if (n < 1 || n > GEMM_GROUP_MAX) return DAMC_ERR_ARG;
  if (epi != EPI_GATE && epi != EPI_STORE) return DAMC_ERR_UNSUPPORTED;
  GemmGroup g;
  const int bm = 64 * DAMC_GEMM_MT;
  int tot = 0;
  for (int i = 0; i < n; ++i) {
    const GemmArgs& x = a[i];
    if (x.M <= 0 || x.N <= 0 || x.K <= 0 || x.A3 || x.b_kmajor || x.k_per_z < x.K) return DAMC_ERR_ARG;
    // the dense vector path only: float4 rows of A and B
    if (x.lda % 4 || x.K % 4 || x.ldb % 4 || x.N % 4 || ((uintptr_t)x.A | (uintptr_t)x.B) % 16) return DAMC_ERR_UNSUPPORTED;
    if ((double)x.M * x.lda >= 2147483647.0 || (double)x.K * x.ldb >= 2147483647.0) return DAMC_ERR_UNSUPPORTED;
    g.a[i] = x;
    g.start[i] = tot;
    tot += ((x.M + bm - 1) / bm) * ((x.N + BN - 1) / BN);
  }
  for (int i = n; i <= GEMM_GROUP_MAX; ++i) g.start[i] = tot;
  g.n = n;
  ProfScope ps(prof_name, flops, s);
  constexpr int BKc = DAMC_GEMM_BK, OCCc = DAMC_GEMM_OCC, MTc = DAMC_GEMM_MT;
  if (epi == EPI_GATE)
    hipLaunchKernelGGL((gemm_f32_group_kernel<A_DENSE, EPI_GATE, O_DENSE, true, BKc, OCCc, MTc, DAMC_GEMM_SCHED>),
                       dim3(tot), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((gemm_f32_group_kernel<A_DENSE, EPI_STORE, O_DENSE, true, BKc, OCCc, MTc, DAMC_GEMM_SCHED>),
                       dim3(tot), dim3(256), 0, s, g);
  return (int)hipGetLastError();
}

int launch_gemm(const GemmArgs& a, AMode am, Epi epi, OMode om, int zdim, const char* prof_name, double flops,
                hipStream_t s) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return DAMC_ERR_ARG;
  if (a.A3 || (a.a_f32 && a.B3)) {
    if (am != A_CONV) return DAMC_ERR_ARG;
    ProfScope ps(prof_name, flops, s);
    return launch_gemm_x3(a, epi, om, zdim, s);
  }
  if (a.b_kmajor) {
    if (am != A_CONV) return DAMC_ERR_ARG;
    ProfScope ps(prof_name, flops, s);
    return launch_gemm_km(a, epi, om, zdim, s);
  }
  // 32-bit element offsets inside the kernel
  const double a_elems = (am == A_DENSE) ? (double)a.M * a.lda : (double)a.Hin * a.Win * a.Cg * ((double)a.M / ((double)a.Hq * a.Wq) + 1);
  if (a_elems >= 2147483647.0 || (double)a.K * a.ldb >= 2147483647.0) return DAMC_ERR_UNSUPPORTED;
  const bool bvec = (a.ldb % 4 == 0) && (a.N % 4 == 0) && ((uintptr_t)a.B % 16 == 0);
  if (am == A_DENSE && (a.lda % 4 != 0 || a.K % 4 != 0 || (uintptr_t)a.A % 16 != 0)) am = A_CONV_SCALAR;
  if (am == A_CONV && (a.Cg % 4 != 0 || (uintptr_t)a.A % 16 != 0)) am = A_CONV_SCALAR;
  GemmArgs b = a;
  if (am == A_CONV_SCALAR && a.Hq == 1 && a.Wq == 1 && a.Hin == 1 && a.Win == 1 && a.kw == 1) {
    // dense-as-scalar: treat A (M,K) as an NHWC map with one pixel of Cg = lda channels
    b.Cg = (int)a.lda;
  }
  ProfScope ps(prof_name, flops, s);
  constexpr int BKc = DAMC_GEMM_BK, OCCc = DAMC_GEMM_OCC, MTc = DAMC_GEMM_MT;
#define DAMC_G(AM_, EPI_, OM_)                                                          \
  if (am == AM_ && epi == EPI_ && om == OM_) {                                          \
    if (bvec) launch_t<AM_, EPI_, OM_, true, BKc, OCCc, MTc>(b, zdim, s);               \
    else launch_t<AM_, EPI_, OM_, false, BKc, OCCc, MTc>(b, zdim, s);                   \
    return (int)hipGetLastError();                                                      \
  }
  DAMC_G(A_DENSE, EPI_STORE, O_DENSE)
  DAMC_G(A_DENSE, EPI_BIAS_ACT, O_DENSE)
  DAMC_G(A_DENSE, EPI_MASK, O_DENSE)
  DAMC_G(A_DENSE, EPI_RESID, O_DENSE)
  DAMC_G(A_DENSE, EPI_GATE, O_DENSE)
  DAMC_G(A_CONV, EPI_BIAS_ACT, O_PHASE)
  DAMC_G(A_CONV, EPI_MASK, O_DENSE)
  DAMC_G(A_CONV, EPI_BIAS_ACT, O_DENSE)
  DAMC_G(A_CONV, EPI_STORE, O_DENSE)
  DAMC_G(A_CONV_SCALAR, EPI_STORE, O_DENSE)
  DAMC_G(A_CONV_SCALAR, EPI_BIAS_ACT, O_DENSE)
  DAMC_G(A_CONV_SCALAR, EPI_MASK, O_DENSE)
  DAMC_G(A_CONV_SCALAR, EPI_RESID, O_DENSE)
  DAMC_G(A_CONV_SCALAR, EPI_BIAS_ACT, O_PHASE)
  DAMC_G(A_CONV_SCALAR, EPI_MASK, O_PHASE)
#undef DAMC_G
  return DAMC_ERR_UNSUPPORTED;
}

}  // namespace damc

#ifndef DAMC_GEMM_NO_C_API
extern "C" int damc_gemm(const float* a, int lda, const float* b, int ldb, const float* bias, float* c, int ldc,
                         int m, int n, int k, int act, float slope, void* stream) {
  if (!a || !b || !c || act < DAMC_ACT_NONE || act > DAMC_ACT_RELU) return DAMC_ERR_ARG;
  if (lda < k || ldb < n || ldc < n) return DAMC_ERR_ARG;
  if (act == DAMC_ACT_RELU) {  // the epilogue's act_apply has no ReLU of its own: LeakyReLU with slope 0
    act = DAMC_ACT_LRELU;
    slope = 0.f;
  }
  damc::GemmArgs g;
  g.A = a;
  g.lda = lda;
  g.B = b;
  g.ldb = ldb;
  g.C = c;
  g.ldc = ldc;
  g.M = m;
  g.N = n;
  g.K = k;
  g.k_per_z = k;
  g.bias = bias;
  g.bias_mod = n;
  g.act = act;
  g.slope = slope;
  return damc::launch_gemm(g, damc::A_DENSE, damc::EPI_BIAS_ACT, damc::O_DENSE, 1, "gemm", 2.0 * m * n * k,
                           as_stream(stream));
}
#endif
