// gemm_km.hip — K-major convolution engine (A_CONV with Cg % 32 == 0, B packed [n][k]); launch_gemm (gemm.hip)
// dispatches here for GemmArgs::b_kmajor.
//
// Both operands are staged k-contiguous: a global float4 (4 consecutive channels of one pixel, or 4
// consecutive k of one weight row) -> one ds_write_b128 -> the MFMA fragments come back as
// ds_read_b128 through a k-permutation (MFMA step s of k-quad q uses k = 8q + 4(lane>>5) + s, the same
// bijection on A and B, so every lane's 4 consecutive steps are one 16-B read).  Rows are padded to
// 36 floats: any 16 consecutive rows then cover all 64 banks, which makes both the b128 reads (16-lane
// groups of rows) and the b128 writes (8-lane groups along one row) conflict-free.
// Since a 32-wide K tile never straddles a filter tap, the tap walk is a scalar counter; each A row
// carries a bitmask of the taps that land inside the image (computed once), and every load is a
// buffer load whose offset is pushed out of the descriptor's range when the tap is padding, so the
// hardware returns zeros -- no per-load bounds arithmetic or exec-mask branches in the K loop.
#include <algorithm>
#include <cstdlib>

#include "gemm_impl.h"

namespace damc {

constexpr int KM_BM = 128;
constexpr int KM_RS = KM_BK + 4;

// PIPE 0: per tile {fragments of tile kt -> regs, stage tile kt+1, load tile kt+2, MFMAs, barrier}.
// PIPE 1: fragments register-prefetched one tile ahead; per tile {barrier, fragments of kt+1 -> regs,
//         stage tile kt+2, load tile kt+3, MFMAs of kt} so the MFMA operands are resident when the
//         barrier releases and the LDS traffic runs under the MFMAs.
#ifndef DAMC_KM_PIPE
#define DAMC_KM_PIPE 3
#endif
// DBG (timing experiments only, wrong results): 1 = every row loads the same cache lines,
// 2 = no global loads in the K loop
template <int EPI, int OM, int PIPE = DAMC_KM_PIPE, int DBG = 0>
__global__ __launch_bounds__(256, 2) void gemm_km_kernel(GemmArgs p) {
  constexpr int BK = KM_BK, RS = KM_RS, BM = KM_BM, MT = 2;
  __shared__ __attribute__((aligned(16))) float As[2][BM * RS];
  __shared__ __attribute__((aligned(16))) float Bs[2][BN * RS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int wgid = xcd_remap(blockIdx.x, gridDim.x);
  const int ntn = (p.N + BN - 1) / BN;
  const int tm = wgid / ntn, tn = wgid - tm * ntn;
  const int m0 = tm * BM, n0 = tn * BN;
  const int z = blockIdx.z;

  int pad_y = p.pad_y, pad_x = p.pad_x, py = 0, px = 0;
  const float* Bg = p.B;
  if (OM == O_PHASE) {
    py = z >> 1;
    px = z & 1;
    pad_y = 1 - py;
    pad_x = 1 - px;
    Bg += (long)z * p.b_zstride;
  }
  const int Cg = p.Cg, kw = p.kw, Win = p.Win;
  const int kh = p.K / Cg / kw;
  // O_DENSE: blockIdx.z is a split-K slice [kbeg, kend) (k_per_z a multiple of BK)
  const int kbeg = (OM == O_DENSE) ? z * p.k_per_z : 0;
  const int kend = (OM == O_DENSE) ? min(p.K, kbeg + p.k_per_z) : p.K;
  const int nk = kend > kbeg ? (kend - kbeg) / BK : 0;
  const int hwq = p.Hq * p.Wq;
  const int nimg = (p.M + hwq - 1) / hwq;
  const __amdgpu_buffer_rsrc_t rsA =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.A, (short)0, nimg * p.Hin * Win * Cg * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void*)Bg, (short)0, p.N * (int)p.ldb * 4, 0x00020000);

  // ---- per-thread rows: A rows / B rows (tid>>3) + 32j, float4 slot tid&7 of the K tile
  const int q4 = tid & 7, r0 = tid >> 3;
  int abase[4];
  unsigned amask[4], boff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + r0 + 32 * j;
    unsigned msk = 0;
    int base = 0;
    if (m < p.M) {
      const int b = m / hwq;
      const int r = m - b * hwq;
      const int qy = r / p.Wq, qx = r - qy * p.Wq;
      const int iy0 = qy * p.stride - pad_y, ix0 = qx * p.stride - pad_x;
      base = ((b * p.Hin + iy0) * Win + ix0) * Cg;
      for (int ky = 0; ky < kh; ++ky)
        for (int kx = 0; kx < kw; ++kx)
          if ((unsigned)(iy0 + ky) < (unsigned)p.Hin && (unsigned)(ix0 + kx) < (unsigned)Win)
            msk |= 1u << (ky * kw + kx);
    }
    abase[j] = base * 4 + q4 * 16;
    amask[j] = msk;
    boff[j] = (unsigned)((n0 + r0 + 32 * j) * (int)p.ldb * 4 + q4 * 16);  // rows >= N fall out of range
    if (DBG == 1) {
      abase[j] = q4 * 16;
      amask[j] = 0xFFFFFFFFu;
      boff[j] = q4 * 16;
    }
  }

  // ---- scalar tap walk over the K tiles still to be loaded
  int tap = kbeg / Cg, ci0 = kbeg - (kbeg / Cg) * Cg;
  int tky = tap / kw, tkx = tap - (tap / kw) * kw;
  unsigned aoff[4];
  auto set_tap = [&]() {
    const int toff = DBG == 1 ? 0 : (tky * Win + tkx) * Cg * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) aoff[j] = ((amask[j] >> (tap & 31)) & 1u) ? (unsigned)(abase[j] + toff) : KM_OOB;
  };
  set_tap();
  f32x4 ra[4], rb[4];
  auto load_ab = [&](int k0) {
    if (DBG == 2) return;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)aoff[j], DBG == 1 ? 0 : ci0 * 4, 0));
#pragma unroll
    for (int j = 0; j < 4; ++j)
      rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)boff[j], DBG == 1 ? 0 : k0 * 4, 0));
    ci0 += BK;
    if (ci0 == Cg) {
      ci0 = 0;
      ++tap;
      if (++tkx == kw) {
        tkx = 0;
        ++tky;
      }
      set_tap();
    }
  };
  // branch-free form for the interleaved pipelines (one basic block per K step): a tile past the end
  // of K loads nothing (every offset out of range) and the tap walk advances with selects
  auto load_ab_nb = [&](int k0) {
    const bool live = k0 < kend;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)(live ? aoff[j] : KM_OOB), ci0 * 4, 0));
#pragma unroll
    for (int j = 0; j < 4; ++j)
      rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)(live ? boff[j] : KM_OOB), k0 * 4, 0));
    ci0 += BK;
    const int wrap = ci0 == Cg;
    ci0 = wrap ? 0 : ci0;
    tap = min(tap + wrap, 31);
    tkx += wrap;
    const int wx = tkx == kw;
    tkx = wx ? 0 : tkx;
    tky += wx;
    set_tap();
  };
  auto store_ab = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<f32x4*>(&As[buf][(r0 + 32 * j) * RS + 4 * q4]) = ra[j];
      *reinterpret_cast<f32x4*>(&Bs[buf][(r0 + 32 * j) * RS + 4 * q4]) = rb[j];
    }
  };

  f32x16 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int lrow = lane & 31, lk = lane >> 5;
  const int afr = (wm * 64 + lrow) * RS + 4 * lk, bfr = (wn * 64 + lrow) * RS + 4 * lk;
  auto read_frags = [&](int buf, f32x4 (&fa)[4][MT], f32x4 (&fb)[4][2]) {
    const float* as = As[buf];
    const float* bs = Bs[buf];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int i = 0; i < MT; ++i) fa[q][i] = *reinterpret_cast<const f32x4*>(as + afr + 32 * i * RS + 8 * q);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[q][j] = *reinterpret_cast<const f32x4*>(bs + bfr + 32 * j * RS + 8 * q);
    }
  };
  auto mfma_tile = [&](const f32x4 (&fa)[4][MT], const f32x4 (&fb)[4][2]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][i][s2], fb[q][0][s2], acc[i][0], 0, 0, 0);
          acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][i][s2], fb[q][1][s2], acc[i][1], 0, 0, 0);
        }
  };

  constexpr int SG_MFMA = 0x8, SG_VMEM_RD = 0x20, SG_DS_RD = 0x100, SG_DS_WR = 0x200;
  if (PIPE == 0 || PIPE == 2) {  // PIPE >= 3: the prefetch structure below
    if (nk > 0) {
      load_ab(kbeg);
      store_ab(0);
      if (nk > 1) load_ab(kbeg + BK);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      f32x4 fa[4][MT], fb[4][2];
      if (PIPE == 0) {
        read_frags(cur, fa, fb);
        if (kt + 1 < nk) {
          store_ab(cur ^ 1);
          if (kt + 2 < nk) load_ab(kbeg + (kt + 2) * BK);
        }
        mfma_tile(fa, fb);
      } else {
        // stores past the last tile land in the buffer nobody reads again; loads past K are empty
        read_frags(cur, fa, fb);
        store_ab(cur ^ 1);
        load_ab_nb(kbeg + (kt + 2) * BK);
        mfma_tile(fa, fb);
        // the first k-quad's 4 fragments, then the remaining reads, stores and loads one per MFMA
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 4, 0);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
          __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
          __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
          __builtin_amdgcn_sched_group_barrier(SG_VMEM_RD, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 36, 0);
      }
      __syncthreads();
    }
  } else {
    // prologue: tiles 0 and 1 staged, tile 2 in flight, fragments of tile 0 resident
    if (nk > 0) {
      load_ab(kbeg);
      store_ab(0);
      if (nk > 1) {
        load_ab(kbeg + BK);
        store_ab(1);
        if (nk > 2) load_ab(kbeg + 2 * BK);
      }
    }
    __syncthreads();
    f32x4 f0a[4][MT], f0b[4][2], f1a[4][MT], f1b[4][2];
    if (nk > 0) read_frags(0, f0a, f0b);
    auto step = [&](int kt, const f32x4 (&fca)[4][MT], const f32x4 (&fcb)[4][2], f32x4 (&fna)[4][MT],
                    f32x4 (&fnb)[4][2]) {
      __syncthreads();
      if (PIPE == 1) {
        if (kt + 1 < nk) read_frags((kt + 1) & 1, fna, fnb);
        if (kt + 2 < nk) {
          store_ab(kt & 1);
          if (kt + 3 < nk) load_ab(kbeg + (kt + 3) * BK);
        }
        mfma_tile(fca, fcb);
      } else {
        read_frags((kt + 1) & 1, fna, fnb);
        store_ab(kt & 1);
        load_ab_nb(kbeg + (kt + 3) * BK);
        mfma_tile(fca, fcb);
        // one LDS read / LDS write / global load per MFMA gap, so every wave always has MFMAs ready
        if (PIPE == 3) {  // 16 reads, 8 writes, 8 loads on the first 32 MFMAs
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_VMEM_RD, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(SG_MFMA, 32, 0);
        } else if (PIPE == 4) {  // the same order spread over all 64 MFMAs
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_VMEM_RD, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
          }
        } else {  // PIPE 5: global loads first (they have the longest latency), then reads, then writes
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_VMEM_RD, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(SG_MFMA, 32, 0);
        }
      }
    };
    for (int kt = 0; kt < nk; kt += 2) {
      step(kt, f0a, f0b, f1a, f1b);
      if (kt + 1 < nk) step(kt + 1, f1a, f1b, f0a, f0b);
    }
  }
  if (OM == O_PHASE) {
    // one row-offset division per row instead of one per (row, lane): table in the (drained) A buffer
    long* rowtab = reinterpret_cast<long*>(&As[0][0]);
    __syncthreads();
    if (tid < BM) rowtab[tid] = gemm_row_offset<OM>(p, m0 + tid, py, px);
    __syncthreads();
    gemm_epilogue<EPI, OM, MT>(p, acc, m0, n0, wm, wn, lane, z, py, px, rowtab);
  } else {
    gemm_epilogue<EPI, OM, MT>(p, acc, m0, n0, wm, wn, lane, z, py, px);
  }
}

// The first layer's input gradient at per-rank batches (dz_slabs: M = B dense rows as a 1 x 1 "convolution",
// split-K slices of k_per_z, EPI_STORE into per-slice slabs): one workgroup per (slice, 128 columns, 32 rows), 4 waves of 32
// columns, every fragment straight from memory into registers with 4 K tiles' loads in flight (the 128 x 128 kernel
// walks a slice's 8 K tiles through a 2-3 deep LDS pipeline, latency-bound at this size).  The same 32x32x2 MFMA
// sequence per output (k-quad q, then step s; lane half lk takes k = 8 q + 4 lk + s of each 32-deep tile) from zero
// per slice, so every slab value is bitwise gemm_km_kernel's.
__global__ __launch_bounds__(256) void km_skinny_kernel(GemmArgs p) {
  constexpr int KU = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 31, lk = lane >> 5;
  const int z = blockIdx.x, n0 = blockIdx.y * 128 + wave * 32, rb0 = blockIdx.z * 32;
  const int kbeg = z * p.k_per_z, kend = min(p.K, kbeg + p.k_per_z);
  const int nk = kend > kbeg ? (kend - kbeg) / KM_BK : 0;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, (short)0, p.M * p.Cg * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.B, (short)0, p.N * (int)p.ldb * 4, 0x00020000);
  constexpr int OOB = 0x7FFFFFF0;
  const int aoff = rb0 + lrow < p.M ? ((rb0 + lrow) * p.Cg + 4 * lk) * 4 : OOB;
  const int boff = n0 + lrow < p.N ? ((n0 + lrow) * (int)p.ldb + 4 * lk) * 4 : OOB;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int kt = 0; kt < nk; kt += KU) {
    f32x4 fa[KU][4], fb[KU][4];
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool live = kt + u < nk;
        const int k0 = (kbeg + (kt + u) * KM_BK + 8 * q) * 4;
        fa[u][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 ra, live ? aoff : OOB, live ? k0 : 0, 0));
        fb[u][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 rb, live ? boff : OOB, live ? k0 : 0, 0));
      }
    __builtin_amdgcn_sched_barrier(0);  // every load of the batch issued before the first MFMA waits on one
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if (kt + u >= nk) break;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u][q][s2], fb[u][q][s2], acc, 0, 0, 0);
    }
  }
  float* Cz = p.C + (long)z * p.c_zstride;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = rb0 + (r & 3) + 8 * (r >> 2) + 4 * lk, n = n0 + lrow;
    if (m < p.M && n < p.N) Cz[(long)m * p.ldc + n] = acc[r];
  }
}

template <int EPI, int OM, int PIPE = DAMC_KM_PIPE, int DBG = 0>
static void launch_km_t(const GemmArgs& a, int zdim, hipStream_t s) {
  const int ntm = (a.M + KM_BM - 1) / KM_BM, ntn = (a.N + BN - 1) / BN;
  hipLaunchKernelGGL((gemm_km_kernel<EPI, OM, PIPE, DBG>), dim3(ntm * ntn, 1, zdim), dim3(256), 0, s, a);
}

// K-major dispatch; splits the batch so every launch's gathered tensor stays below 2^31 bytes
int launch_gemm_km(const GemmArgs& a, Epi epi, OMode om, int zdim, hipStream_t s) {
  const int taps = a.Cg > 0 ? a.K / a.Cg : 0;
  if (!conv_kmajor_ok(a.Cg) || taps * a.Cg != a.K || a.kw <= 0 || taps % a.kw != 0 || taps > 32) return DAMC_ERR_ARG;
  if (om == O_PHASE && zdim != 4) return DAMC_ERR_ARG;
  if (om == O_DENSE && (a.k_per_z <= 0 || a.k_per_z % KM_BK != 0 ||
                        (long)zdim * a.k_per_z < a.K || (long)(zdim - 1) * a.k_per_z >= a.K))
    return DAMC_ERR_ARG;
  if (a.ldb < a.K || ((uintptr_t)a.A | (uintptr_t)a.B) % 16 != 0 || (a.ldb % 4) != 0) return DAMC_ERR_ARG;
  if ((double)a.N * a.ldb * 4 >= 2147483647.0) return DAMC_ERR_UNSUPPORTED;
  const long hwq = (long)a.Hq * a.Wq;
  if (a.M % hwq != 0) return DAMC_ERR_ARG;
  const long img = (long)a.Hin * a.Win * a.Cg;  // floats per gathered image
  const long nimg = a.M / hwq;
  // DAMC_KM_CHUNK_BYTES lowers the per-launch limit (tests exercise the chunked path on small inputs)
  static const long lim = [] {
    const char* e = getenv("DAMC_KM_CHUNK_BYTES");
    const long v = e ? atol(e) : 0;
    return (v > 0 && v < 2147483647L) ? v : 2147483647L;
  }();
  const long per = (lim / 4 - 1) / img;
  if (per < 1) return DAMC_ERR_UNSUPPORTED;
  const long cimg = (om == O_PHASE) ? (long)a.Hout * a.Wout * a.ldc : hwq * a.ldc;  // output floats per image
  for (long b0 = 0; b0 < nimg; b0 += per) {
    const long nb = std::min(per, nimg - b0);
    GemmArgs c = a;
    c.A = a.A + b0 * img;
    c.C = a.C + b0 * cimg;
    if (a.mask) c.mask = a.mask + b0 * cimg;
    c.M = (int)(nb * hwq);
    // dz_slabs at per-rank batches: km_skinny_kernel (bitwise gemm_km_kernel); DAMC_KM_SKINNY=0 (read per call) keeps
    // the tiled kernel
    const char* esk = getenv("DAMC_KM_SKINNY");
    // rows: up to 64, in 32-row workgroups (round 6: SVHN B=64's two workgroups per slice took 11.4 us against 17.2 for
    // one 64-row workgroup of two tiles per wave, profiles/r06/km_skinny_mt.txt); DAMC_KM_SKINNY_ROWS (read per call)
    // moves the limit for A/B against the tiled kernel
    const char* ekr = getenv("DAMC_KM_SKINNY_ROWS");
    const int km_rows = ekr ? atoi(ekr) : 64;
    if (epi == EPI_STORE && om == O_DENSE && c.M <= km_rows && c.Hin == 1 && c.Win == 1 && c.Hq == 1 && c.Wq == 1 &&
        c.kw == 1 && c.Cg == c.K && !(esk && esk[0] == '0')) {
      const dim3 g((unsigned)zdim, (unsigned)((c.N + 127) / 128), (unsigned)((c.M + 31) / 32));
      hipLaunchKernelGGL(km_skinny_kernel, g, dim3(256), 0, s, c);
      continue;
    }
#define DAMC_KM(E_, O_)                \
  if (epi == E_ && om == O_) {         \
    launch_km_t<E_, O_>(c, zdim, s);   \
    continue;                          \
  }
    DAMC_KM(EPI_BIAS_ACT, O_PHASE)
    DAMC_KM(EPI_MASK, O_DENSE)
    DAMC_KM(EPI_BIAS_ACT, O_DENSE)
    DAMC_KM(EPI_STORE, O_DENSE)
#undef DAMC_KM
    return DAMC_ERR_UNSUPPORTED;
  }
  return (int)hipGetLastError();
}

}  // namespace damc
