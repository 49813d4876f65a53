// gemm_x3.hip — limb engine: fp32-accurate convolution GEMM on bf16 MFMA; launch_gemm (gemm.hip) dispatches here
// for limb operands (GemmArgs::A3, or a_f32 with B3).  The limb split and weight-pack kernels are in x3_pack.hip, the
// tile constants, swizzles and variant bits in gemm_impl.h.
//
// Every fp32 operand value a is carried as three bf16 limbs a = a0 + a1 + a2 (RNE splits: a0 = bf16(a),
// a1 = bf16(a - a0), a2 = bf16(a - a0 - a1); both subtractions are exact, so the limbs hold all 24
// significand bits).  A product a*b is the sum of the six limb products with i + j <= 2; the dropped
// three are below 2^-23 |ab|.  Each limb product is exact in the MFMA (8 x 8 significand bits) and the
// sum is accumulated in fp32 by v_mfma_f32_16x16x32_bf16, smallest terms first.  Error against fp64 is
// the fp32 GEMM's (tools/gemm_bench.hip prints both), at 16/6 of the fp32-MFMA rate per clock.
//
// "x3" tensor layout: a row of C channels is C/8 octets, each octet stored as [limb][8] bf16 (48 B), so
// a 32-channel K tile of one row is 192 contiguous bytes.  The A operand is an NHWC x3 map gathered by
// the same tap walk as the K-major engine (a K tile never straddles a tap, padding taps read zero
// through an out-of-range buffer offset); B is x3 over K, [n][K/8][3][8].
//
// Block 256 x 128, 8 waves (4 along M x 2 along N), each wave 64 x 64 of accumulators.
// LDS rows are the 192 B of a K tile, unpadded, with the four 48-B octets of row r stored at octet
// position q ^ ((r >> 1) & 3): the ds_read_b128 lane groups of a 16x16x32 fragment read ({0-3,12-15,
// 20-27}, ...) then hit 16 distinct 4-bank groups, and the staging writes are lane-linear (each thread
// stores the PHYSICAL chunk id % 12 of row id / 12 and gathers the matching logical chunk), so 8-lane
// write groups are contiguous.  Double-buffered: 2 x 384 rows x 192 B = 147,456 B, one workgroup per CU.
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "gemm_impl.h"

namespace damc {

// Output-layer projection of 16 rows of an LDS tile (row stride ts floats, C channels, C % 16 == 0) on
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation): lane (row m = lane & 15, quarter q = lane >> 4) reads
// the f32x4 run c = 16 g + 4 q .. + 3 of its row and of weight row n = 16 t + m, element e feeding MFMA step e (one k
// bijection for both operands).  acc[t][r] = P[row r0 + 4 q + r][16 t + m].  gemm_x3_kernel's fused epilogue and
// proj_rows_kernel share it, so the two forms are bitwise equal.
template <int NT>
__device__ __forceinline__ void proj16(const float* tile, int ts, int r0, int C, const float* w, int ldw,
                                       f32x4 (&acc)[NT]) {
  const int lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < C / 16; ++g) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(tile + (r0 + m) * ts + 16 * g + 4 * q);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(w + (long)(16 * t + m) * ldw + 16 * g + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc[t], 0, 0, 0);
    }
  }
}

// proj16 in two parts, for a caller that has other work to put between them: proj16_load_w takes this lane's weight
// fragments of a chunk of cw <= PROJ_CHUNK channels (proj16's b operands: row 16 t + m, k = 16 g + 4 q .. + 3; zero past
// cw) to registers, proj16_w runs proj16's MFMA sequence per output on them -- so the weight loads overlap whatever
// comes between instead of chaining through proj16's k loop, and the result is bitwise proj16's
template <int NT, int G0 = 0, int G1 = PROJ_CHUNK / 16>
__device__ __forceinline__ void proj16_load_w(const float* w, int ldw, int cw, f32x4 (&wb)[PROJ_CHUNK / 16][NT]) {
  const int lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
#pragma unroll
  for (int g = G0; g < G1; ++g)
#pragma unroll
    for (int t = 0; t < NT; ++t)
      wb[g][t] = 16 * g < cw ? *reinterpret_cast<const f32x4*>(w + (long)(16 * t + m) * ldw + 16 * g + 4 * q)
                             : f32x4{0.f, 0.f, 0.f, 0.f};
}
template <int NT>
__device__ __forceinline__ void proj16_w(const float* tile, int ts, int r0, int cw, const f32x4 (&wb)[PROJ_CHUNK / 16][NT],
                                         f32x4 (&acc)[NT]) {
  const int lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < PROJ_CHUNK / 16; ++g) {
    if (16 * g >= cw) break;
    const f32x4 a = *reinterpret_cast<const f32x4*>(tile + (r0 + m) * ts + 16 * g + 4 * q);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wb[g][t][e], acc[t], 0, 0, 0);
  }
}

// the projection alone: 128 pixels per workgroup (8 waves x 16 rows) staged in LDS with gemm_x3_kernel's WIDE tile
// stride, then proj16 (NT = np / 16) per 128-channel chunk (PROJ_CHUNK): chunk j's chain goes to partial buffer j
// (P + j npix np), and the gather adds the partials in order -- the chunking of the F32A tile's fused projection, whose
// workgroups each hold one 128-channel N tile
template <int NT>
__global__ __launch_bounds__(512) void proj_rows_kernel(const float* __restrict__ h, long npix, int C,
                                                        const float* __restrict__ w, int ldw, float* __restrict__ P,
                                                        long pstride) {
  constexpr int TS = 256 + 4;
  __shared__ __attribute__((aligned(16))) float tile[128 * TS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long p0 = (long)blockIdx.x * 128;
  const int c4 = C / 4;
  for (int i = tid; i < 128 * c4; i += 512) {
    const int r = i / c4, c = (i - r * c4) * 4;
    const long pix = p0 + r;
    *reinterpret_cast<f32x4*>(tile + r * TS + c) =
        pix < npix ? *reinterpret_cast<const f32x4*>(h + pix * C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  const int m = lane & 15, q = lane >> 4;
  for (int c0 = 0; c0 < C; c0 += PROJ_CHUNK) {  // one chain per 128-channel chunk, into its own partial buffer
    f32x4 acc[NT];
    proj16<NT>(tile + c0, TS, wave * 16, min(PROJ_CHUNK, C - c0), w + c0, ldw, acc);
    float* Pc = P + (c0 / PROJ_CHUNK) * pstride;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long pix = p0 + wave * 16 + 4 * q + r;
        if (pix < npix) Pc[pix * (16 * NT) + 16 * t + m] = acc[t][r];
      }
  }
}

int launch_proj_rows(const float* h, long npix, int C, const float* w, int ldw, int np, float* P, long pstride,
                     hipStream_t s) {
  if (C <= 0 || C > 256 || C % 16 || (np != 32 && np != 64) || npix <= 0) return DAMC_ERR_ARG;
  if (C > PROJ_CHUNK && pstride < npix * np) return DAMC_ERR_ARG;
  const dim3 grid((unsigned)((npix + 127) / 128));
  if (np == 32)
    hipLaunchKernelGGL(proj_rows_kernel<2>, grid, dim3(512), 0, s, h, npix, C, w, ldw, P, pstride);
  else
    hipLaunchKernelGGL(proj_rows_kernel<4>, grid, dim3(512), 0, s, h, npix, C, w, ldw, P, pstride);
  return (int)hipGetLastError();
}

// The limb GEMM kernel (V: the variant bits, gemm_impl.h).  One function body, in this order; each stage starts at the
// comment quoted here:
//   tile and split-K setup           from the top: raster, phase, K range, buffer descriptors
//   per-thread chunk table           "---- per-thread chunks", then the tap walk (set_tap, next_ktile) and dma_ab
//   the K loop, one of four          NARROW "---- 64 x 128 tile" | F32A "---- fp32 A image" (per-tap) |
//                                    TSHARE "---- X3_TAPSHARE" (tap-shared; inside the F32A branch, which holds the
//                                    lambdas both share) | "---- the limb A image" (X3_BASE, WIDE, KREG, O_WGRAD)
//   slab store                       KREG: inside the loops' block flush (flush_blk / "split-K: every sign block");
//                                    KSPLIT row-major: "row-major slabs", behind the tile write
//   epilogue                         "---- epilogue through LDS": TSHARE unsplit "the tap-shared tile's own epilogue",
//                                    every other launch the `octet` / `epilogue` lambdas
//   norm statistics                  "the encoder norm's statistics of this tile"
// The stages are not functions of their own: lifted into __forceinline__ templates (tried: both epilogues, the tile
// write, the row-major slab store, the statistics), hipcc generated different code for every instantiation the lifted
// stage is part of, several with other register counts (profiles/r22/isa_identity.txt).
template <int EPI, int OM, int V = X3_BASE>
__global__ __launch_bounds__(512, (V & X3_NARROW) ? 2 : 1) void gemm_x3_kernel(GemmArgs p) {
  static_assert((V & X3_BASE) == X3_BASE && !(V & ~X3_BITS), "V: X3_BASE and the named variant bits only");
  constexpr bool WIDE = (V & X3_WIDE) != 0;
  constexpr bool NARROW = (V & X3_NARROW) != 0;
  static_assert(!NARROW || !(V & (X3_RASTER | X3_WIDE | X3_KREG | X3_F32A)), "NARROW: the default limb path, unsplit");
  constexpr int BM = WIDE ? 128 : NARROW ? 64 : X3_BM, BN = WIDE ? 256 : X3_BN;
  // X3_F32A: A staged as fp32 (4 B per element instead of 6 B of limbs) and split into its RNE limbs in registers after
  // the fragment read, the same split as the producing epilogue's, so the MFMA operands and results are bitwise the
  // limb path's; waves 8 along M x 1 along N (each 32 x 128), so every A element is split by one wave only (the per-tap
  // loop; the X3_TAPSHARE loop reads its A fragments as limbs from LDS and keeps the 4 x 2 grid of 64 x 64)
  constexpr bool F32A = (V & X3_F32A) != 0;
  static_assert(!F32A || (OM != O_WGRAD && !WIDE), "F32A: 256 x 128 tiles, not the weight gradient");
  constexpr int AROWB = F32A ? X3A_ROWB : X3_ROWB, ESZ = F32A ? 4 : 6;
  constexpr int AJ = (BM * (F32A ? 8 : X3_CHUNKS) + 511) / 512, BJ = BN * X3_CHUNKS / 512;  // NARROW: 1.5 -> 2
  // one LDS buffer (A image, then B image)
  constexpr int BUFB = BM * AROWB + BN * X3_ROWB;
  // X3_TAPSHARE's LDS instead: the limb image of the current group, the fp32 staging image of the next, the two B
  // images, four all-zero limb rows and the read table (one word per walk position and tile row)
  constexpr int TS_NT = OM == O_PHASE ? 4 : 16;
  constexpr int TS_STG = BM * X3_ROWB, TS_B = TS_STG + BM * X3A_ROWB, TS_ZERO = TS_B + 2 * BN * X3_ROWB;
  constexpr int TS_TOFF = TS_ZERO + 4 * X3_ROWB, TS_END = TS_TOFF + TS_NT * BM * 4;
  constexpr int SMEMB =
      ((V & X3_TAPSHARE) && TS_END > 2 * (BM + BN) * X3_ROWB) ? TS_END : 2 * (BM + BN) * X3_ROWB;
  static_assert(SMEMB <= 160 * 1024 && TS_ZERO % 256 == 0, "the LDS of a CU; zero rows on the images' bank phase");
  // K tiles per MFMA accumulation block = the GEMM's sign block (GemmArgs::negk, a power of two >= 32)
  const int FLOG = __builtin_ctz((unsigned)p.negk >> 5), FLUSH = 1 << FLOG;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEMB];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (WIDE || NARROW) ? wave >> 2 : wave >> 1, wn = (WIDE || NARROW) ? wave & 3 : wave & 1;
  unsigned long long clk_t0 = 0, clk_r0 = 0;
  if (p.clk && tid == 0) {
    clk_t0 = __builtin_amdgcn_s_memtime();
    clk_r0 = __builtin_amdgcn_s_memrealtime();
  }
  constexpr bool RASTER = (V & X3_RASTER) != 0 && OM != O_WGRAD;
  const int wgid = xcd_remap(blockIdx.x, gridDim.x);
  const int ntn = (p.N + BN - 1) / BN;
  int tm, tn, z;
  if constexpr (RASTER) {
    const int nph = OM == O_PHASE ? 4 : 1;
    const int ntm = (p.M + BM - 1) / BM;
    int pr;
    supertile(wgid, ntm, ntn * nph, tm, pr);
    tn = pr / nph;
    z = pr - tn * nph;
  } else {
    tm = wgid / ntn;
    tn = wgid - tm * ntn;
    z = blockIdx.z;
  }
  const int m0 = tm * BM, n0 = tn * BN;

  int pad_y = p.pad_y, pad_x = p.pad_x, py = 0, px = 0;
  const unsigned short* Bg = p.B3;
  // split-K (O_PHASE / O_DENSE): z = phase * (ksplit / kbpw) + workgroup slice of kbpw sign blocks
  const bool KSPLIT = OM != O_WGRAD && p.ksplit > 1;
  constexpr bool KREG = (V & X3_KREG) != 0;  // register-layout slabs (launched only split)
  static_assert(!KREG || !WIDE, "KREG: 256 x 128 tiles only");
  constexpr bool TSHARE = (V & X3_TAPSHARE) != 0;
  static_assert(!TSHARE || F32A, "TAPSHARE: the F32A path (on the slice-major walk)");
  const int nslz = KSPLIT ? p.ksplit / p.kbpw : 1;
  const int zph = KSPLIT ? z / nslz : z, zsl = KSPLIT ? z - zph * nslz : 0;
  if (OM == O_PHASE) {
    py = zph >> 1;
    px = zph & 1;
    pad_y = 1 - py;
    pad_x = 1 - px;
    Bg += (long)zph * p.b_zstride * 3;
  }
  int kbeg = 0, kend = p.K;
  if (KSPLIT) {
    kbeg = zsl * p.k_per_z;
    kend = min(p.K, kbeg + p.k_per_z);
  }
  if constexpr (OM == O_WGRAD) {  // z = phase * slices + split-K slice
    const int nsl = gridDim.z / p.wg_phases;
    const int ph = z / nsl, sl = z - ph * nsl;
    if (p.wg_phases == 4) {
      py = ph >> 1;
      px = ph & 1;
      pad_y = 1 - py;
      pad_x = 1 - px;
    } else {
      pad_y = pad_x = 0;
    }
    Bg += (long)ph * p.b_zstride * 3;
    kbeg = sl * p.k_per_z;
    kend = min(p.K, kbeg + p.k_per_z);
  }
  const int Cg = p.Cg, kw = p.kw, Win = p.Win;
  const int kh = p.K / Cg / kw;
  const int nk = (OM == O_WGRAD || KSPLIT) ? max(kend - kbeg, 0) / X3_BK : p.K / X3_BK;
  const int kt0 = kbeg / X3_BK;  // global index of the first K tile (sign blocks follow the global index)
  const int hwq = p.Hq * p.Wq;
  const int nimg = (p.M + hwq - 1) / hwq;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      F32A ? (void*)p.A : (void*)p.A3, (short)0, (OM == O_WGRAD) ? Cg * p.K * 6 : nimg * p.Hin * Win * Cg * ESZ,
      0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc((void*)Bg, (short)0, p.N * p.K * 6, 0x00020000);

  // ---- per-thread chunks: chunk id = tid + 512 j -> (row id / 12, 16-B chunk id % 12)
  int abase[AJ];
  unsigned amask[AJ], boff[BJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int nch = F32A ? 8 : X3_CHUNKS;
    const int id = tid + 512 * j, row = id / nch, ch = id - row * nch;
    const int m = m0 + row;
    unsigned msk = 0;
    int base = 0;
    if constexpr (OM == O_WGRAD) {
      // row m = (tap, ci): A row ci shifted by (dy, dx) pixels = (dy * Win + dx) * wg_bp elements; the shift
      // is packed into the mask word ((dy+1) | (dx+1) << 2), all-ones for rows beyond M
      msk = 0xFFFFFFFFu;
      if (m < p.M) {
        const int t = m / Cg, ci = m - t * Cg;
        const int ty = t / kw, tx = t - ty * kw;
        const int dy = ty - pad_y, dx = tx - pad_x;
        base = ci * p.K + (dy * Win + dx) * p.wg_bp;
        msk = (unsigned)(dy + 1) | ((unsigned)(dx + 1) << 2);
      }
    } else if (m < p.M) {
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
    const int q = (ch / 3) ^ x3_swz(row), limb = ch - (ch / 3) * 3;  // logical octet of physical chunk ch
    abase[j] = F32A ? base * 4 + ((id & 7) ^ f32a_swz(row & 15)) * 16 : base * 6 + q * 48 + limb * 16;
    amask[j] = msk;
  }
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int id = tid + 512 * j, row = id / X3_CHUNKS, ch = id - row * X3_CHUNKS;
    const int q = (ch / 3) ^ x3_swz(row), limb = ch - (ch / 3) * 3;
    boff[j] = (unsigned)((n0 + row) * p.K * 6 + q * 48 + limb * 16);  // rows >= N fall out of range
  }

  int tap = 0, ci0 = 0, tky = 0, tkx = 0;
  // GemmArgs::kwalk: K tile kt = channels 32 (kt / WT) .. of the tap at walk position wpos = kt % WT; O_DENSE (a
  // 4 x 4 conv): WT = 16, tap x3_walk_tap(wpos); O_PHASE (a phase's 2 x 2 conv): WT = 4, tap wpos
  const bool walk = OM != O_WGRAD && p.kwalk != 0;
  constexpr int WT = OM == O_PHASE ? 4 : 16;
  int wpos = 0;
  if (OM != O_WGRAD && kbeg > 0) {  // a split slice starts mid-walk
    if (walk) {
      const int kt = kbeg / X3_BK;
      wpos = kt & (WT - 1);
      ci0 = (kt / WT) * X3_BK;
      tap = OM == O_PHASE ? wpos : x3_walk_tap(wpos);
    } else {  // tap-major: K tile = (tap, 32 channels)
      tap = kbeg / Cg;
      ci0 = kbeg - tap * Cg;
    }
    tky = tap / kw;
    tkx = tap - tky * kw;
  }
  unsigned aoff[AJ];
  auto set_tap = [&]() {
    const int toff = (tky * Win + tkx) * Cg * ESZ;
#pragma unroll
    for (int j = 0; j < AJ; ++j) aoff[j] = ((amask[j] >> (tap & 31)) & 1u) ? (unsigned)(abase[j] + toff) : KM_OOB;
  };
  set_tap();
  // the next K tile's (channels, tap): tap-major, or the 4 x 4 conv walk
  auto next_ktile = [&]() {
    if (walk) {
      if (++wpos == WT) {
        wpos = 0;
        ci0 += X3_BK;
      }
      tap = OM == O_PHASE ? wpos : x3_walk_tap(wpos);
      tky = OM == O_PHASE ? tap >> 1 : tap >> 2;
      tkx = OM == O_PHASE ? tap & 1 : tap & 3;
      set_tap();
      return;
    }
    ci0 += X3_BK;
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
  // LDS-DMA form: chunk id -> LDS byte 16 id, so each wave-instruction fills 1 KiB at a wave-uniform base
  typedef __attribute__((address_space(3))) void* lds_t;
  const int wbase = (tid & ~63) * 16;
  auto dma_ab = [&](int k0, int buf) {
    unsigned char* base = smem + buf * BUFB + wbase;
    if constexpr (OM == O_WGRAD) {
      // the K tile is 32 samples of ONE pixel (wg_bp % 32 == 0): a chunk is live when its shifted pixel
      // lies inside the grid
      const int pix = k0 / p.wg_bp;
      const int qy = pix / Win, qx = pix - qy * Win;
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        const int dy = (int)(amask[j] & 3u) - 1, dx = (int)((amask[j] >> 2) & 3u) - 1;
        const bool live = amask[j] != 0xFFFFFFFFu && (unsigned)(qy + dy) < (unsigned)p.Hin &&
                          (unsigned)(qx + dx) < (unsigned)Win;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_t)(base + 512 * 16 * j), 16,
                                                 live ? (int)(abase[j] + k0 * 6) : (int)KM_OOB, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < AJ; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_t)(base + 512 * 16 * j), 16, (int)aoff[j], ci0 * ESZ, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_t)(base + BM * AROWB + 512 * 16 * j), 16, (int)boff[j],
                                               k0 * 6, 0, 0);
    if constexpr (OM != O_WGRAD) next_ktile();
  };

  // Blocked accumulation: the MFMA chain runs over FLUSH K tiles, then adds into tot16 (a second fp32 sum
  // over the blocks, round-to-nearest VALU adds) and restarts from zero.  Rounding error of one output then
  // grows with sqrt(K/32 * FLUSH) + K/32/sqrt(FLUSH) instead of K/32: ~3x less at K = 16384
  // (tools/diag_hq.py), for 64 VGPRs and 64 v_add_f32 per FLUSH tiles.
  // Sign alternation (b_negblk): v_mfma_f32_16x16x32_bf16 aligns its 32 products and the accumulator before
  // one rounding and drops the low bits toward -inf, a bias of -0.19 x 2^-24 max|term| per instruction on
  // random operands that flips sign when the operands are negated (tools/mfma_bias.hip).  A bias that keeps
  // its sign survives every later layer and the first layer's 32768-term sum where rounding noise cancels
  // (tools/diag_chain.py: 3x the CPU's error on CelebA-HQ's z gradient); with -B stored on odd blocks and
  // those blocks subtracted, consecutive blocks' biases cancel.
  f32x4 acc16[4][4], tot16[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc16[i][j] = tot16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // a fragment's lane: row lrow of a 16-row tile, quarter loct = octet loct of the row (the whole 32-deep K tile in one
  // MFMA); tile bases are multiples of 16 rows, so the row swizzle is a function of lrow alone
  const int lrow = lane & 15, loct = lane >> 4;
  const int sw = x3_swz(lrow);
  const int afr = (wm * 64 + lrow) * X3_ROWB, bfr = (BM + wn * 64 + lrow) * X3_ROWB;
  const int oct16 = (loct ^ sw) * 48;

  auto flush16 = [&](int ktd) {  // block flush after the MFMAs of K tile ktd
    const float sg = (p.b_negblk && (((ktd + kt0) >> FLOG) & 1)) ? -1.f : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) tot16[i][j][r] = __builtin_fmaf(sg, acc16[i][j][r], tot16[i][j][r]);
        acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  };
  if constexpr (NARROW) {
    // ---- 64 x 128 tile: A chunks 512 .. 767 are issued by waves 0-3 only (wave-uniform guard); per K tile each wave
    // reads 2 A + 2 B tiles (12 ds_read_b128) and runs 24 MFMAs, smallest limb products first
    auto dma_n = [&](int k0, int buf) {
      unsigned char* base = smem + buf * BUFB + wbase;
#pragma unroll
      for (int j = 0; j < AJ; ++j)
        if (512 * j + (tid & ~63) < BM * X3_CHUNKS)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_t)(base + 512 * 16 * j), 16, (int)aoff[j], ci0 * 6, 0, 0);
#pragma unroll
      for (int j = 0; j < BJ; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_t)(base + BM * X3_ROWB + 512 * 16 * j), 16, (int)boff[j],
                                                 k0 * 6, 0, 0);
      next_ktile();
    };
    if (nk > 0) dma_n(kbeg, 0);
    __syncthreads();
    const int afn = (wm * 32 + lrow) * X3_ROWB, bfn = (BM + wn * 32 + lrow) * X3_ROWB;
    for (int kt = 0; kt < nk; ++kt) {
      const unsigned char* base = smem + (kt & 1) * BUFB;
      if (kt + 1 < nk) dma_n(kbeg + (kt + 1) * X3_BK, (kt + 1) & 1);
      bf16x8 fa[2][3], fb[2][3];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          fa[t][l] = *reinterpret_cast<const bf16x8*>(base + afn + t * 16 * X3_ROWB + oct16 + l * 16);
          fb[t][l] = *reinterpret_cast<const bf16x8*>(base + bfn + t * 16 * X3_ROWB + oct16 + l * 16);
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x4 c = acc16[i][j];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][2], fb[j][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[j][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][2], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[j][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][1], c, 0, 0, 0);
          acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][0], c, 0, 0, 0);
        }
      __syncthreads();
      if (((kt + 1) & (FLUSH - 1)) == 0) {
        const float sg = (p.b_negblk && (((kt + kt0) >> FLOG) & 1)) ? -1.f : 1.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) tot16[i][j][r] = __builtin_fmaf(sg, acc16[i][j][r], tot16[i][j][r]);
            acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
  } else if constexpr (F32A) {
    // ---- fp32 A image (X3A_ROWB rows, f32a_swz), limb B image; wave w owns rows 32 w .. 32 w + 31 and all 128 columns:
    // acc16[2 a + (t >> 2)][t & 3] is A tile a (16 rows) x B tile t (16 columns).  A runs one tile ahead of B: during
    // tile kt's MFMAs (limb fragments of A(kt) in registers, B(kt) read from LDS one 16-column tile ahead) each wave
    // reads its fp32 rows of A(kt + 1) (4 ds_read_b128) and splits them into the next tile's limbs (split3_octet, the
    // producing epilogue's RNE split), so the split's VALU runs in the MFMA gaps.  LDS-DMA: B(kt + 1) and A(kt + 2)
    // are issued at the start of tile kt into the buffers tile kt - 1 finished with; the end-of-tile barrier lands
    // them.  Double-buffered: 2 x (256 x 128 + 128 x 192) B.
    auto dma_a = [&](int buf) {
      unsigned char* dst = smem + buf * BUFB + wbase;
#pragma unroll
      for (int j = 0; j < AJ; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_t)(dst + 512 * 16 * j), 16, (int)aoff[j], ci0 * ESZ, 0, 0);
      next_ktile();
    };
    // B image buf: at BOFF behind the start of buffer buf
    constexpr int BOFF = TSHARE ? TS_B : BM * X3A_ROWB, BBUF = TSHARE ? BN * X3_ROWB : BUFB;
    // the tap-shared loop keeps the wave's LDS-DMA base in an SGPR: no v_readfirstlane per DMA instruction (round 11:
    // they pay for the two more read-address v_xor of the 4 x 2 grid, SQ_INSTS_VALU stays below round 9's)
    const int wbase_s = TSHARE ? __builtin_amdgcn_readfirstlane(wbase) : 0;
    auto dma_b = [&](int k0, int buf) {
      unsigned char* dst = smem + buf * BBUF + BOFF + (TSHARE ? wbase_s : wbase);
#pragma unroll
      for (int j = 0; j < BJ; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_t)(dst + 512 * 16 * j), 16, (int)boff[j], k0 * 6, 0, 0);
    };
    const int fs = f32a_swz(lrow);
    const int ca0 = ((2 * loct) ^ fs) * 16, ca1 = ((2 * loct + 1) ^ fs) * 16;
    const int arow = (wave * 32 + lrow) * X3A_ROWB, brow = BOFF + lrow * X3_ROWB + oct16;
    auto rd_a = [&](const unsigned char* buf, f32x4 (&av)[2][2]) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        av[a][0] = *reinterpret_cast<const f32x4*>(buf + arow + a * 16 * X3A_ROWB + ca0);
        av[a][1] = *reinterpret_cast<const f32x4*>(buf + arow + a * 16 * X3A_ROWB + ca1);
      }
    };
    // RNE limb split of elements e, e + 1 of A tile a (split3_octet's arithmetic, element by element)
    auto split2 = [&](const f32x4 (&av)[2][2], bf16x8 (&f)[2][3], int a, int e) {
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const float v = av[a][(e + d) >> 2][(e + d) & 3];
        const __bf16 b0 = (__bf16)v;
        const float r1 = sub_rn(v, (float)b0);
        const __bf16 b1 = (__bf16)r1;
        const float r2 = sub_rn(r1, (float)b1);
        f[a][0][e + d] = b0;
        f[a][1][e + d] = b1;
        f[a][2][e + d] = (__bf16)r2;
      }
    };
    auto rd_split = [&](const unsigned char* buf, bf16x8 (&f)[2][3]) {
      f32x4 av[2][2];
      rd_a(buf, av);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 8; e += 2) split2(av, f, a, e);
    };
    // ---- X3_TAPSHARE: one image per group of four K tiles.  The launcher guarantees the slice-major walk, whole groups
    // per workgroup (K slices start at multiples of 4 K tiles), hwq | 256 with 64-row pieces a uniform stride apart
    // (x3_tapshare_ok), and the geometry of a ConvT phase (2 x 2, stride 1) or of its input gradient (4 x 4, stride 2,
    // pad 1).
    // The fp32 image of a group is staged once (TS_STG: 256 rows x 128 B, ts_swz; piece j = rows 64 j .. 64 j + 63,
    // chunk id tid + 512 j; DMA: this thread's chunk of the undisplaced pixel of row tid >> 3, pieces ts_pstr bytes
    // apart, rows beyond M out of range) and split into limbs once (round 9), into the limb image at LDS byte 0: row r
    // = 192 B as three 64-B limb planes, octet q of limb l at l * 64 + (q ^ x3_swz(r)) * 16.  The four taps read their
    // MFMA A fragments from it at rows r + delta(tap) -- the limbs the in-register split of each tap's fp32 rows gave,
    // so the MFMA operands are bit for bit those of per-tap staging.  A row's slot (16-B bank group of ds_read_b128) is
    // 4 ((l - r) & 3) + (q ^ x3_swz(r)): every lane group of a fragment read hits 16 distinct slots for every row
    // rotation, and the 8-lane groups of the conversion's ds_write_b128 hit 8 distinct 16-B groups of their 32 banks.
    // TS_ZERO: four all-zero limb rows, one per r & 3: a padding tap reads the chunk it would read in a live row of
    // its residue, so it takes that row's slot and the lane group stays conflict-free.
    // TS_TOFF, the read table: for walk position pos and tile row r, the LDS byte of limb 0, octet 0 ^ x3_swz of the
    // row tap(pos) reads for r -- image row r + delta(pos), or the zero row -- built once per workgroup, so a tile's
    // read addresses (four rows 16 apart per lane) cost two ds_read2_b32 and four v_xor per lane.
    // Timeline of group G (K tiles 4 G .. 4 G + 3): the pieces of image G + 1 are DMA'd during tiles 4 G .. 4 G + 2 into
    // the staging image (its last reader, the conversion of G during tile 4 G - 1, retired by that tile's barrier);
    // during tile 4 G + 3 every thread reads its 16 staged values (two octets, rows wave * 32 + 16 a + lrow), splits
    // them in that tile's MFMA gaps and writes the 6 limb octets over image G, behind the tile's second barrier: every
    // tile reads its own A fragments (the 4 x 2 grid's twelve do not fit the register file a tile ahead), so tile
    // 4 G + 3 still reads image G in its first column; the barrier of 4 G + 3 publishes image G + 1.  Sign blocks are
    // whole groups (x3_tapshare_shape), so only a group's last tile flushes.
    unsigned ts_ibase = 0;
    int ts_nv = 0, ts_pstr = 0;
    // x3_tapshare_ok admits only grids whose Hq Wq divides 256, so Hq Wq and Wq are powers of two: a row's (image, y, x)
    // by shifts
    [[maybe_unused]] const int ts_lhw = TSHARE ? __builtin_ctz((unsigned)hwq) : 0,
                               ts_lwq = TSHARE ? __builtin_ctz((unsigned)p.Wq) : 0;
    if constexpr (TSHARE) {
      const int r0 = tid >> 3, mi = m0 + r0;
      const unsigned b = (unsigned)mi >> ts_lhw, r = mi & (hwq - 1), qy = r >> ts_lwq, qx = r & (p.Wq - 1);
      ts_ibase = ((b * p.Hin + qy * p.stride) * Win + qx * p.stride) * Cg * 4 + ((tid & 7) ^ ts_swz(r0)) * 16;
      ts_nv = min(4, max(0, (p.M - mi + 63) >> 6));
      ts_pstr = ((64 % hwq == 0) ? (64 >> ts_lhw) * p.Hin * Win : (64 >> ts_lwq) * p.stride * Win) * Cg * 4;
    }
    // the read table and the zero rows (round 14: built behind the issue of image 0's and B(0)'s DMA, which do not
    // depend on them; a thread's row -- id & 255 at stride 512 -- and its (y, x) are the same for all its entries)
    auto ts_table = [&]() {
      const int row = tid & (BM - 1), m = m0 + row;
      const int rr = m & (hwq - 1), y = rr >> ts_lwq, x = rr & (p.Wq - 1);
      const int iy = y * p.stride - pad_y, ix = x * p.stride - pad_x;
#pragma unroll
      for (int k = 0; k < TS_NT / 2; ++k) {
        const int pos = (tid >> 8) + 2 * k;
        int ky, kx, dlt;
        if constexpr (OM == O_PHASE) {
          ky = pos >> 1;
          kx = pos & 1;
          dlt = (ky - pad_y) * p.Wq + kx - pad_x;
        } else {
          const int c = pos >> 2, jj = pos & 3, tp = x3_walk_tap(pos);
          ky = tp >> 2;
          kx = tp & 3;
          dlt = ((jj >> 1) - 1 + (c >> 1)) * p.Wq + (jj & 1) - 1 + (c & 1);
        }
        const int R = row + dlt;
        const bool live = m < p.M && (unsigned)(iy + ky) < (unsigned)p.Hin && (unsigned)(ix + kx) < (unsigned)Win &&
                          (unsigned)R < (unsigned)BM;
        reinterpret_cast<int*>(smem + TS_TOFF)[tid + 512 * k] =
            (live ? R * X3_ROWB : TS_ZERO + (R & 3) * X3_ROWB) + x3_swz(R) * 16;
      }
      if (tid < 4 * X3_ROWB / 4) reinterpret_cast<float*>(smem + TS_ZERO)[tid] = 0.f;
    };
    // piece j of local group G: global group gg = (slice, class) for the 4 x 4 conv (class c = taps of parity (c >> 1,
    // c & 1), reading the pixels of the opposite parity), slice for a ConvT phase
    auto dma_img = [&](int G, int j) {
      const int gg = (kt0 >> 2) + G;
      int sl = gg, coff = 0;
      if constexpr (OM == O_DENSE) {
        const int c = gg & 3;
        sl = gg >> 2;
        coff = ((1 - (c >> 1)) * Win + (1 - (c & 1))) * Cg * 4;
      }
      unsigned char* dst = smem + TS_STG + wbase_s + 512 * 16 * j;
      const int vo = j < ts_nv ? (int)(ts_ibase + (unsigned)(j * ts_pstr)) : (int)KM_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_t)dst, 16, vo, sl * (X3_BK * 4) + coff, 0, 0);
    };
    // the LDS byte addresses (limb 0; limb l is 64 l further) of this lane's four fragment rows (A tile i of the wave's
    // 64 rows: row 64 wm + 16 i + lrow) of local K tile ktn, from the table: four words 64 B apart, two ds_read2_b32;
    // every address is an image row or a zero row
    const int ts_tb = TS_TOFF + (wm * 64 + lrow) * 4;
    auto ts_addr = [&](int ktn, int (&o)[4]) {
      const int ta = ts_tb + ((kt0 + ktn) & (TS_NT - 1)) * (BM * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = *reinterpret_cast<const int*>(smem + ta + i * 64) ^ (loct << 4);
    };
    // the conversion: this lane's two octets (rows wave * 32 + 16 a + lrow, octet loct) of the staging image ...
    const int cv_rd = TS_STG + (wave * 32 + lrow) * X3A_ROWB + ((2 * loct) ^ ts_swz(lrow)) * 16;
    auto rd_stg = [&](f32x4 (&av)[2][2], int a) {
      av[a][0] = *reinterpret_cast<const f32x4*>(smem + cv_rd + a * 16 * X3A_ROWB);
      av[a][1] = *reinterpret_cast<const f32x4*>(smem + (cv_rd ^ 16) + a * 16 * X3A_ROWB);
    };
    // ... and their limbs into the limb image
    const int cv_wr = (wave * 32 + lrow) * X3_ROWB + (loct ^ sw) * 16;
    auto wr_limb = [&](const bf16x8 (&f)[2][3], int a) {
#pragma unroll
      for (int l = 0; l < 3; ++l) *reinterpret_cast<bf16x8*>(smem + cv_wr + a * 16 * X3_ROWB + l * 64) = f[a][l];
    };
    bf16x8 fx[2][3], fy[2][3], fb[2][3];
    constexpr int SG_MFMA = 0x8, SG_VALU = 0x2, SG_DS_RD = 0x100, SG_DS_WR = 0x200;
    auto mfma6 = [&](const bf16x8 (&fc)[2][3], int t) {  // B tile t (slot t & 1) against both A tiles
      const int sl = t & 1;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        f32x4 c = acc16[2 * a + (t >> 2)][t & 3];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[a][2], fb[sl][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[a][1], fb[sl][1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[a][0], fb[sl][2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[a][1], fb[sl][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[a][0], fb[sl][1], c, 0, 0, 0);
        acc16[2 * a + (t >> 2)][t & 3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[a][0], fb[sl][0], c, 0, 0, 0);
      }
    };
    // the end of a sign block after the MFMAs of K tile kt: into the register slab (KREG) or the block total
    auto flush_blk = [&](int kt) {
      if constexpr (KREG) {
        // the register slab layout of the 4 x 2 wave grid (x3_ksplit_reduce_tile_kernel): A tile a of this wave is
        // row tile (w & 1) * 2 + a of wave row w >> 1, B tile t is column tile t & 3 of wave column t >> 2
        const float sg = (p.b_negblk && (((kt + kt0) >> FLOG) & 1)) ? -1.f : 1.f;
        const int ntile = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
        const __amdgpu_buffer_rsrc_t rsl = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.kslab + ((long)zph * p.ksplit + zsl * p.kbpw) * ntile * (BM * BN)), (short)0,
            p.kbpw * ntile * (BM * BN) * 4, 0x00020000);
        const int soff = ((kt >> FLOG) * ntile + tm * ntn + tn) * (BM * BN * 4);
        if constexpr (TSHARE) {
          // the tap-shared loop runs on the 4 x 2 grid itself (round 11): acc16[i][j] is tile i * 4 + j of wave `wave`;
          // the offset whole in the VGPR and soffset 0, as below
          const int voff = (wave * 1024 + lane) * 16;
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc16[i][j] *= sg;
              if (m0 + wm * 64 + i * 16 < p.M)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc16[i][j]), rsl,
                                                       voff + soff + (i * 4 + j) * 1024, 0, 0);
              acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
          return;
        }
        const int voff = ((wave >> 1) * 2 * 1024 + ((wave & 1) * 2) * 4 * 64 + lane) * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int a = i >> 1, wnp = i & 1;
            acc16[i][j] *= sg;
            if (m0 + wave * 32 + a * 16 < p.M) {
              // the whole offset in the VGPR, soffset the inline constant 0 (round 6; was SGPR soffset + an `s_nop 4`):
              // the VMEM-store-data hazard -- a > 64-bit store's data VGPRs rewritten by the next VALU before the store
              // has read them -- needs a wait state that LLVM's GCNHazardRecognizer (createsVALUHazard) inserts only
              // for MUBUF stores whose soffset is not an SGPR; with an SGPR soffset it assumed the exemption, the
              // register allocator reused the data VGPRs for the next tile's scaled copy at once, and 3 of every 16
              // slab tiles held the next tile's values on gfx950 (gemm_bench eq, profiles/r04/f32a_kreg_hazard.txt).
              // With soffset = 0 the recognizer pads the hazard itself (profiles/r06/kreg_store_isa.txt);
              // test_f32a_posterior_is_bitwise (B=16, register slabs) stays the gate
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc16[i][j]), rsl,
                                                     voff + soff + (wnp * 1024 + (a * 4 + j) * 64) * 16, 0, 0);
            }
            acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      } else {
        flush16(kt);
      }
    };
    if constexpr (TSHARE) {
      int oa[4], ob[4];  // fragment read addresses: this K tile's and the next one's
      if (nk > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) dma_img(0, j);
        dma_b(kbeg, 0);
      }
      ts_table();
      __syncthreads();  // the table, the zero rows, the staged image 0, B(0)
      {
        f32x4 av0[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          rd_stg(av0, a);
#pragma unroll
          for (int e = 0; e < 8; e += 2) split2(av0, fx, a, e);
          wr_limb(fx, a);
        }
      }
      ts_addr(0, oa);
      __syncthreads();  // limb image 0
      // K tile kt = position PH of its group, on the 4 x 2 wave grid (round 11): acc16[i][j] is A tile i (image rows
      // 64 wm + 16 i + lrow through the read table) x B tile j (B image rows 64 wn + 16 j + lrow), so a B fragment feeds
      // four A tiles: 12 A + 12 B ds_read_b128 per wave and tile instead of 6 + 24.  The four A tiles stay resident and
      // B streams through two slots, column by column -- (0, j) .. (3, j) for j = 0 .. 3 --: A tiles 1 .. 3 are read one
      // group of MFMAs ahead of their first use (every A read of the tile is issued within its first 12 MFMAs), B tile
      // j + 1 twelve MFMAs ahead.  A tile 0 of tiles PH 1 .. 3 is read during the previous tile's last 12 MFMAs, across its
      // barrier (the image does not change inside a group), so only B tile 0 stands in front of their first MFMA; PH 0
      // reads its own (six reads in front).  Measured: +0.2-0.3 % over reading every tile's own A tile 0
      // (profiles/r11/wave_grid_ab.txt).  oc: this tile's read addresses; on receives A(kt + 1)'s.
      // PH 3 converts image G + 1 over image G, which this tile's own A fragments still come from: a second barrier
      // after column 0 (every wave's A fragments in registers) stands between them and the first limb write.  That
      // barrier waits for the LDS-DMA in flight as any barrier does, so PH 3 issues B(kt + 1) behind it (in front of it:
      // 3 % slower).  The split runs one 16-row half at a time, in the MFMA gaps of column 1 and of column 2 (8 staged
      // values and 12 limb registers live at once; the whole conversion at once spills).
      bf16x8 pa[3];  // A tile 0 of the next K tile, read during this one's last MFMAs
      auto tile = [&](int kt, auto PH_, int (&oc)[4], int (&on)[4]) {
        constexpr int PH = decltype(PH_)::value;
        constexpr bool PFI = PH > 0, PFO = PH < 3;  // A tile 0 arrives in pa / the next tile's is read into it
        const unsigned char* base = smem + (PH & 1) * BBUF;  // groups start at even local tiles
        if constexpr (PH < 3) {
          if (kt + 1 < nk) dma_b(kbeg + (kt + 1) * X3_BK, (PH + 1) & 1);
          const int G = (kt >> 2) + 1;  // the next group's image: pieces 0 and 1, 2, 3
          if (4 * G < nk) {
            if constexpr (PH == 0) dma_img(G, 0);
            dma_img(G, PH + 1);
          }
        }
        bf16x8 fa[4][3], fq[2][3], fl[2][3];
        f32x4 av[2][2];
        auto rd_a = [&](int i) {
#pragma unroll
          for (int l = 0; l < 3; ++l) fa[i][l] = *reinterpret_cast<const bf16x8*>(smem + oc[i] + l * 64);
        };
        auto rd_b = [&](int j) {
#pragma unroll
          for (int l = 0; l < 3; ++l)
            fq[j & 1][l] = *reinterpret_cast<const bf16x8*>(base + brow + (wn * 64 + j * 16) * X3_ROWB + l * 16);
        };
        auto mf = [&](int i, int j) {  // the six limb products of A tile i x B tile j, smallest first
          const int sl = j & 1;
          f32x4 c = acc16[i][j];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][2], fq[sl][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fq[sl][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fq[sl][2], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fq[sl][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fq[sl][1], c, 0, 0, 0);
          acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fq[sl][0], c, 0, 0, 0);
        };
        // N MFMAs of the schedule, V of the split's VALU behind each (PH 3)
        auto pin = [&](auto N_, auto V_) {
#pragma unroll
          for (int m = 0; m < decltype(N_)::value; ++m) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            if constexpr (decltype(V_)::value > 0) __builtin_amdgcn_sched_group_barrier(SG_VALU, 1, 0);
            if constexpr (decltype(V_)::value > 1) __builtin_amdgcn_sched_group_barrier(SG_VALU, 1, 0);
          }
        };
        constexpr x3_ic<0> V0{};
        constexpr x3_ic<PH == 3 ? 2 : 0> V2{};
        // column 0, with the tile's remaining A reads, then B tile 1 and the next tile's addresses, behind its MFMAs
        if constexpr (PFI) {
#pragma unroll
          for (int l = 0; l < 3; ++l) fa[0][l] = pa[l];
        } else {
          rd_a(0);
        }
        rd_b(0);
        rd_a(1);
        mf(0, 0);
        rd_a(2);
        mf(1, 0);
        rd_a(3);
        mf(2, 0);
        rd_b(1);
        ts_addr(kt + 1, on);
        // (past the last group the conversion reads a stale, in-bounds staging image into an image nobody reads)
        if constexpr (PH == 3) rd_stg(av, 0);
        mf(3, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, PFI ? 3 : 6, 0);
        pin(x3_ic<1>{}, V0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        pin(x3_ic<5>{}, V0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        pin(x3_ic<6>{}, V0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        pin(x3_ic<6>{}, V0);
        // B tile 1, the table's two ds_read2_b32, PH 3: the staged values of the conversion's first half
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, PH == 3 ? 3 + 2 + 2 : 3 + 2, 0);
        pin(x3_ic<6>{}, V0);
        if constexpr (PH == 3) {
          // every A fragment of this wave is in its registers; behind the barrier, every wave's
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
          __builtin_amdgcn_sched_barrier(0);
          if (kt + 1 < nk) dma_b(kbeg + (kt + 1) * X3_BK, 0);
        }
        // columns 1 .. 3: B tile j + 1 into the slot column j - 1 released, 12 MFMAs ahead; PH 3: one half of the
        // conversion in the gaps of column 1, the other in those of column 2, each written at the next column's start
        if constexpr (PH == 3) split2(av, fl, 0, 0);
        mf(0, 1);
        if constexpr (PH == 3) split2(av, fl, 0, 2);
        mf(1, 1);
        rd_b(2);
        if constexpr (PH == 3) split2(av, fl, 0, 4);
        mf(2, 1);
        if constexpr (PH == 3) split2(av, fl, 0, 6);
        mf(3, 1);
        if constexpr (PH == 3) {
          wr_limb(fl, 0);
          rd_stg(av, 1);
          split2(av, fl, 1, 0);
        }
        mf(0, 2);
        if constexpr (PH == 3) split2(av, fl, 1, 2);
        mf(1, 2);
        rd_b(3);
        if constexpr (PH == 3) split2(av, fl, 1, 4);
        mf(2, 2);
        if constexpr (PH == 3) split2(av, fl, 1, 6);
        mf(3, 2);
        if constexpr (PH == 3) wr_limb(fl, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) mf(i, 3);
        if constexpr (PFO) {
#pragma unroll
          for (int l = 0; l < 3; ++l) pa[l] = *reinterpret_cast<const bf16x8*>(smem + on[0] + l * 64);
        }
        pin(x3_ic<12>{}, V2);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        pin(x3_ic<12>{}, V2);
        if constexpr (PH == 3) {
          __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 3, 0);
          __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 2, 0);
        }
        pin(x3_ic<12>{}, V2);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        pin(x3_ic<12>{}, V2);
        if constexpr (PH == 3) __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 3, 0);
        pin(x3_ic<12>{}, V0);
        if constexpr (PFO) __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        pin(x3_ic<12>{}, V0);
        __syncthreads();
        if constexpr (PH == 3) {
          if (((kt + 1) & (FLUSH - 1)) == 0) flush_blk(kt);
        }
      };
      for (int kt = 0; kt < nk; kt += 4) {  // one group per trip: the address sets trade roles in place
        tile(kt, std::integral_constant<int, 0>{}, oa, ob);
        tile(kt + 1, std::integral_constant<int, 1>{}, ob, oa);
        tile(kt + 2, std::integral_constant<int, 2>{}, oa, ob);
        tile(kt + 3, std::integral_constant<int, 3>{}, ob, oa);
      }
    } else {
      if (nk > 0) {
        dma_a(0);
        dma_b(kbeg, 0);
      }
      if (nk > 1) dma_a(1);
      __syncthreads();
      rd_split(smem, fx);
      auto tile = [&](int kt, bf16x8 (&fc)[2][3], bf16x8 (&fn)[2][3]) {
        const unsigned char* base = smem + (kt & 1) * BUFB;
        if (kt + 1 < nk) dma_b(kbeg + (kt + 1) * X3_BK, (kt + 1) & 1);
        if (kt + 2 < nk) dma_a(kt & 1);
        // A(kt + 1): read and split unconditionally (past the last tile it is stale, in-bounds LDS, never used); two
        // elements per B tile, in that tile's MFMA gaps
        f32x4 av[2][2];
        rd_a(smem + ((kt + 1) & 1) * BUFB, av);
        auto rd_b = [&](int t, int slot) {
#pragma unroll
          for (int l = 0; l < 3; ++l) fb[slot][l] = *reinterpret_cast<const bf16x8*>(base + brow + t * 16 * X3_ROWB + l * 16);
        };
        rd_b(0, 0);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (t + 1 < 8) rd_b(t + 1, (t + 1) & 1);
          split2(av, fn, t >> 2, (t & 3) * 2);
          mfma6(fc, t);
        }
        // schedule: the 4 A reads and B tiles 0 and 1 (6 reads) first, then per B tile t its 12 MFMAs with the split's
        // VALU in their gaps, then B tile t + 2's reads (into the slot tile t's MFMAs just released)
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 10, 0);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
#pragma unroll
          for (int m = 0; m < 12; ++m) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_VALU, 1, 0);
          }
          if (t + 2 < 8) __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        }
        // the next tile's limbs are complete before the barrier: otherwise the compiler sinks the split into the next
        // tile, where it runs ahead of the first MFMAs instead of in this tile's gaps
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int l = 0; l < 3; ++l) asm volatile("" : "+v"(fn[a][l]));
        __syncthreads();
        if (((kt + 1) & (FLUSH - 1)) == 0) flush_blk(kt);
      };
      for (int kt = 0; kt < nk; kt += 2) {  // two tiles per trip: the limb sets trade roles without register moves
        tile(kt, fx, fy);
        if (kt + 1 < nk) tile(kt + 1, fy, fx);
      }
    }
  } else {
    // ---- the limb A image (X3_BASE alone, X3_WIDE, X3_KREG; the only O_WGRAD path): each wave 4 x 4 tiles of 16 x 16
    if (nk > 0) dma_ab(kbeg, 0);
    __syncthreads();
    bf16x8 fa[4][3], fb[4][3];  // [tile][limb]
    // (the loop stays a lambda: written as a plain loop in the kernel body, hipcc orders the prologue and allocates
    // registers differently in every instantiation of this path; DESIGN.md, retired variant bits)
    auto kloop = [&]() {
      for (int kt = 0; kt < nk; ++kt) {
        const unsigned char* base = smem + (kt & 1) * BUFB;
        // the next tile goes into the other buffer (read before the previous barrier) now; the barrier at the end of
        // this tile (its vmcnt(0)) lands it (issuing it later -- after the fragment reads, or mid-MFMA -- measured
        // 10-15 % slower)
        if (kt + 1 < nk) dma_ab(kbeg + (kt + 1) * X3_BK, (kt + 1) & 1);
        // fragment reads one group ahead of the MFMAs that consume them, in the order those MFMAs run (A tile 0 against
        // B tiles 0..3, then A tiles 1..3), pinned by sched_group_barrier: the first MFMAs wait for 6 reads instead of
        // the ~15 the compiler's own schedule puts in front of its first lgkmcnt(0).  2.5-3.9 % less time on the four
        // CIFAR shapes, bit-identical results (profiles/r02/gemm_bench_rdorder.txt).  Measured and dropped: reading the
        // next tile's first fragments after the barrier into the registers the trailing MFMAs free (cross-tile pipeline,
        // 1-2 % slower than this), all reads issued by the end of A row 0 so the barrier moves up (5-8 % slower), A tile
        // 3 read later so it moves down (0-2 % slower).
        auto rd_a = [&](int t) {
#pragma unroll
          for (int l = 0; l < 3; ++l) fa[t][l] = *reinterpret_cast<const bf16x8*>(base + afr + t * 16 * X3_ROWB + oct16 + l * 16);
        };
        auto rd_b = [&](int t) {
#pragma unroll
          for (int l = 0; l < 3; ++l) fb[t][l] = *reinterpret_cast<const bf16x8*>(base + bfr + t * 16 * X3_ROWB + oct16 + l * 16);
        };
        auto mf = [&](int i, int j) {  // the six limb products of A tile i x B tile j, smallest first
          f32x4 c = acc16[i][j];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][2], fb[j][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[j][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][2], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[j][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][1], c, 0, 0, 0);
          acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][0], c, 0, 0, 0);
        };
        constexpr int SG_MFMA = 0x8, SG_DS_RD = 0x100;
        rd_a(0);
        rd_b(0);
        rd_b(1);
        mf(0, 0);
        rd_b(2);
        mf(0, 1);
        rd_b(3);
        mf(0, 2);
        rd_a(1);
        mf(0, 3);
        rd_a(2);
#pragma unroll
        for (int j = 0; j < 4; ++j) mf(1, j);
        rd_a(3);
#pragma unroll
        for (int i = 2; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) mf(i, j);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 9, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 6, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 6, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 6, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 6, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 24, 0);
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 3, 0);
        __builtin_amdgcn_sched_group_barrier(SG_MFMA, 48, 0);
        __syncthreads();
        // block flush after the barrier: the compiler keeps hoisting the barrier above the tile's trailing MFMAs
        // (a flush between them and the barrier measured 6-8 % slower)
        if (KREG) {
          if (((kt + 1) & (FLUSH - 1)) != 0) continue;
          // split-K: every sign block's signed sum straight from the accumulators into its own slab, in the register
          // layout (one 16-B store per lane and tile: 1 KB per wave-instruction); x3_ksplit_reduce_kernel maps back
          // buffer stores: one VGPR of offset (wave, lane), the rest scalar, so the 256 accumulator VGPRs do not spill
          const float sg = (p.b_negblk && (((kt + kt0) >> FLOG) & 1)) ? -1.f : 1.f;
          const int ntile = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
          const __amdgpu_buffer_rsrc_t rsl = __builtin_amdgcn_make_buffer_rsrc(
              (void*)(p.kslab + ((long)zph * p.ksplit + zsl * p.kbpw) * ntile * (BM * BN)), (short)0,
              p.kbpw * ntile * (BM * BN) * 4, 0x00020000);
          const int soff = ((kt >> FLOG) * ntile + tm * ntn + tn) * (BM * BN * 4);
          const int voff = (wave * 1024 + lane) * 16;
          const bool live = m0 + wm * 64 < p.M;  // a wave whose 64 rows are all past M stores nothing (the reduce skips them)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc16[i][j] *= sg;
              if (live)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc16[i][j]), rsl, voff,
                                                       soff + (i * 4 + j) * 1024, 0);
              acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else if (((kt + 1) & (FLUSH - 1)) == 0) {
          flush16(kt);
        }
      }
    };
    kloop();
  }
  if (p.clk && tid == 0) {  // the K loop's shader clocks over its 100 MHz ticks (damc_clock_probe)
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    unsigned long long* c = p.clk + 4 * ((blockIdx.z * gridDim.x + blockIdx.x) % (unsigned)p.clk_n);
    c[0] = clk_t0;
    c[1] = clk_r0;
    c[2] = t1;
    c[3] = r1;
  }
  if (KREG) return;  // every block already in its slab
  {  // the last partial block
    const float sg = (p.b_negblk && nk > 0 && (((nk - 1 + kt0) >> FLOG) & 1)) ? -1.f : 1.f;
    constexpr int MI = NARROW ? 2 : 4;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < MI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc16[i][j][r] = __builtin_fmaf(sg, acc16[i][j][r], tot16[i][j][r]);
  }
  // ---- epilogue through LDS: the block's 256 x 128 fp32 tile, then one thread per (row, channel octet):
  // 2 x 16-B fp32 stores and (C3) 3 x 16-B limb stores per octet, each row's 128 channels contiguous
  constexpr int TS = BN + 4;  // tile row stride (floats): 4-row groups of a 16x16 store land 16 banks apart
  static_assert(BM * TS * 4 + BM * 8 <= 2 * (BM + BN) * X3_ROWB, "epilogue tile exceeds the LDS");
  float* tile = reinterpret_cast<float*>(smem);
  long* rowtab = reinterpret_cast<long*>(smem + BM * TS * 4);
  float* Cz = p.C;
  if ((OM == O_DENSE || OM == O_WGRAD) && Cz) Cz += (long)(KSPLIT ? zph : z) * p.c_zstride;
  if constexpr (TSHARE) {
    // ---- the tap-shared tile's own epilogue (round 14; the unsplit launch -- a row-major slab goes the common way
    // below): the arithmetic per output of the common octet pass and of proj16, so every byte stays the per-tap
    // kernel's, scheduled for a CU whose MFMA pipes stand idle until the next tile's K loop:
    //  - the fused projection's weight fragments are loaded first (proj16_load_w), under the tile write and the octet
    //    pass, and the P stores take the output pixel from a second row table (rowpix) instead of dividing
    //    rowtab by ldc per stored value;
    //  - both row tables come from shifts (the grid's Hq Wq and Wq are powers of two);
    //  - a thread's octet column (id % 16 at stride 512) is the same in its 8 rows: its bias is loaded once.
    // Measured and not kept: a thread owning (row, four consecutive octets) with the four
    // sign bytes as one dword -- 1.2 % slower per step, also where only the sign bytes are stored.
    if (!KSPLIT) {  // workgroup-uniform
      static_assert(BM * TS * 4 + BM * 8 + BM * 4 <= SMEMB, "epilogue tile and row tables exceed the LDS");
      int* rowpix = reinterpret_cast<int*>(smem + BM * TS * 4 + BM * 8);
      auto ts_epilogue = [&](auto NT_) {  // NT: 16-column tiles of the fused projection, 0 without one
        constexpr int NT = decltype(NT_)::value;
        constexpr bool PROJ = NT > 0;
        f32x4 wb[PROJ_CHUNK / 16][PROJ ? NT : 1];
        const int cw = min(PROJ_CHUNK, p.N - n0);  // a chunk narrower than 128 channels: the dead columns are skipped
        // 64 registers of them here, under the tile write and the octet pass (np = 32: all; np = 64: the first four
        // channel groups, the other four behind the octet pass, whose own registers they would crowd out)
        constexpr int GW = NT <= 2 ? PROJ_CHUNK / 16 : PROJ_CHUNK / 32;
        if constexpr (PROJ) proj16_load_w<NT, 0, GW>(p.proj_w + n0, p.proj_ldw, cw, wb);
        if (tid < BM) {  // gemm_row_offset by shifts, and its pixel
          const int m = m0 + tid;
          long pix = -1;
          if (m < p.M) {
            if constexpr (OM == O_PHASE) {
              const int lhw = __builtin_ctz((unsigned)hwq), lwq = __builtin_ctz((unsigned)p.Wq);
              const int b = m >> lhw, rr = m & (hwq - 1), qy = rr >> lwq, qx = rr & (p.Wq - 1);
              pix = ((long)b * p.Hout + 2 * qy + py) * p.Wout + 2 * qx + px;
            } else {
              pix = m;
            }
          }
          rowtab[tid] = pix < 0 ? -1L : pix * p.ldc;
          if constexpr (PROJ) rowpix[tid] = (int)pix;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              tile[(wm * 64 + i * 16 + 4 * (lane >> 4) + r) * TS + wn * 64 + j * 16 + (lane & 15)] = acc16[i][j][r];
        __syncthreads();
        // one octet (8 channels from n0 + 8 oct of tile row `row`, output offset idx): the common octet pass's arithmetic
        // and stores but the sign byte, which it returns; bb: the octet's bias, mbits: its LReLU' mask bits
        auto octet8 = [&](int row, int oct, long idx, const float (&bb)[8], unsigned mbits) -> unsigned {
          const f32x4 t0 = *reinterpret_cast<const f32x4*>(tile + row * TS + oct * 8);
          const f32x4 t1 = *reinterpret_cast<const f32x4*>(tile + row * TS + oct * 8 + 4);
          float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
          if (EPI == EPI_BIAS_ACT) {
            if (p.bias) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] += bb[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = act_apply(v[e], p.act, p.slope);
          } else if (EPI == EPI_MASK) {
            if (p.mask_sgn) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] *= ((mbits >> e) & 1u) ? 1.f : p.mask_slope;
            } else {
              const f32x4 k0 = *reinterpret_cast<const f32x4*>(p.mask + idx);
              const f32x4 k1 = *reinterpret_cast<const f32x4*>(p.mask + idx + 4);
              const float kk[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] *= act_grad_from_out(kk[e], p.mask_act, p.mask_slope);
            }
          }
          unsigned bits = 0;
#pragma unroll
          for (int e = 0; e < 8; ++e) bits |= (v[e] > 0.f ? 1u : 0u) << e;
          if (Cz && !p.proj_nostore) {
            *reinterpret_cast<f32x4*>(Cz + idx) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(Cz + idx + 4) = f32x4{v[4], v[5], v[6], v[7]};
          }
          if (p.C3) {
            bf16x8 h, m, l;
            split3_octet(v, h, m, l);
            bf16x8* o = reinterpret_cast<bf16x8*>(p.C3 + 3 * idx);
            o[0] = h;
            o[1] = m;
            o[2] = l;
          }
          if constexpr (PROJ) {  // the stored row back into the tile, for the projection
            *reinterpret_cast<f32x4*>(tile + row * TS + oct * 8) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(tile + row * TS + oct * 8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
          }
          return bits;
        };
        {
          float bb[8] = {};  // this thread's octet column is id % 16 = tid & 15 in all of its rows
          if (EPI == EPI_BIAS_ACT && p.bias && n0 + (tid & 15) * 8 < p.N) {
            const int n = n0 + (tid & 15) * 8;
            const int nb = p.bias_mod < p.N ? n % p.bias_mod : n;
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + nb);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + nb + 4);
            bb[0] = b0.x, bb[1] = b0.y, bb[2] = b0.z, bb[3] = b0.w;
            bb[4] = b1.x, bb[5] = b1.y, bb[6] = b1.z, bb[7] = b1.w;
          }
#pragma unroll 2
          for (int it = 0; it < BM * BN / 8 / 512; ++it) {
            const int id = tid + 512 * it, row = id / (BN / 8), oct = id % (BN / 8);
            const int n = n0 + oct * 8;
            const long rowoff = rowtab[row];
            if (rowoff < 0 || n >= p.N) continue;
            const long idx = rowoff + n;
            const unsigned mb = (EPI == EPI_MASK && p.mask_sgn) ? p.mask_sgn[idx >> 3] : 0u;
            const unsigned sg = octet8(row, oct, idx, bb, mb);
            if (p.sgn) p.sgn[idx >> 3] = (unsigned char)sg;
          }
        }
        if constexpr (PROJ) {
          // the fused output-layer projection (GemmArgs::proj_out): this tile's channels n0 .. n0 + 127 are chunk
          // n0 / 128, 8 waves x 32 rows (two 16-row groups each), P indexed by the output pixel
          if constexpr (GW < PROJ_CHUNK / 16)
            proj16_load_w<NT, GW, PROJ_CHUNK / 16>(p.proj_w + n0, p.proj_ldw, cw, wb);
          __syncthreads();
          const int m = lane & 15, q = lane >> 4;
          // the tap-shared K loop has no register to carry this wave's row base across it: taken from the thread id anew
          int ptid = tid;
          asm volatile("" : "+v"(ptid));
          float* Pc = p.proj_out + (n0 / PROJ_CHUNK) * p.proj_pstride;
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            const int r0 = (ptid >> 6) * 32 + g * 16;
            // one row group at a time: scheduled across this point, the F32A ConvT forward (CIFAR B=128) measured
            // 0.8 % slower
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc[PROJ ? NT : 1];
            proj16_w<PROJ ? NT : 1>(tile, TS, r0, cw, wb, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int pix = rowpix[r0 + 4 * q + r];
#pragma unroll
              for (int t = 0; t < NT; ++t)
                if (pix >= 0) Pc[(long)pix * (16 * NT) + 16 * t + m] = acc[t][r];
            }
          }
        }
      };
      if constexpr (OM == O_PHASE && EPI == EPI_BIAS_ACT) {
        if (p.proj_out) {  // workgroup-uniform
          if (p.proj_np == 32)
            ts_epilogue(std::integral_constant<int, 2>{});
          else
            ts_epilogue(std::integral_constant<int, 4>{});
          return;
        }
      }
      ts_epilogue(std::integral_constant<int, 0>{});
      return;
    }
  }
  // one (row, channel octet) of the tile through the epilogue (bias + act / LReLU' mask, sign bits, fp32, limbs)
  auto octet = [&](int row, int oct) {
    const int n = n0 + oct * 8;
    const long rowoff = rowtab[row];
    if (rowoff < 0 || n >= p.N) return;
    const long idx = rowoff + n;
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(tile + row * TS + oct * 8);
    const f32x4 t1 = *reinterpret_cast<const f32x4*>(tile + row * TS + oct * 8 + 4);
    float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    if (EPI == EPI_BIAS_ACT) {
      if (p.bias) {
        const int nb = p.bias_mod < p.N ? n % p.bias_mod : n;
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + nb);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + nb + 4);
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bb[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = act_apply(v[e], p.act, p.slope);
    } else if (EPI == EPI_MASK) {
      if (p.mask_sgn) {  // LReLU' from the sign bits of the activation: 1 where it was > 0, else slope
        const unsigned bits = p.mask_sgn[idx >> 3];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= ((bits >> e) & 1u) ? 1.f : p.mask_slope;
      } else {
        const f32x4 k0 = *reinterpret_cast<const f32x4*>(p.mask + idx);
        const f32x4 k1 = *reinterpret_cast<const f32x4*>(p.mask + idx + 4);
        const float kk[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= act_grad_from_out(kk[e], p.mask_act, p.mask_slope);
      }
    }
    if (p.sgn) {
      unsigned bits = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) bits |= (v[e] > 0.f ? 1u : 0u) << e;
      p.sgn[idx >> 3] = (unsigned char)bits;
    }
    if (Cz && !p.proj_nostore) {
      *reinterpret_cast<f32x4*>(Cz + idx) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(Cz + idx + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
    if (p.C3) {
      bf16x8 h, m, l;
      split3_octet(v, h, m, l);
      bf16x8* o = reinterpret_cast<bf16x8*>(p.C3 + 3 * idx);
      o[0] = h;
      o[1] = m;
      o[2] = l;
    }
    if ((OM == O_PHASE && EPI == EPI_BIAS_ACT && (WIDE || F32A) && p.proj_out) ||
        (OM == O_DENSE && EPI == EPI_BIAS_ACT && !WIDE && !NARROW && p.in_part)) {  // the stored row back into the tile
      *reinterpret_cast<f32x4*>(tile + row * TS + oct * 8) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(tile + row * TS + oct * 8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
  };
  auto epilogue = [&]() {  // the whole tile
#pragma unroll 2
    for (int it = 0; it < BM * BN / 8 / 512; ++it) {
      const int id = tid + 512 * it;
      octet(id / (BN / 8), id % (BN / 8));
    }
    if constexpr (OM == O_PHASE && EPI == EPI_BIAS_ACT && (WIDE || F32A)) {
      // fused output-layer projection (GemmArgs::proj_out), proj16 as proj_rows_kernel, P indexed by the output pixel,
      // one chain per 128-channel chunk into partial buffer chunk (proj_rows_kernel's chunking).  WIDE: the tile holds
      // every channel (n0 == 0, N <= 256), 8 waves x 16 rows, all chunks.  F32A: the tile holds channels n0 .. n0 + 127
      // = chunk n0 / 128, 8 waves x 32 rows (two 16-row groups each)
      if (p.proj_out) {
        __syncthreads();
        const int m = lane & 15, q = lane >> 4;
        auto store = [&](auto NT_) {
          constexpr int NT = decltype(NT_)::value;
          constexpr int RG = F32A ? 2 : 1;
          // the tap-shared K loop has no register to carry this wave's row base across it: taken from the thread id anew
          int ptid = tid;
          if constexpr (TSHARE) asm volatile("" : "+v"(ptid));
#pragma unroll
          for (int g = 0; g < RG; ++g) {
            const int r0 = F32A ? (TSHARE ? ptid >> 6 : wave) * 32 + g * 16 : wave * 16;
            // one row group at a time: scheduled across this point, the F32A ConvT forward (CIFAR B=128) measured
            // 0.8 % slower
            __builtin_amdgcn_sched_barrier(0);
            for (int c0 = 0; c0 < (F32A ? BN : p.N); c0 += PROJ_CHUNK) {
              const int cc = F32A ? n0 : c0;  // global channel of the chunk's first column
              if (cc >= p.N) break;
              f32x4 acc[NT];
              proj16<NT>(tile + c0, TS, r0, min(PROJ_CHUNK, p.N - cc), p.proj_w + cc, p.proj_ldw, acc);
              float* Pc = p.proj_out + (cc / PROJ_CHUNK) * p.proj_pstride;
#pragma unroll
              for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const long ro = rowtab[r0 + 4 * q + r];
                  if (ro >= 0) Pc[(ro / p.ldc) * (16 * NT) + 16 * t + m] = acc[t][r];
                }
            }
          }
        };
        if (p.proj_np == 32)
          store(std::integral_constant<int, 2>{});
        else
          store(std::integral_constant<int, 4>{});
      }
    }
  };
  if (tid < BM) rowtab[tid] = (m0 + tid < p.M) ? gemm_row_offset<OM>(p, m0 + tid, py, px) : -1L;
  if (F32A && !TSHARE) {  // the per-tap loop's 8 x 1 waves; the tap-shared loop's 4 x 2 grid takes the last branch
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tile[(wave * 32 + (i >> 1) * 16 + 4 * (lane >> 4) + r) * TS + ((i & 1) * 4 + j) * 16 + (lane & 15)] =
              acc16[i][j][r];
  } else if (NARROW) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tile[(wm * 32 + i * 16 + 4 * (lane >> 4) + r) * TS + wn * 32 + j * 16 + (lane & 15)] = acc16[i][j][r];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tile[(wm * 64 + i * 16 + 4 * (lane >> 4) + r) * TS + wn * 64 + j * 16 + (lane & 15)] = acc16[i][j][r];
  }
  __syncthreads();
  if (KSPLIT) {  // row-major slabs (one block per workgroup): the fp32 tile into its slab; the reduce applies the epilogue
    float* sl = p.kslab + ((long)zph * p.ksplit + zsl) * p.M * p.N;
#pragma unroll 2
    for (int it = 0; it < BM * BN / 8 / 512; ++it) {
      const int id = tid + 512 * it, row = id / (BN / 8), oct = id % (BN / 8);
      const int m = m0 + row, n = n0 + oct * 8;
      if (m >= p.M || n >= p.N) continue;
      float* d = sl + (long)m * p.N + n;
      *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(tile + row * TS + oct * 8);
      *reinterpret_cast<f32x4*>(d + 4) = *reinterpret_cast<const f32x4*>(tile + row * TS + oct * 8 + 4);
    }
    return;
  }
  if constexpr (!TSHARE) epilogue();
  if constexpr (OM == O_DENSE && EPI == EPI_BIAS_ACT && !WIDE && !NARROW && BM == 256 && BN == 128) {
    // the encoder norm's statistics of this tile (GemmArgs::in_part): its 256 rows are one strip of one sample
    static_assert(BM * TS * 4 + BM * 8 + 1024 * 4 <= 2 * (BM + BN) * X3_ROWB, "statistics scratch exceeds the LDS");
    if (p.in_part && !KSPLIT) {  // workgroup-uniform
      __syncthreads();
      float* red = reinterpret_cast<float*>(smem + BM * TS * 4 + BM * 8);
      float st[3];
      strip256_stats(tile, TS, tid, n0 + (tid & 127) < p.N, red, st);
      if (tid < 128 && n0 + tid < p.N) {
        const int b = m0 / p.in_hw, sp = (m0 - b * p.in_hw) >> 8;
        float* o = p.in_part + (((long)b * p.N + n0 + tid) * p.in_S + sp) * 3;
        o[0] = st[0];
        o[1] = st[1];
        o[2] = st[2];
      }
    }
  }
}

// the split-K reduce: one thread per (phase, row, channel octet); the slices in fixed order, then the limb GEMM's
// epilogue (bias + act or the LReLU' mask, sign bits, fp32 and limb outputs) on the sum
// the epilogue of one output octet (8 consecutive channels n .. n + 7 of GEMM row m) from its fp32 sums
template <int EPI, int OM>
__device__ __forceinline__ void x3_octet_epilogue(const GemmArgs& p, int m, int n, int py, int px, float (&v)[8]);
template <int EPI>
__device__ __forceinline__ void x3_octet_epilogue_at(const GemmArgs& p, long idx, int n, float (&v)[8]);

// register slab layout, one wave per 16x16 MFMA tile: lane l sums its f32x4 (rows 4 (l >> 4) .. + 3, column l & 15)
// over the blocks in order (1 KB per wave-load; a thread per 4 rows x 8 channels measured 5-10 % slower per step at B=8-32), then the tile goes through
// LDS and 32 lanes apply the octet epilogue
template <int EPI, int OM>
__global__ __launch_bounds__(256) void x3_ksplit_reduce_tile_kernel(GemmArgs p, int zdim) {
  __shared__ float red[4][16][17];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long blk = (long)blockIdx.x * 4 + w;  // ((phase * ntile + tile) * 8 + wave) * 16 + tile16
  const int ntm = (p.M + X3_BM - 1) / X3_BM, ntn = (p.N + X3_BN - 1) / X3_BN;
  const long ntile = (long)ntm * ntn;
  const int ij = (int)(blk & 15), wave = (int)((blk >> 4) & 7);
  const long tl = blk >> 7;
  const int tile = (int)(tl % ntile), ph = (int)(tl / ntile);
  const int tm = tile / ntn, tn = tile - tm * ntn;
  const int m0 = tm * X3_BM + (wave >> 1) * 64 + (ij >> 2) * 16, n0 = tn * X3_BN + (wave & 1) * 64 + (ij & 3) * 16;
  const bool live = ph < zdim && m0 < p.M && n0 < p.N;  // wave-uniform
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const long sstride = ntile * (X3_BM * X3_BN / 4);
    const f32x4* src = reinterpret_cast<const f32x4*>(p.kslab) + (long)ph * p.ksplit * sstride +
                       (((long)tile * 8 + wave) * 16 + ij) * 64 + lane;
    // the blocks in order, the sign already applied; four slabs' loads in flight before their adds (one load per
    // trip left each lane waiting a memory round trip per slab: 11.5 us for 8 MB at CIFAR B=16)
    int sl = 0;
    for (; sl + 4 <= p.ksplit; sl += 4) {
      const f32x4 t0 = src[(long)sl * sstride], t1 = src[(long)(sl + 1) * sstride];
      const f32x4 t2 = src[(long)(sl + 2) * sstride], t3 = src[(long)(sl + 3) * sstride];
      v += t0;
      v += t1;
      v += t2;
      v += t3;
    }
    for (; sl < p.ksplit; ++sl) v += src[(long)sl * sstride];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[w][4 * (lane >> 4) + r][lane & 15] = v[r];
  __syncthreads();
  if (!live || lane >= 32) return;
  const int row = lane >> 1, oc = (lane & 1) * 8, m = m0 + row, n = n0 + oc;
  if (m >= p.M || n >= p.N) return;
  float o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = red[w][row][oc + c];
  const int py = OM == O_PHASE ? ph >> 1 : 0, px = OM == O_PHASE ? ph & 1 : 0;
  x3_octet_epilogue<EPI, OM>(p, m, n, py, px, o);
}

// the split-K reduce of a ConvT forward whose epilogue also runs the output layer's projection (GemmArgs::proj_out,
// register slab layout): one workgroup of 4 waves per (phase, 256 x 128 tile, 64-row quarter).  Wave w sums the 8
// 16x16 tiles of rows 16 w .. + 15 of the quarter (x3_ksplit_reduce_tile_kernel's per-lane order) into an LDS tile,
// the octet epilogue writes the sign bits (and C unless proj_nostore) and leaves the activated rows in the tile, and
// wave w projects its 16 rows with proj16 into the chunk's partial buffer -- the F32A tile's fused epilogue on the
// same sums, so the result is bitwise the unsplit kernel's, without the fp32 activation's write and re-read by
// proj_rows_kernel
template <int NT>
__global__ __launch_bounds__(256) void x3_ksplit_reduce_proj_kernel(GemmArgs p, int zdim) {
  constexpr int TS = X3_BN + 4, RW = 64;
  __shared__ __attribute__((aligned(16))) float tile[RW * TS];
  __shared__ long rowtab[RW];
  __shared__ int rowpix[RW];  // rowtab / ldc: the projection's output row
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ntm = (p.M + X3_BM - 1) / X3_BM, ntn = (p.N + X3_BN - 1) / X3_BN;
  const long ntile = (long)ntm * ntn;
  const int qtr = blockIdx.x & 3;
  const long tl = blockIdx.x >> 2;
  const int tile_i = (int)(tl % ntile), ph = (int)(tl / ntile);
  if (ph >= zdim) return;  // workgroup-uniform
  const int tm = tile_i / ntn, tn = tile_i - tm * ntn;
  const int py = ph >> 1, px = ph & 1;
  const int r16 = qtr * RW + 16 * w;  // this wave's 16 rows within the 256-row tile
  const int wm = r16 >> 6, ti = (r16 & 63) >> 4;
  const long sstride = ntile * (X3_BM * X3_BN / 4);
  const f32x4* src = reinterpret_cast<const f32x4*>(p.kslab) + (long)ph * p.ksplit * sstride + (long)tile_i * 8 * 16 * 64;
  f32x4 v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the chunk's projection weights (proj16's b operands: row 16 t + m, k = 16 g + 4 q .. + 3) into registers first,
  // so their loads overlap the slab loads instead of chaining through proj16's k loop
  const int cc = tn * X3_BN, cw = min(PROJ_CHUNK, p.N - cc);
  const int mm = lane & 15, qq = lane >> 4;
  f32x4 wb[PROJ_CHUNK / 16][NT];
#pragma unroll
  for (int g = 0; g < PROJ_CHUNK / 16; ++g)
#pragma unroll
    for (int t = 0; t < NT; ++t)
      wb[g][t] = 16 * g < cw ? *reinterpret_cast<const f32x4*>(p.proj_w + cc + (long)(16 * t + mm) * p.proj_ldw + 16 * g + 4 * qq)
                             : f32x4{0.f, 0.f, 0.f, 0.f};
  if (tm * X3_BM + r16 < p.M) {  // wave-uniform
    // two slabs' 16 loads in flight before their adds (in slab order per output)
    int sl = 0;
    for (; sl + 2 <= p.ksplit; sl += 2) {
      f32x4 t[2][8];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 8; ++u) {  // u = (wave_n, j): columns 64 (u >> 2) + 16 (u & 3)
          const int wv = wm * 2 + (u >> 2), ij = ti * 4 + (u & 3);
          t[h][u] = src[(long)(sl + h) * sstride + ((long)wv * 16 + ij) * 64 + lane];
        }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] += t[h][u];
    }
    for (; sl < p.ksplit; ++sl) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int wv = wm * 2 + (u >> 2), ij = ti * 4 + (u & 3);
        v[u] += src[(long)sl * sstride + ((long)wv * 16 + ij) * 64 + lane];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[(16 * w + 4 * (lane >> 4) + r) * TS + 16 * u + (lane & 15)] = v[u][r];
  if (tid < RW) {
    const int m = tm * X3_BM + qtr * RW + tid;
    const long ro = m < p.M ? gemm_row_offset<O_PHASE>(p, m, py, px) : -1;
    rowtab[tid] = ro;
    rowpix[tid] = ro >= 0 ? (int)(ro / p.ldc) : -1;
  }
  __syncthreads();
  GemmArgs q = p;
  if (p.proj_nostore) q.C = nullptr;
  for (int o = tid; o < RW * 16; o += 256) {
    const int row = o >> 4, oc = (o & 15) * 8;
    const int m = tm * X3_BM + qtr * RW + row, n = tn * X3_BN + oc;
    if (m >= p.M || n >= p.N) continue;
    float e8[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) e8[c] = tile[row * TS + oc + c];
    x3_octet_epilogue_at<EPI_BIAS_ACT>(q, rowtab[row] + n, n, e8);
    *reinterpret_cast<f32x4*>(tile + row * TS + oc) = f32x4{e8[0], e8[1], e8[2], e8[3]};
    *reinterpret_cast<f32x4*>(tile + row * TS + oc + 4) = f32x4{e8[4], e8[5], e8[6], e8[7]};
  }
  __syncthreads();
  // proj16's arithmetic (same MFMA sequence per output) with the preloaded weights
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < PROJ_CHUNK / 16; ++g) {
    if (16 * g >= cw) break;
    const f32x4 a = *reinterpret_cast<const f32x4*>(tile + (16 * w + mm) * TS + 16 * g + 4 * qq);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wb[g][t][e], acc[t], 0, 0, 0);
  }
  float* Pc = p.proj_out + (cc / PROJ_CHUNK) * p.proj_pstride;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pix = rowpix[16 * w + 4 * qq + r];
      if (pix >= 0) Pc[(long)pix * (16 * NT) + 16 * t + mm] = acc[t][r];
    }
}

template <int EPI, int OM>
__global__ void x3_ksplit_reduce_kernel(GemmArgs p, int zdim) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int noct = p.N / 8;
  if (i >= (long)zdim * p.M * noct) return;
  const int oct = (int)(i % noct);
  const long r = i / noct;
  const int m = (int)(r % p.M), ph = (int)(r / p.M);
  const int py = OM == O_PHASE ? ph >> 1 : 0, px = OM == O_PHASE ? ph & 1 : 0;
  const int n = oct * 8;
  // the blocks in order from 0: each add the kernel's fmaf(sign, block, tot) with the sign already applied
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int sl = 0; sl < p.ksplit; ++sl) {
    const float* src = p.kslab + ((long)(ph * p.ksplit + sl) * p.M + m) * p.N + n;
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(src);
    const f32x4 t1 = *reinterpret_cast<const f32x4*>(src + 4);
    v[0] += t0.x; v[1] += t0.y; v[2] += t0.z; v[3] += t0.w;
    v[4] += t1.x; v[5] += t1.y; v[6] += t1.z; v[7] += t1.w;
  }
  x3_octet_epilogue<EPI, OM>(p, m, n, py, px, v);
}

// the octet epilogue at output offset idx (row offset + n)
template <int EPI>
__device__ __forceinline__ void x3_octet_epilogue_at(const GemmArgs& p, long idx, int n, float (&v)[8]) {
  if (EPI == EPI_BIAS_ACT) {
    if (p.bias) {
      const int nb = p.bias_mod < p.N ? n % p.bias_mod : n;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += p.bias[nb + e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = act_apply(v[e], p.act, p.slope);
  } else if (EPI == EPI_MASK) {
    if (p.mask_sgn) {
      const unsigned bits = p.mask_sgn[idx >> 3];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= ((bits >> e) & 1u) ? 1.f : p.mask_slope;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= act_grad_from_out(p.mask[idx + e], p.mask_act, p.mask_slope);
    }
  }
  if (p.sgn) {
    unsigned bits = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) bits |= (v[e] > 0.f ? 1u : 0u) << e;
    p.sgn[idx >> 3] = (unsigned char)bits;
  }
  if (p.C) {
    *reinterpret_cast<f32x4*>(p.C + idx) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p.C + idx + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
  if (p.C3) {
    bf16x8 h, mm, l;
    split3_octet(v, h, mm, l);
    bf16x8* o = reinterpret_cast<bf16x8*>(p.C3 + 3 * idx);
    o[0] = h;
    o[1] = mm;
    o[2] = l;
  }
}
template <int EPI, int OM>
__device__ __forceinline__ void x3_octet_epilogue(const GemmArgs& p, int m, int n, int py, int px, float (&v)[8]) {
  x3_octet_epilogue_at<EPI>(p, gemm_row_offset<OM>(p, m, py, px) + n, n, v);
}

// Skinny limb GEMM for the first layer at per-rank batches (z . W, M = B <= 32 rows, K <= negk: one sign block,
// a 1 x 1 "convolution" of dense rows): 4 waves per workgroup, each 16 rows x 64 columns; the K tiles go from memory
// straight into registers (two tiles' 30 loads of 16 B per lane in flight, no LDS staging, no barrier) -- the
// 128 x 256 kernel streams its 50 MB of weight limbs through a two-deep LDS pipeline that left each workgroup
// latency-bound at 4 K tiles.  Same fragments (octet q of the tile per lane quarter), the same six-product MFMA
// sequence and the same block fold (fmaf(+1, acc, 0)), then gemm_x3_kernel's octet epilogue (x3_octet_epilogue):
// every output is bitwise the 128 x 256 kernel's (tests/test_gpu_langevin.py).
// Round 5: each wave takes 16 rows x 16 NTW columns (NTW = 2 by default: twice the waves of the 64-column form, which
// serialised its loads at 86 VGPRs, and half those of NTW = 1, whose 1024 workgroups measured 5-17 us slower per CIFAR
// B=16 step), and
// F32B reads the weights as fp32 rows split in registers with the packer's RNE split (2/3 of the limb bytes).  The
// MFMA sequence per output is unchanged, so every output is still bitwise the 128 x 256 kernel's.
template <bool F32B, int NTW>
__global__ __launch_bounds__(256) void x3_skinny_kernel(GemmArgs p) {
  constexpr int WC = 16 * NTW, KU = 4;  // columns per wave, K tiles per batch of loads
  __shared__ __attribute__((aligned(16))) float st[4][16][WC + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int n0 = (blockIdx.x * 4 + wave) * WC, r0 = blockIdx.y * 16;
  if (n0 >= p.N) return;  // wave-uniform; the waves share no barrier
  const int K8 = p.K >> 3, nk = p.K >> 5;
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.A3, (short)0, p.M * p.K * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = F32B ? __builtin_amdgcn_make_buffer_rsrc((void*)p.b32k, (short)0, p.N * p.K * 4, 0x00020000)
                                        : __builtin_amdgcn_make_buffer_rsrc((void*)p.B3, (short)0, p.N * p.K * 6, 0x00020000);
  constexpr int OOB = 0x7FFFFFF0;
  const int aoff = (r0 + m < p.M) ? ((r0 + m) * K8 + q) * 48 : OOB;
  int boff[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t)
    boff[t] = (n0 + 16 * t + m < p.N) ? (F32B ? ((n0 + 16 * t + m) * p.K + 8 * q) * 4 : ((n0 + 16 * t + m) * K8 + q) * 48)
                                      : OOB;
  f32x4 acc[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto ld = [&](const __amdgpu_buffer_rsrc_t& r, int off, int kt, int l) {
    // the sgpr offset must be wave-uniform (a per-lane soffset made the compiler wrap every load in a waterfall loop);
    // an out-of-range lane's voffset (OOB) alone takes the load out of range
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, off, kt * 192 + l * 16, 0));
  };
  for (int kt = 0; kt < nk; kt += KU) {
    bf16x8 fa[KU][3], fb[KU][NTW][3];
    if constexpr (F32B) {
      // 8 fp32 of row n per lane and K tile (two 16-B loads), split as the packer splits (K <= negk: sign block 0)
      f32x4 fv[KU][NTW][2];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const bool live = kt + u < nk;
#pragma unroll
        for (int l = 0; l < 3; ++l) fa[u][l] = ld(ra, live ? aoff : OOB, kt + u, l);
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            fv[u][t][h] = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, live ? boff[t] : OOB, (kt + u) * 128 + h * 16, 0));
      }
      __builtin_amdgcn_sched_barrier(0);  // every load of the batch issued before the split waits on one
#pragma unroll
      for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
          const float v[8] = {fv[u][t][0][0], fv[u][t][0][1], fv[u][t][0][2], fv[u][t][0][3],
                              fv[u][t][1][0], fv[u][t][1][1], fv[u][t][1][2], fv[u][t][1][3]};
          split3_octet(v, fb[u][t][0], fb[u][t][1], fb[u][t][2]);
        }
    } else {
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const bool live = kt + u < nk;
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          fa[u][l] = ld(ra, live ? aoff : OOB, kt + u, l);
#pragma unroll
          for (int t = 0; t < NTW; ++t) fb[u][t][l] = ld(rb, live ? boff[t] : OOB, kt + u, l);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // every load of the batch issued before the first MFMA waits on one
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if (kt + u >= nk) break;
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        f32x4 c = acc[t];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[u][2], fb[u][t][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[u][1], fb[u][t][1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[u][0], fb[u][t][2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[u][1], fb[u][t][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[u][0], fb[u][t][1], c, 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[u][0], fb[u][t][0], c, 0, 0, 0);
      }
    }
  }
  // the block fold of gemm_x3_kernel's last partial block (tot = 0, sign block 0 positive), then the epilogue
#pragma unroll
  for (int t = 0; t < NTW; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) st[wave][4 * q + r][16 * t + m] = __builtin_fmaf(1.f, acc[t][r], 0.f);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  constexpr int NOCT = 16 * WC / 8;  // (row, octet) items of the wave's tile
#pragma unroll
  for (int j = 0; j < (NOCT + 63) / 64; ++j) {
    const int id = lane + 64 * j, row = id / (WC / 8), oct = id % (WC / 8);
    const int mg = r0 + row, n = n0 + 8 * oct;
    if (id >= NOCT || mg >= p.M || n >= p.N) continue;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = st[wave][row][8 * oct + e];
    x3_octet_epilogue<EPI_BIAS_ACT, O_DENSE>(p, mg, n, 0, 0, v);
  }
}

// split-K plan of a limb-engine conv: an under-filled grid (see below; DAMC_X3_KSPLIT_WGS pins the bound) splits K
// into its negk sign blocks (GemmArgs::negk), one per slice.  A slice's tile is then exactly the unsplit kernel's block sum (sign applied), and the reduce adds
// the blocks in the kernel's order with the kernel's single rounding per block: the split result is bitwise the
// unsplit one, so a batch split over ranks (or calls) still reproduces the one-call chains bit for bit
int x3_ksplit(int M, int N, int K, int zdim, int bm, int bn, int negk = X3_NEGK) {
  // DAMC_X3_KSPLIT=0 disables; DAMC_X3_KSPLIT_WGS: the grid size below which a conv splits (A/B)
  const char* ev = getenv("DAMC_X3_KSPLIT");  // per call: tests compare both paths in one process
  const bool on = !(ev && ev[0] == '0');
  static const long below = [] {
    const char* e = getenv("DAMC_X3_KSPLIT_WGS");
    return e ? atol(e) : -1L;
  }();
  const long wgs = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * zdim;
  if (!on || K % negk != 0 || K / negk < 2) return 1;
  const int ks = K / negk;
  // default: below 128 workgroups always; below 256 (half the chip idle) when K has at most 16 sign blocks, since
  // the slab bytes grow with K (CIFAR B=16/32 per-rank steps -2.6 / -1.5 %, B=64's K=8192 dgrad stays unsplit)
  const bool split = below >= 0 ? wgs < below : (wgs < 128 || (wgs < 256 && ks <= 16));
  return split ? ks : 1;
}

long x3_ksplit_floats(int M, int N, int K, int zdim, int negk) {  // either block layout (gemm_x3_kernel, X3_WIDE)
  const int ks = std::max(x3_ksplit(M, N, K, zdim, X3_BM, X3_BN, negk), x3_ksplit(M, N, K, zdim, 128, 256, negk));
  // the register slab layout covers whole 256 x 128 tiles
  const long padded = (long)((M + X3_BM - 1) / X3_BM) * X3_BM * ((N + X3_BN - 1) / X3_BN) * X3_BN;
  return ks > 1 ? (long)zdim * ks * std::max((long)M * N, padded) : 0;
}

// whether an F32A launch stages one image per group of four K tiles (gemm_x3_kernel X3_TAPSHARE): the caller allows it
// (GemmArgs::tapshare), the walk is slice-major, the conv is a ConvT phase (2 x 2, stride 1) or the stride-2 4 x 4 input
// gradient, and the grid passes x3_tapshare_ok.  DAMC_X3_TAPSHARE=0 (read per call) keeps the per-tap staging (bitwise
// the same) for A/B
static std::atomic<unsigned long long> g_tapshare_launches{0};
static bool x3_tapshare_shape(const GemmArgs& a, OMode om) {
  if (!a.a_f32 || !a.kwalk || !x3_tapshare_ok(a.Hq, a.Wq) || a.negk % (4 * X3_BK) != 0) return false;
  if (om == O_PHASE)
    return a.kw == 2 && a.stride == 1 && a.Hin == a.Hq && a.Win == a.Wq && a.K == 4 * a.Cg;
  return om == O_DENSE && a.kw == 4 && a.stride == 2 && a.pad_y == 1 && a.pad_x == 1 && a.Hin == 2 * a.Hq &&
         a.Win == 2 * a.Wq && a.K == 16 * a.Cg;
}
static bool x3_tapshare_on() {
  const char* e = getenv("DAMC_X3_TAPSHARE");
  return !(e && e[0] == '0');
}

// V: X3_BASE, + X3_F32A, or + X3_WIDE, as launch_gemm_x3 chooses; X3_TAPSHARE, X3_KREG and X3_RASTER are added here
// (X3_NARROW: launch_x3_narrow_split)
template <int EPI, int OM, int V = X3_BASE>
static int launch_x3_t(const GemmArgs& a0, int zdim, hipStream_t s) {
  static_assert(OM != O_WGRAD && (V & X3_BASE) == X3_BASE && !(V & ~(X3_BASE | X3_F32A | X3_WIDE | X3_TAPSHARE)) &&
                    !((V & X3_WIDE) && (V & X3_F32A)),
                "the caller picks the operand form and the tile; the other variants are chosen below");
  constexpr bool F32A = (V & X3_F32A) != 0, WIDE = (V & X3_WIDE) != 0;
  if constexpr (F32A && !(V & X3_TAPSHARE) &&
                ((EPI == EPI_BIAS_ACT && OM == O_PHASE) || ((EPI == EPI_MASK || EPI == EPI_STORE) && OM == O_DENSE))) {
    if (a0.tapshare && x3_tapshare_on() && x3_tapshare_shape(a0, (OMode)OM)) {
      g_tapshare_launches.fetch_add(1, std::memory_order_relaxed);
      return launch_x3_t<EPI, OM, V | X3_TAPSHARE>(a0, zdim, s);
    }
  }
  GemmArgs a = a0;
  constexpr int BM = WIDE ? 128 : X3_BM, BN = WIDE ? 256 : X3_BN;
  const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
  // the norm statistics in the epilogue (GemmArgs::in_part): the unsplit 256 x 128 dense tile only; every other launch
  // clears in_done and leaves them to the caller's kernel
  auto no_stats = [&]() {
    if (a.in_part && a.in_done) *a.in_done = 0;
    a.in_part = nullptr;
  };
  if (a.in_part && !(OM == O_DENSE && EPI == EPI_BIAS_ACT && !WIDE && zdim == 1 && a.in_hw > 0 &&
                     a.in_hw % 256 == 0 && a.M % a.in_hw == 0 && a.in_S == a.in_hw / 256))
    no_stats();
  if (a.kslab) {
    const int ks = x3_ksplit(a.M, a.N, a.K, zdim, BM, BN, a.negk);
    if (ks > 1 && (long)zdim * ks * a.M * a.N <= a.kslab_floats && a.N % 8 == 0) {
      no_stats();
      a.ksplit = ks;
      const int nostore0 = a.proj_nostore;  // the caller's: honoured where the reduce runs the projection itself
      a.proj_nostore = 0;  // the reduce writes C; the projection then runs as proj_rows_kernel over it
      auto proj_after = [&]() {
        if (OM == O_PHASE && a.proj_out)
          return launch_proj_rows(a.C, (long)(a.M / (a.Hq * a.Wq)) * a.Hout * a.Wout, a.N, a.proj_w, a.proj_ldw,
                                  a.proj_np, a.proj_out, a.proj_pstride, s);
        return 0;
      };
      // sign blocks per workgroup: the most (a power of two dividing ks) that still leaves >= 256 workgroups, so one
      // round covers the chip (256 x 128 tiles only); DAMC_X3_KSPLIT_BPW (read per call) pins it
      int bpw = 1;
      if (!WIDE) {
        const char* eb = getenv("DAMC_X3_KSPLIT_BPW");
        if (eb) {
          bpw = std::max(1, atoi(eb));
          while (bpw > 1 && ks % bpw) bpw >>= 1;
        } else {
          while (ks % (2 * bpw) == 0 && (long)ntm * ntn * zdim * ks / (2 * bpw) >= 256) bpw *= 2;
        }
      }
      // the register slab layout on 256 x 128 tiles (X3_KREG), row-major slabs (one block per workgroup) otherwise;
      // DAMC_X3_KSLAB_REG=0, read per call, forces row-major
      const char* er = getenv("DAMC_X3_KSLAB_REG");
      a.kslab_reg = (!(er && er[0] == '0') && !WIDE && (long)zdim * ks * ntm * ntn * BM * BN <= a.kslab_floats &&
                     (long)bpw * ntm * ntn * BM * BN * 4 < (1L << 31))
                        ? 1 : 0;
      if (!a.kslab_reg) bpw = 1;
      a.kbpw = bpw;
      a.k_per_z = a.K / ks * bpw;
      if constexpr (!WIDE) {
        if (a.kslab_reg)
          hipLaunchKernelGGL((gemm_x3_kernel<EPI, OM, V | X3_KREG>), dim3(ntm * ntn, 1, zdim * ks / bpw), dim3(512), 0,
                             s, a);
      }
      if (!a.kslab_reg)
        hipLaunchKernelGGL((gemm_x3_kernel<EPI, OM, V>), dim3(ntm * ntn, 1, zdim * ks / bpw), dim3(512), 0, s, a);
      if (a.kslab_reg) {  // one wave per 16x16 tile, four per workgroup
        if (EPI == EPI_BIAS_ACT && OM == O_DENSE && a.ksplit_deferred && !a.C3 && !a.sgn) {
          *a.ksplit_deferred = ks;  // the consumer sums the slabs (GemmArgs::ksplit_deferred)
          return 0;
        }
        // a ConvT forward with the fused output-layer projection: the reduce runs the projection too (bitwise the
        // reduce + proj_rows_kernel); DAMC_REDUCE_PROJ=0 (read per call) keeps the two kernels
        const char* erp = getenv("DAMC_REDUCE_PROJ");
        if (OM == O_PHASE && EPI == EPI_BIAS_ACT && a.proj_out && a.N % 16 == 0 && a.N <= 256 &&
            (a.N <= PROJ_CHUNK || a.N % PROJ_CHUNK == 0) && (a.proj_np == 32 || a.proj_np == 64) &&
            !(erp && erp[0] == '0')) {
          a.proj_nostore = nostore0;
          const unsigned nwg = (unsigned)(zdim * ntm * ntn * 4);
          if (a.proj_np == 32)
            hipLaunchKernelGGL((x3_ksplit_reduce_proj_kernel<2>), dim3(nwg), dim3(256), 0, s, a, zdim);
          else
            hipLaunchKernelGGL((x3_ksplit_reduce_proj_kernel<4>), dim3(nwg), dim3(256), 0, s, a, zdim);
          return (int)hipGetLastError();
        }
        const long waves = (long)zdim * ntm * ntn * 128;
        hipLaunchKernelGGL((x3_ksplit_reduce_tile_kernel<EPI, OM>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s,
                           a, zdim);
        return proj_after();
      }
      const long tot = (long)zdim * a.M * (a.N / 8);
      hipLaunchKernelGGL((x3_ksplit_reduce_kernel<EPI, OM>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a,
                         zdim);
      return proj_after();
    }
  }
  a.ksplit = 1;
  a.kbpw = 1;
  a.kslab_reg = 0;
  if constexpr (F32A && OM == O_PHASE) {
    // round 5: the unsplit F32A ConvT forward on the supertile raster (X3_RASTER: each XCD's concurrent workgroups cover
    // <= 8 M tiles x the 4 phases of an N tile, so the phases' overlapping input windows and weight panels are shared
    // in its L2).  Bitwise the default raster; CIFAR B=128 upconv_fwd FETCH 1059 -> 705 MB per launch at the same
    // time (548 vs 551 us; profiles/r05/walk_ab.txt).  DAMC_X3_RASTER=0 (read per call) keeps the default raster
    const char* er = getenv("DAMC_X3_RASTER");
    if (!(er && er[0] == '0')) {
      // the phases folded into a 1-D grid
      hipLaunchKernelGGL((gemm_x3_kernel<EPI, OM, V | X3_RASTER>), dim3(ntm * ntn * zdim, 1, 1), dim3(512), 0, s, a);
      return 0;
    }
  }
  hipLaunchKernelGGL((gemm_x3_kernel<EPI, OM, V>), dim3(ntm * ntn, 1, zdim), dim3(512), 0, s, a);
  return 0;
}

// damc_clock_probe: the buffer O_PHASE limb-engine launches stamp (null: off)
static unsigned long long* g_clk = nullptr;
static int g_clk_n = 0;
static unsigned g_clk_launch = 0;  // DAMC_CLOCK_REGIONS=R (tools): every limb-engine launch stamps region launch % R

// an at-most-128-row GEMM whose K holds >= 8 sign blocks (the encoder's last conv: M = B, N = nemb, K = 16 Cin): the
// 64 x 128 tile split into its sign blocks (row-major slabs, x3_ksplit_reduce_kernel), 4x the workgroups of the
// 128 x 256 layout's split (CIFAR B=128: 16 x 16 = 256 instead of 64); bitwise the same (one slab per sign block)
template <int EPI>
static void launch_x3_narrow_split(const GemmArgs& a0, hipStream_t s) {
  GemmArgs a = a0;
  const int ks = a.K / a.negk;
  a.ksplit = ks;
  a.kbpw = 1;
  a.kslab_reg = 0;
  a.k_per_z = a.negk;
  a.proj_nostore = 0;
  const int ntm = (a.M + 63) / 64, ntn = (a.N + X3_BN - 1) / X3_BN;
  hipLaunchKernelGGL((gemm_x3_kernel<EPI, O_DENSE, X3_BASE | X3_NARROW>), dim3(ntm * ntn, 1, ks), dim3(512), 0, s,
                     a);
  const long tot = (long)a.M * (a.N / 8);
  hipLaunchKernelGGL((x3_ksplit_reduce_kernel<EPI, O_DENSE>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a,
                     1);
}

// the skinny first-layer kernel's row limit: 32.  DAMC_X3_SKINNY_ROWS (read per call) moves it for A/B; at the
// headline's B = 128 the skinny form (8 x N / 64 workgroups, bitwise the same) took 81.8 us against 30.4 us for the
// 128 x 256 layout (profiles/r05/skinny128_ab.txt)
static int x3_skinny_max_rows() {
  const char* e = getenv("DAMC_X3_SKINNY_ROWS");
  return e ? atoi(e) : 32;
}

// limb-engine dispatch (A3 / B3 set, A_CONV geometry as the K-major engine); splits the batch so every
// launch's gathered x3 tensor stays below 2^31 bytes
int launch_gemm_x3(const GemmArgs& a, Epi epi, OMode om, int zdim, hipStream_t s) {
  const int taps = a.Cg > 0 ? a.K / a.Cg : 0;
  if (!(a.a_f32 ? a.A != nullptr : a.A3 != nullptr) || !a.B3 || a.Cg % X3_BK != 0 || taps * a.Cg != a.K || a.kw <= 0 ||
      taps % a.kw != 0 || taps > 32)
    return DAMC_ERR_ARG;
  if ((om == O_PHASE) != (zdim == 4) || (om == O_DENSE && zdim != 1)) return DAMC_ERR_ARG;
  // the 4 x 4 conv walk (GemmArgs::kwalk): O_DENSE, 16 taps of whole 32-channel slices, the default / F32A tiles only
  if (a.kwalk && (!(om == O_DENSE && taps == 16 && a.kw == 4) && !(om == O_PHASE && taps == 4 && a.kw == 2)))
    return DAMC_ERR_ARG;
  if (a.kwalk && a.Cg % 32 != 0) return DAMC_ERR_ARG;
  if (((uintptr_t)a.A3 | (uintptr_t)a.A | (uintptr_t)a.B3 | (uintptr_t)a.C | (uintptr_t)a.C3 | (uintptr_t)a.mask) % 16 !=
      0)
    return DAMC_ERR_ARG;
  if (!a.C && !a.C3) return DAMC_ERR_ARG;
  if (epi == EPI_MASK && !a.mask && !a.mask_sgn) return DAMC_ERR_ARG;
  if (a.mask_sgn && a.mask_act != DAMC_ACT_LRELU) return DAMC_ERR_ARG;
  // octet epilogue: 8 consecutive channels per thread, 16-B aligned rows and bias
  if (a.N % 8 != 0 || a.ldc % 8 != 0 || (a.bias && ((uintptr_t)a.bias % 16 != 0 || a.bias_mod % 8 != 0)))
    return DAMC_ERR_UNSUPPORTED;
  if ((double)a.N * a.K * 6 >= 2147483647.0) return DAMC_ERR_UNSUPPORTED;
  const long hwq = (long)a.Hq * a.Wq;
  if (a.M % hwq != 0) return DAMC_ERR_ARG;
  const long img = (long)a.Hin * a.Win * a.Cg;  // elements per gathered image
  const long nimg = a.M / hwq;
  static const long lim = [] {
    const char* e = getenv("DAMC_KM_CHUNK_BYTES");
    const long v = e ? atol(e) : 0;
    return (v > 0 && v < 2147483647L) ? v : 2147483647L;
  }();
  const long per = (lim / 6 - 1) / img;
  if (per < 1) return DAMC_ERR_UNSUPPORTED;
  const long cimg = (om == O_PHASE) ? (long)a.Hout * a.Wout * a.ldc : hwq * a.ldc;
  if (a.ksplit_deferred) *a.ksplit_deferred = 0;
  for (long b0 = 0; b0 < nimg; b0 += per) {
    const long nb = std::min(per, nimg - b0);
    GemmArgs c = a;
    if (nimg > per) c.ksplit_deferred = nullptr;  // one launch's slabs only
    static const int regions = [] {
      const char* e = getenv("DAMC_CLOCK_REGIONS");
      return e ? std::max(1, atoi(e)) : 1;
    }();
    if (g_clk && (om == O_PHASE || regions > 1)) {
      const int per_region = g_clk_n / regions;
      c.clk = g_clk + 4L * per_region * (g_clk_launch++ % regions);
      c.clk_n = per_region;
    }
    if (a.A3) c.A3 = a.A3 + b0 * img * 3;
    if (a.a_f32) c.A = a.A + b0 * img;
    if (a.in_part) c.in_part = a.in_part + b0 * hwq / (a.in_hw > 0 ? a.in_hw : 1) * (long)a.N * a.in_S * 3;
    if (a.C) c.C = a.C + b0 * cimg;
    if (a.C3) c.C3 = a.C3 + b0 * cimg * 3;
    if (a.sgn) c.sgn = a.sgn + b0 * cimg / 8;
    if (a.mask_sgn) c.mask_sgn = a.mask_sgn + b0 * cimg / 8;
    if (a.mask) c.mask = a.mask + b0 * cimg;
    c.M = (int)(nb * hwq);
    if (a.proj_out) {  // the fused output-layer projection (GemmArgs::proj_out, 128-channel chunks)
      if (om != O_PHASE || epi != EPI_BIAS_ACT || a.N > 256 || a.N % 16 || !a.C || !a.proj_w ||
          (a.proj_np != 32 && a.proj_np != 64) || (a.N > PROJ_CHUNK && a.proj_pstride <= 0))
        return DAMC_ERR_ARG;
      c.proj_out = a.proj_out + b0 * (long)a.Hout * a.Wout * a.proj_np;
      if (c.a_f32) {  // the F32A tile: each 128-channel N tile projects its chunk
        if (a.N > PROJ_CHUNK && a.N % PROJ_CHUNK) return DAMC_ERR_UNSUPPORTED;
        if (const int rc_ = launch_x3_t<EPI_BIAS_ACT, O_PHASE, X3_BASE | X3_F32A>(c, zdim, s)) return rc_;
      } else {  // the 128 x 256 layout: one N tile holding every channel
        if (const int rc_ = launch_x3_t<EPI_BIAS_ACT, O_PHASE, X3_BASE | X3_WIDE>(c, zdim, s)) return rc_;
      }
      continue;
    }
    // at most 128 rows (the first layer, M = B <= 128): the 128 x 256 block layout, no half-empty 256-row tile
    // (bitwise the default layout: every output takes the same MFMA sequence; 46.6 -> 35.7 us for CIFAR's B = 128
    // first layer, tools/gemm_bench.hip).  DAMC_X3_WIDE=0 (read per call) keeps the default layout
    const char* ew = getenv("DAMC_X3_WIDE");
    // the first layer at per-rank batches: the skinny kernel (bitwise the 128 x 256 layout); DAMC_X3_SKINNY=0 (read
    // per call) keeps the tiled kernel
    const char* esk = getenv("DAMC_X3_SKINNY");
    if (epi == EPI_BIAS_ACT && om == O_DENSE && !c.kwalk && c.M <= x3_skinny_max_rows() && c.K <= c.negk && c.Hin == 1 &&
        c.Win == 1 &&
        c.kw == 1 && c.Cg == c.K && c.A3 && !c.a_f32 && !c.proj_out && !(esk && esk[0] == '0')) {
      // fp32 weights split in registers where the caller passes them (2/3 of the limb bytes; bitwise the same
      // operands); DAMC_X3_SKINNY_F32B=0 (read per call) reads the limbs
      const char* efb = getenv("DAMC_X3_SKINNY_F32B");
      if (c.in_part && c.in_done) *c.in_done = 0;  // no norm statistics from this kernel
      const dim3 gsk((unsigned)((c.N + 63) / 64), (unsigned)((c.M + 15) / 16));
      // 32 columns per wave by default (NTW = 2: CIFAR B=16 step -5 to -17 us, B=32 -4 us against 16 columns, same-box
      // pairs in profiles/r05/skinny_ntw_ab.txt); DAMC_X3_SKINNY_NTW=1 (read per call) keeps 16
      const char* ent = getenv("DAMC_X3_SKINNY_NTW");
      if (!(ent && ent[0] == '1') && c.b32k && (c.K % 32) == 0 && (uintptr_t)c.b32k % 16 == 0 && !(efb && efb[0] == '0'))
        hipLaunchKernelGGL((x3_skinny_kernel<true, 2>), dim3((unsigned)((c.N + 127) / 128), gsk.y), dim3(256), 0, s, c);
      else if (c.b32k && (c.K % 32) == 0 && (uintptr_t)c.b32k % 16 == 0 && !(efb && efb[0] == '0'))
        hipLaunchKernelGGL((x3_skinny_kernel<true, 1>), gsk, dim3(256), 0, s, c);
      else
        hipLaunchKernelGGL((x3_skinny_kernel<false, 1>), gsk, dim3(256), 0, s, c);
      continue;
    }
    const char* ens = getenv("DAMC_X3_NARROW_SPLIT");  // (read per call) 0: the 128 x 256 layout below
    if (epi == EPI_BIAS_ACT && om == O_DENSE && c.M <= 128 && !c.a_f32 && !c.proj_out && c.kslab && !c.kwalk &&
        c.K % c.negk == 0 && c.K / c.negk >= 8 && c.N % 8 == 0 && (long)(c.K / c.negk) * c.M * c.N <= c.kslab_floats &&
        !(ens && ens[0] == '0')) {
      if (c.in_part && c.in_done) *c.in_done = 0;  // no norm statistics from this kernel
      launch_x3_narrow_split<EPI_BIAS_ACT>(c, s);
      continue;
    }
    if (epi == EPI_BIAS_ACT && om == O_DENSE && c.M <= 128 && !c.a_f32) {
      if (!(ew && ew[0] == '0')) {
        if (const int rc_ = launch_x3_t<EPI_BIAS_ACT, O_DENSE, X3_BASE | X3_WIDE>(c, zdim, s)) return rc_;
        continue;
      }
    }
    if (ew && ew[0] == '2' && !c.a_f32) {  // A/B only: every limb GEMM on the 128 x 256 layout (bitwise the default)
      if (epi == EPI_BIAS_ACT && om == O_PHASE) {
        if (const int rc_ = launch_x3_t<EPI_BIAS_ACT, O_PHASE, X3_BASE | X3_WIDE>(c, zdim, s)) return rc_;
        continue;
      }
      if (epi == EPI_MASK && om == O_DENSE) {
        if (const int rc_ = launch_x3_t<EPI_MASK, O_DENSE, X3_BASE | X3_WIDE>(c, zdim, s)) return rc_;
        continue;
      }
    }
#define DAMC_X3(E_, O_)                                                      \
  if (epi == E_ && om == O_) {                                               \
    const int rc_ = c.a_f32 ? launch_x3_t<E_, O_, X3_BASE | X3_F32A>(c, zdim, s) \
                            : launch_x3_t<E_, O_>(c, zdim, s);               \
    if (rc_) return rc_;                                                     \
    continue;                                                                \
  }
    DAMC_X3(EPI_BIAS_ACT, O_PHASE)
    DAMC_X3(EPI_MASK, O_DENSE)
    DAMC_X3(EPI_BIAS_ACT, O_DENSE)
    DAMC_X3(EPI_STORE, O_DENSE)
#undef DAMC_X3
    return DAMC_ERR_UNSUPPORTED;
  }
  return (int)hipGetLastError();
}

// O_WGRAD: A3 [Cg][K] and B3 [wg_phases][N][K] pixel-major x3 operands, C = fp32 slabs
// [wg_phases * slices][M][ldc] (EPI_STORE); slice length k_per_z (a multiple of 32)
int launch_wgrad_x3(const GemmArgs& a, int slices, const char* prof_name, double flops, hipStream_t s) {
  if (!a.A3 || !a.B3 || !a.C || a.C3 || a.sgn || a.M <= 0 || a.N <= 0 || a.K <= 0 || slices < 1) return DAMC_ERR_ARG;
  if (a.wg_phases != 1 && a.wg_phases != 4) return DAMC_ERR_ARG;
  if (a.wg_bp <= 0 || a.wg_bp % X3_BK != 0 || a.K % a.wg_bp != 0 || a.K / a.wg_bp != a.Hin * a.Win)
    return DAMC_ERR_ARG;
  if (a.k_per_z <= 0 || a.k_per_z % X3_BK != 0 || (long)a.k_per_z * slices < a.K) return DAMC_ERR_ARG;
  if (a.kw < 1 || a.kw > 2 || a.M != a.kw * a.kw * a.Cg || (a.wg_phases == 1 && a.kw != 1)) return DAMC_ERR_ARG;
  if (a.N % 8 != 0 || a.ldc % 8 != 0 || a.ldc < a.N || a.c_zstride < (long)a.M * a.ldc) return DAMC_ERR_ARG;
  if (((uintptr_t)a.A3 | (uintptr_t)a.B3 | (uintptr_t)a.C) % 16 != 0) return DAMC_ERR_ARG;
  if ((double)a.Cg * a.K * 6 >= 2147483647.0 || (double)a.N * a.K * 6 >= 2147483647.0) return DAMC_ERR_UNSUPPORTED;
  const int ntm = (a.M + X3_BM - 1) / X3_BM, ntn = (a.N + X3_BN - 1) / X3_BN;
  ProfScope ps(prof_name, flops, s);
  hipLaunchKernelGGL((gemm_x3_kernel<EPI_STORE, O_WGRAD, X3_BASE>),dim3(ntm * ntn, 1, a.wg_phases * slices), dim3(512), 0, s,
                     a);
  return (int)hipGetLastError();
}

void set_clock_probe(unsigned long long* buf, int n) {
  g_clk = (buf && n > 0) ? buf : nullptr;
  g_clk_n = g_clk ? n : 0;
  g_clk_launch = 0;
}

}  // namespace damc

#ifndef DAMC_GEMM_NO_C_API
extern "C" int damc_clock_probe(unsigned long long* buf, int n_slots) {
  damc::set_clock_probe(buf, n_slots);
  return 0;
}

extern "C" unsigned long long damc_x3_tapshare_launches(void) {
  return damc::g_tapshare_launches.load(std::memory_order_relaxed);
}
#endif
