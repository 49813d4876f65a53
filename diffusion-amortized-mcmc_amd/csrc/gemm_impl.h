// gemm_impl.h — what more than one of the GEMM engine files shares: the generic epilogue, the tile rasters, the limb
// engine's constants and swizzles, and the two engine dispatchers launch_gemm calls.  Included only by gemm.hip,
// gemm_km.hip, gemm_x3.hip, x3_pack.hip and tools/gemm_bench.hip; everything else goes through gemm.h.
#pragma once
#include <type_traits>

#include "gemm.h"

namespace damc {

constexpr int BN = 128;  // block tile columns of the generic fp32 and the K-major engine

// ---- epilogue: lane holds col = lane&31, rows (r&3) + 8(r>>2) + 4(lane>>5) of each 32x32 tile
// output row offset of GEMM row m (O_PHASE: pixel (b, 2qy+py, 2qx+px) of the Hout x Wout map)
template <int OM>
__device__ __forceinline__ long gemm_row_offset(const GemmArgs& p, int m, int py, int px) {
  if (OM == O_PHASE) {
    const int hwq = p.Hq * p.Wq;
    const int b = m / hwq;
    const int rr = m - b * hwq;
    const int qy = rr / p.Wq, qx = rr - qy * p.Wq;
    return (((long)b * p.Hout + 2 * qy + py) * p.Wout + 2 * qx + px) * p.ldc;
  }
  return (long)m * p.ldc;
}

// one output element: epilogue arithmetic + store (idx = row offset + n)
template <int EPI>
__device__ __forceinline__ void epi_element(const GemmArgs& p, float* Cz, long idx, int n, bool bias_wrap, float v) {
  if (EPI == EPI_BIAS_ACT) {
    if (p.bias) v += p.bias[bias_wrap ? n % p.bias_mod : n];
    v = act_apply(v, p.act, p.slope);
  } else if (EPI == EPI_MASK) {
    v *= act_grad_from_out(p.mask[idx], p.mask_act, p.mask_slope);
  } else if (EPI == EPI_GATE) {
    if (p.bias) v += p.bias[n];
    if (n < p.gate_cols) v = 1.f / (1.f + expf(-v));
  } else if (EPI == EPI_RESID) {
    if (p.bias) v += p.bias[n % p.bias_mod];
    const float t = act_apply(v, p.act, p.slope);
    if (p.xhat) p.xhat[idx] = t;
    const float res = t - p.xres[idx];
    if (p.sqerr) atomicAdd(p.sqerr, 0.5f * p.inv_s2 * res * res);
    v = res * p.inv_s2 * act_grad_from_out(t, p.act, p.slope);
  }
  Cz[idx] = v;
}

// rowtab: optional per-block table of gemm_row_offset for rows m0 .. m0 + 32*MT*2 - 1
template <int EPI, int OM, int MT>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& p, f32x16 (&acc)[MT][2], int m0, int n0, int wm,
                                              int wn, int lane, int z, int py, int px,
                                              const long* rowtab = nullptr) {
  const int lrow = lane & 31;
  float* Cz = p.C;
  if (OM == O_DENSE) Cz += (long)z * p.c_zstride;
  const bool bias_wrap = p.bias_mod < p.N;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ml = wm * (32 * MT) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const int m = m0 + ml;
      if (m >= p.M) continue;
      const long rowoff = rowtab ? rowtab[ml] : gemm_row_offset<OM>(p, m, py, px);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + lrow;
        if (n >= p.N) continue;
        epi_element<EPI>(p, Cz, rowoff + n, n, bias_wrap, acc[i][j][r]);
      }
    }
  }
}

// the same for a wave's 4 x 4 grid of 16x16 accumulators (col = lane&15, row = 4(lane>>4) + r)
template <int EPI, int OM>
__device__ __forceinline__ void gemm_epilogue16(const GemmArgs& p, f32x4 (&acc)[4][4], int m0, int n0, int wm, int wn,
                                                int lane, int z, int py, int px, const long* rowtab) {
  float* Cz = p.C;
  if (OM == O_DENSE) Cz += (long)z * p.c_zstride;
  const bool bias_wrap = p.bias_mod < p.N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ml = wm * 64 + i * 16 + 4 * (lane >> 4) + r;
      const int m = m0 + ml;
      if (m >= p.M) continue;
      const long rowoff = rowtab ? rowtab[ml] : gemm_row_offset<OM>(p, m, py, px);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + (lane & 15);
        if (n >= p.N) continue;
        epi_element<EPI>(p, Cz, rowoff + n, n, bias_wrap, acc[i][j][r]);
      }
    }
  }
}

// XCD-aware bijective remap: consecutive work-group ids land on one XCD (dispatch is round-robin over 8)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// supertile raster: linear id l in [0, T * P) -> (M tile tm, pair p), blocks of SM x SP ids (SP = min(4, P) pairs
// fastest, then SM = 32 / SP M tiles), blocks ordered M-major; edge blocks are smaller.  Bijective.
__device__ __forceinline__ void supertile(int l, int T, int P, int& tm, int& p) {
  const int SP = P < 4 ? P : 4;
  const int SMf = 32 / SP;
  const int SM = T < SMf ? T : SMf;
  const int rowsz = SM * P;              // ids of one full block row (SM M tiles, all pairs)
  const int tmb = l / rowsz;
  const int sm = min(SM, T - tmb * SM);  // M tiles in this block row (smaller on the last)
  int rem = l - tmb * rowsz;
  const int pb = rem / (sm * SP);        // full pair blocks come first; the last may be narrower
  const int sp = min(SP, P - pb * SP);
  rem -= pb * sm * SP;
  tm = tmb * SM + rem / sp;
  p = pb * SP + rem % sp;
}

// the K-major and the limb engine push a padding tap's buffer offset here
constexpr unsigned KM_OOB = 0xF0000000u;  // any offset >= the descriptor size reads as zero

// ---- limb engine (gemm_x3.hip has the engine's description): tile shape, LDS row bytes, swizzles, variant bits
constexpr int X3_BM = 256, X3_BN = 128, X3_BK = 32, X3_ROWB = 192;
__device__ __forceinline__ int x3_swz(int row) { return (row >> 1) & 3; }
// F32A (variant bit 2097152): the A operand staged as fp32, one 128-B row of 8 16-B chunks per K tile, physical chunk
// = logical chunk ^ f32a_swz(row & 15).  A lane of a 16x16x32 fragment read (row lane & 15, octet q = lane >> 4)
// takes logical chunks 2q and 2q + 1 in two ds_read_b128; with u = (r >> 1) & 7 and the bit-1 flip on rows 4-11
// (the rows the b128 lane groups pair with the other octet) every 16-lane group hits 16 distinct 4-bank groups.
constexpr int X3_F32A = 2097152, X3A_ROWB = 128;
// X3_NARROW (variant bit 4194304): a 64 x 128 block tile, 8 waves 2 (M) x 4 (N) of 32 x 32 (2 x 2 MFMA tiles each),
// 74 KB of LDS so two workgroups share a CU: a small-batch conv fills the chip without split-K slabs (every output
// takes the default tile's MFMA sequence, so it is bitwise the default and the split forms)
constexpr int X3_NARROW = 4194304;
// X3_TAPSHARE (round 7; F32A with the slice-major walk GemmArgs::kwalk, an Hq x Wq grid that x3_tapshare_ok accepts):
// the four K tiles of a group (one 32-channel slice x the four taps of a ConvT phase, or of a parity class of the
// stride-2 4 x 4 conv) read the same 256 input pixels displaced by 0 / +-1 grid positions, so the undisplaced 256 x
// 128-B fp32 image is staged once per group (8 KB instead of 32 KB of A per K tile) and, since round 9, split into its
// limbs once, into an LDS limb image; each tap's fragment reads take limb-image row r + delta(tap), or an all-zero row
// where the tap falls in the padding: the same limbs of the same fp32 operands, bitwise the per-tap staging.  Since
// round 11 the loop runs on the 4 (M) x 2 (N) wave grid of the limb-A base loop: no wave splits anything in registers
// any more, and a B fragment feeds four A tiles instead of two (24 instead of 30 ds_read_b128 per wave and K tile).
// (Rounds 7-8 under this value: the taps read the fp32 image and each ran the split in registers; rounds 9-10: the
// limb image on the per-tap loop's 8 x 1 waves.)
constexpr int X3_TAPSHARE = 16777216;
__device__ __forceinline__ int f32a_swz(int r) { return ((r >> 1) & 7) ^ ((((r >> 2) ^ (r >> 3)) & 1) << 1); }
// the swizzle of the X3_TAPSHARE fp32 staging image.  Chosen in round 7, when the taps read it at rows r + delta: the
// 16 rows of a ds_read_b128 lane group then arrive rotated by any delta mod 16, where f32a_swz is 2-way for every
// rotation but 0 and 8.  With row bit 1 -> chunk bit 0 and row bit 2 -> chunk bit 2 (the bank group of a 16-B chunk is
// 8 (row & 1) + chunk) every rotation of every lane group hits 16 distinct bank groups; the conversion reads it
// undisplaced
__device__ __forceinline__ int ts_swz(int r) { return ((r >> 1) & 1) | (((r >> 2) & 1) << 2); }
static_assert(X3_NEGK % 32 == 0 && (X3_NEGK & (X3_NEGK - 1)) == 0, "sign blocks are whole K tiles, a power of two");
constexpr int X3_CHUNKS = 12;  // 16-B chunks per row and K tile (4 octets x 3 limbs)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int N>
using x3_ic = std::integral_constant<int, N>;

// V, gemm_x3_kernel's variant bits.  The value is part of the kernel's name, which committed profiles and the tools
// match on, so the bits keep their values.  (The retired experiment bits and what they measured: DESIGN.md.)
//   X3_BASE      in every instantiation: v_mfma_f32_16x16x32_bf16 on 16x16 tiles (1); LDS-DMA staging (4: buffer_load
//                ... lds straight into the lane-linear LDS image, one K tile ahead, no staging registers or ds_write);
//                fragment reads in MFMA order (256).  Measured best, profiles/r02/gemm_bench_rdorder.txt
//   X3_RASTER    supertile raster (not O_WGRAD): a 1-D grid; each XCD's 32 concurrent workgroups form a block of <= 8
//                M tiles x 4 (N tile, phase) pairs with the 4 phases of an N tile adjacent, so the phases' overlapping
//                input windows and the weight panels are shared in L2 instead of every XCD streaming all phases' panels
//   X3_WIDE      a 128 x 256 block tile (waves 2 along M x 4 along N, each still 64 x 64) instead of 256 x 128: no
//                half-empty tile at M = 128 (the first layer, M = B) and half the A gather per K tile
//   X3_KREG      split-K into register-layout slabs (GemmArgs::kslab_reg; launched only split, 256 x 128 tiles): a
//                compile-time variant, so the block-total registers of the unsplit kernel drop out
//   X3_F32A, X3_NARROW, X3_TAPSHARE: above
constexpr int X3_BASE = 261, X3_RASTER = 16, X3_WIDE = 524288, X3_KREG = 1048576;
constexpr int X3_BITS = X3_BASE | X3_RASTER | X3_WIDE | X3_KREG | X3_F32A | X3_NARROW | X3_TAPSHARE;
// RNE limb split of 8 consecutive values: v = h + m + l (to 24 significand bits); gemm.h store_x3_octet is the same
// split for the callers outside the engine files
__device__ __forceinline__ void split3_octet(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 b0 = (__bf16)v[e];
    const float r1 = sub_rn(v[e], (float)b0);
    const __bf16 b1 = (__bf16)r1;
    const float r2 = sub_rn(r1, (float)b1);
    h[e] = b0;
    m[e] = b1;
    l[e] = (__bf16)r2;
  }
}

// the engines behind launch_gemm (gemm.hip): the K-major convolution engine (gemm_km.hip) and the limb engine
// (gemm_x3.hip); both split the batch so every launch's gathered tensor stays below 2^31 bytes
int launch_gemm_km(const GemmArgs& a, Epi epi, OMode om, int zdim, hipStream_t s);
int launch_gemm_x3(const GemmArgs& a, Epi epi, OMode om, int zdim, hipStream_t s);

}  // namespace damc

