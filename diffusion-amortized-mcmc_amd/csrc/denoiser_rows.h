// denoiser_rows.h — the row-resident reverse sweep (denoiser_rows.hip) as denoiser.hip and sweep_stages.hip call it.
#pragma once
#include "common.h"

namespace damc {

constexpr int ROWS_TM = 16;                  // rows per workgroup (the MFMA's M)
constexpr int ROWS_GTM = 8;                  // latent rows per workgroup of the guided sweep: each twice in the 16
constexpr size_t ROWS_LDS_MAX = 156 * 1024;  // dynamic LDS of one workgroup (the CU has 160 KB)

struct RowsBlock {
  const float* w;    // packed [ntn][16][kp]: rows 0-7 Wl, 8-15 Ws of the tile's 8 columns (pack_denoiser_kernel)
  const float* bls;  // [ntn][16]: bl, bs
  int din, kp, dout, ntn;
  int ghoff;         // gate columns of the block in a gh row (hyper bias dout further)
  int src, dst;      // float offsets of the block's input and output within a row's LDS image
};

struct RowsArgs {
  RowsBlock b[7];
  const float* bmat;  // B^T (nz / 2, nz)
  int nz, B, n, residual;
  int ld;             // floats per row of the LDS image
  const float* gh;    // (n, B, ldgh)
  long ldgh;
  const float* tab;   // (n, 8): c0..c4, is_last, noisy_k
  float* zt;          // (B, nz), updated in place
  const float* noise; // injected (n - 1, B, nz) or null (Philox)
  float* eps_log;     // (eps_log_steps, B, nz) or null
  uint64_t seed, chain_base, step_offset;
  const damc_draw_state_t* draws;  // damc_reverse_sweep_ds: the device-resident key (common.h draw_key), or null
  int with_noise, eps_log_steps;
  // guided sweep only (launch_sweep_rows_guided): the unconditional planes, and the guidance weights 1 + w and w
  const float* gh_u;  // (n, B, ldgh)
  float gw1, gw;
};

// floats per row of the LDS image of a denoiser of width w (= in0's dout) and in0 padding kp0; fills the blocks' src / dst
int rows_layout(int nz, int w, int kp0, RowsBlock* b);
// one launch: ceil(B / 16) workgroups, each running all n steps x 7 blocks of its rows
int launch_sweep_rows(const RowsArgs& a, hipStream_t s);
// the guided (classifier-free guidance) sweep, one launch: ceil(B / 8) workgroups, each running all n steps x 7 blocks
// of its 8 latent rows twice over, image rows 0-7 on the gates of a.gh (conditional) and 8-15 on those of a.gh_u
// (unconditional); the two eps of a latent row meet in the last block's epilogue as (1 + w) eps_c - w eps_u and both
// twins take the same reverse step.  noise, eps_log and the Philox chain index are per latent row.
int launch_sweep_rows_guided(const RowsArgs& a, hipStream_t s);

// out2 of a denoiser whose nz is no multiple of 4: its columns of the per-call stages, off the float4 GEMM paths.
// Y[m][c] = bias[c] + sum_k f(A[m][k]) W[c][k] for c < N (f = SiLU when silu_a), 0 for N <= c < npad
int launch_narrow_linear(const float* A, long lda, int M, int K, int silu_a, const float* W, long ldw, const float* bias,
                         int N, int npad, float* Y, long ldy, hipStream_t s);
// [gate | hyper bias] = [sigmoid(c Wg^T + bg) | c Wb^T] of M rows, K = N = dout, with the exact sigmoid
int launch_narrow_hyper(const float* cx, long ldc, long M, int dout, const float* wg, const float* bg, const float* wb,
                        float* gh, long ldgh, hipStream_t s);

}  // namespace damc
