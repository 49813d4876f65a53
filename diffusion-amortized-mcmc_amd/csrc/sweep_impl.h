// sweep_impl.h — what more than one of the reverse sweep's files shares: the chain tile's constants, the per-call
// record, the in0 embedding's zB product, the sc1 loads, the team launch's arguments, the workspace layout and the
// per-call stages as structs, and the host functions that cross files.  Included only by denoiser.hip,
// sweep_chain.hip, sweep_team.hip, sweep_finish.hip and sweep_stages.hip; everything else goes through
// include/damc.h.  It defines no variable and no function that is not inline.
#pragma once
#include "gemm.h"

namespace damc {

// ---- the chain tile (chain_kernel, the team kernels and the skinny GEMM all compute it)
#ifndef DAMC_CH_WAVES
#define DAMC_CH_WAVES 4
#endif
constexpr int CH_WAVES = DAMC_CH_WAVES;  // waves per chain workgroup, splitting K
constexpr int CH_THREADS = 64 * CH_WAVES;
constexpr int TM = 16;           // rows per workgroup
constexpr int TC = 8;            // output columns per workgroup (x 2 products)
constexpr int KG = 16 * CH_WAVES;  // K padding granule: one 16-deep k-group per wave
#ifndef DAMC_CH_CHUNK
#define DAMC_CH_CHUNK 4  // 8 until round 4: with the sentinel re-read paths the team kernel at 8 ran 3.92 ms per B=128
                         // sweep against 3.49 at 4 (same box, interleaved; profiles/r04/sweep_ab.txt)
#endif
constexpr int CH_CHUNK = DAMC_CH_CHUNK;  // k-groups whose loads a lane keeps in flight at once
constexpr int EMB_G = 8;         // in0: 16-deep k-groups of z (nz <= 128)

// per-call values read by the last block (device memory in the workspace, written before each sweep so a cached
// graph needs no new kernel arguments)
struct SweepCall {
  const float* noise;  // injected (n-1, B, nz) or null (Philox)
  float* eps_log;      // (eps_log_steps, B, nz) or null
  uint64_t seed, chain_base, step_offset;
  int with_noise, eps_log_steps;
};

__host__ __device__ inline int kpad(int din) { return (din + KG - 1) / KG * KG; }
__host__ __device__ inline int emb_ld(int kp) { return kp + 8; }  // in0 LDS image row stride (floats)

// in0's z B (16 rows x the wave's 16 columns, K = nz <= 128) as two independent MFMA chains over the even and the odd
// k-groups, then their sum: half the dependent-MFMA latency of one chain on the stage's critical path (chain_kernel, the team
// kernel and its rescue all use this function)
__device__ __forceinline__ f32x4 emb_zb(const f32x4 (&zv4)[EMB_G], const f32x4 (&bv)[EMB_G]) {
#ifdef DAMC_EMB_ONE_CHAIN  // A/B only (round 4 sweep attribution): round 2's single chain
  f32x4 a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < EMB_G; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(zv4[g][e], bv[g][e], a1, 0, 0, 0);
  return a1;
#endif
  f32x4 e0 = {0.f, 0.f, 0.f, 0.f}, e1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < EMB_G; g += 2)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(zv4[g][e], bv[g][e], e0, 0, 0, 0);
      e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(zv4[g + 1][e], bv[g + 1][e], e1, 0, 0, 0);
    }
  return e0 + e1;
}

// sc1 (L1-bypassing) loads of handed-off words (MI355X_MICROARCH.md, inter-workgroup visibility): the team kernels
// and their rescue
__device__ __forceinline__ f32x4 ld_sc1(const __amdgpu_buffer_rsrc_t& r, long byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 16));
}
__device__ __forceinline__ float ld_sc1_f(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the team launch's arguments (sweep_team.hip fills and launches them; denoiser.hip holds them between the
// plan, the launch and the finish)
struct TsBlock {
  const float* w;    // packed [ntn][16][kp] (workspace)
  const float* bls;  // [ntn][16]
  int kp, dout, ntn;
  int wa, wb;        // widths of the input halves (in0: wa = din, the embedding; wb = 0: no skip half)
  int kpa, kpb;      // their K paddings (multiples of 64)
  int srcA, srcB;    // producing blocks of the halves (-1: none)
  long ooff;         // output (B, dout) within a step's ring slot, floats
  int ghoff;         // 2 * coloff: gate columns in a gh row
  int toff;          // column tile tn -> slot (tn + toff) % T
};

struct TsArgs {
  TsBlock b[7];
  const float* bmat;  // B^T (nz/2, nz)
  int nz, B, G, n, residual, T;
  const float* gh;    // (n, B, 2S)
  long ldgh;
  float* ring;        // (n, B*S): block outputs of step k at ring + k * ring_step
  long ring_step;
  float* zring;       // (n+1, B, nz): z before step k at zring + k * B * nz
  const float* tab;   // (n, 8): c0..c4, is_last, noisy_k
  const SweepCall* call;
  int* err;           // the error word: set by a wait that gave up (or DAMC_SWEEP_FORCE_FAIL), read by team_finish_kernel
  long budget;        // wait budget in 100 MHz ticks
  int wlds;           // weight LDS floats per workgroup (host maximum over slots)
  int fast;           // 128 / 100: sweep_fast_kernel<fast, 128> (the shapes compiled in; DAMC_SWEEP_FAST=0: off)
  uint64_t* trace;    // tools only (DAMC_SWEEP_TRACE): [P][7n][4] 100 MHz stamps {task start, wake (the
                      // previous block's half is read from here on), reduced, published (the stage's stores issued)}
  int dbg;            // timing experiments only (DAMC_SWEEP_DBG, wrong results):
                      // 2 no payload loads, 4 no MFMA, 8 no epilogue operand loads, 16 no output stores,
                      // 32 no zB / sin / cos (in0), 64 no z loads (in0); tests: 4096 every workgroup reports a
                      // failed wait at once (exercises the rescue in team_finish_kernel)
};

// ---- workspace layout (denoiser.hip carve)
// a block's columns in the per-(step, row) tables (ctx, gate | hyper bias): its dout, up to a multiple of 4 so every
// block starts float4-aligned (only out2 of a denoiser with nz % 4 != 0 is padded: the row-resident form)
inline int lay_dout(int dout) { return (dout + 3) & ~3; }
inline bool narrow_out2(const damc_denoiser_t* d) { return (d->nz & 3) != 0; }

struct SweepWs {
  float *w[7], *bls[7], *wgb[7], *bg2[7];
  float *wctx_t, *wctx_x, *bctx, *tw1t, *tw2t, *bmat;
  float *px, *qt, *t1, *t2, *xs, *cx, *gh, *z;
  float* outs[7];
  SweepCall* call;
  // team sweep: per-step ring slots of the block outputs and of z, the step table, the error word
  float *ring, *zring, *tab;
  int* err;
  size_t bytes;
};

// ---- the per-call stages, shared by the reverse sweep and the guided sweep
struct Stages {
  const damc_denoiser_t* d;
  SweepWs w;
  hipStream_t s;
  int S, nt, nx;
  int coloff[7];
  // nz % 4 != 0: out2 (dout = nz) is off the float4 paths of stages 2 and 3; they run blocks 0 .. nb - 1 as they run
  // every other denoiser's, and out2's columns come from the narrow kernels of denoiser_rows.hip
  bool narrow;
  int nb;
  // the skinny precompute GEMMs read the time MLP and ctx Linears in their PyTorch layouts: no transposes
  bool skinny;
};

// ---- denoiser.hip
int sum_dout(const damc_denoiser_t* d);  // the lay_dout widths of the 7 blocks, summed: S
// the workspace of a (B, n) sweep carved from base (null: sizes only); returns its bytes
size_t carve(const damc_denoiser_t* d, int B, int n, char* base, SweepWs* w);
// the device copy of a schedule's step table (n, 8), uploaded once per (device, schedule) and kept
int step_table(const float* coef, int n, hipStream_t s, const float** out);

// ---- sweep_stages.hip
bool stages_skinny(const damc_denoiser_t* d);
int hyper_limb_blocks(const damc_denoiser_t* d, int nb, const int* coloff);
void stages_init(Stages& st, const damc_denoiser_t* d, int B, int n, void* wsp, hipStream_t s);
int stage_pack(const Stages& st);
int stage_time(const Stages& st, const float* temb_in, int n);
int stage_px(const Stages& st, const float* xemb, int M, float* xs, float* px);
int launch_ctx(const float* px, long pxstep, const float* qt, int n, int B, int S, float* cx, hipStream_t s);
int stage_hyper(const Stages& st, const float* cx, float* gh, long M);

// ---- sweep_chain.hip: the launch chain of a sweep, 7 n launches of chain_kernel
bool graphs_enabled();  // DAMC_SWEEP_GRAPH (read once)
int run_chain_graph(const damc_denoiser_t* d, const SweepWs& w, void* wsp, size_t wsb, int B, int n, const float* coef,
                    hipStream_t s);
int run_chain_eager(const damc_denoiser_t* d, const SweepWs& w, int B, int n, const float* coef, hipStream_t s);
void chain_trace_dump(hipStream_t s);  // tools only (DAMC_CHAIN_TRACE)

// ---- sweep_team.hip: the team launch
bool sweep_team(const damc_denoiser_t* d, const SweepWs& w, int B, int n, bool capturing, int dev, TsArgs* ta, int* tP,
                size_t* tsm);
int run_chain_team(TsArgs& a, int P, size_t smem, const float* coef, hipStream_t s);
int* team_health_word(int dev, bool capturing);
bool team_healthy(int dev);
long team_failures(int dev);  // rescued team launches on the device so far (damc_sweep_team_failures)

// ---- sweep_finish.hip: team_finish_kernel, the copy-out of the team's result to zt or, after a failed wait, the rescue
void launch_team_finish(const TsArgs& a, float* zt, int* hostflag, hipStream_t s);

}  // namespace damc
