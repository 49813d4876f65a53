// denoiser.hip — Diffusion_UnetA eps-prediction and the amortizer's latent reverse sweep
// (_netQ_U.forward, workspace/src/diffusion_net.py:585-622) on gfx950: workspace layout, validation, the dispatch
// among the sweep's forms and the C entry points.
//
// A ConcatSquash block (diffusion_net.py:417-445) is
//     out = (x Wl^T + bl) * sigmoid(c Wg^T + bg) + c Wb^T + (x Ws^T + bs),   c = SiLU(Lc(SiLU(cat(temb, xemb))))
// and its ctx c depends on (step, row) only — never on zt.  So a sweep first runs the per-call stages (pack, ctx,
// hyper: sweep_stages.hip), which take 51 % + 20 % of the reference's per-step MACs (ctx Linear, hyper Linears) out
// of the dependent chain, and then the chain itself: x Wl^T and x Ws^T of the 7 blocks plus the reverse-step update,
// n steps in a row.  The chain has five forms, all rounding alike:
//   1. row-resident (denoiser_rows.hip): one launch, a workgroup runs every step and block of its 16 rows in LDS;
//      the only form for nz % 4 != 0, and DAMC_SWEEP_ROWS=1 asks for it;
//   2. team, generic (sweep_team_kernel): one launch, one workgroup per CU, the chain's weights resident in LDS;
//   3. team, shapes compiled in (sweep_fast_kernel<NZ, W>): the default at w = 128 and nz = 128 or 100;
//   4. launch chain (chain_kernel, 7 n launches replayed from a cached HIP graph): DAMC_SWEEP_TEAM=0, weights that
//      do not fit a team's LDS, or a process whose team launch has needed its rescue (team_finish_kernel) once;
//   5. guided (denoiser_rows.hip, twin rows): classifier-free guidance, always row-resident (damc_guided_sweep).
// reverse_sweep_impl chooses among 1-4 by sweep_rows and sweep_team; damc_sweep_form reports the same choice without
// launching anything, damc_sweep_stages the engines the per-call stages take.
//
// Which file holds what:
//   sweep_impl.h      what the files below share: constants, SweepCall, TsArgs, SweepWs, Stages, declarations
//   sweep_stages.hip  stage_pack / stage_time / stage_px / launch_ctx / stage_hyper and their kernels
//   sweep_team.hip    forms 2 and 3: sweep_team_kernel, sweep_fast_kernel, team_plan, run_chain_team, the health word
//   sweep_finish.hip  team_finish_kernel: the team launch's copy-out and rescue
//   sweep_chain.hip   form 4: chain_kernel, the Launch list, the graph cache, the chain trace
//   denoiser_rows.hip forms 1 and 5, and the narrow out2 kernels of the stages
//   denoiser.hip      sweep_setup_kernel, copy_kernel, carve, validate, the step table, reverse_sweep_impl, the guided
//                     sweep's host side, every extern "C" entry point
// Process-wide host state defined here: the step-table cache with its mutex.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "denoiser_rows.h"
#include "sweep_impl.h"

using namespace damc;

namespace {

// the call's per-call record and z, and (team launch) the error word zeroed: a kernel in
// the stream, not a memset node, so a captured sweep orders it like every other kernel
__global__ void sweep_setup_kernel(SweepCall c, SweepCall* dst, const float* zt, float* zw, long n, unsigned* zero,
                                   long nzero, f32x4* s1, long ns1, f32x4* s2, long ns2, const damc_draw_state_t* ds) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    // damc_reverse_sweep_ds: the record takes its key from the device-resident state, read here once per sweep
    draw_key(ds, c.seed, c.step_offset);
    *dst = c;
  }
  // every range is grid-stride: the grid is capped (sweep_setup_grid), so B*nz may exceed the thread count
  const long st = (long)gridDim.x * blockDim.x;
  // a caller's NaN is stored canonical, so a NaN payload can never be the hand-off sentinel (TS_SENT) in the ring
  for (long j = i; j < n; j += st) {
    const float v = zt[j];
    zw[j] = (v != v) ? __builtin_bit_cast(float, 0x7FC00000u) : v;
  }
  for (long j = i; j < nzero; j += st) zero[j] = 0u;
  // sentinel hand-offs: every ring slot of the sweep (16 B per store)
  const float sv = __builtin_bit_cast(float, 0x7FC0DEADu);
  const f32x4 s4 = {sv, sv, sv, sv};
  for (long j = i; j < ns1; j += st) s1[j] = s4;
  for (long j = i; j < ns2; j += st) s2[j] = s4;
}

__global__ void copy_kernel(const float* src, float* dst, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// the row-resident form's LDS image (denoiser_rows.hip) of 16 rows
int rows_ld(const damc_denoiser_t* d, damc::RowsBlock* b) {
  damc::RowsBlock tmp[7];
  return damc::rows_layout(d->nz, d->blocks[0].dout, kpad(2 * d->nz), b ? b : tmp);
}
bool rows_fit(const damc_denoiser_t* d) {
  return (size_t)damc::ROWS_TM * rows_ld(d, nullptr) * sizeof(float) <= damc::ROWS_LDS_MAX;
}

int validate(const damc_denoiser_t* d) {
  if (!d || d->nz <= 0 || (d->nz & 1) || d->ntemb <= 0 || d->nxemb <= 0) return DAMC_ERR_ARG;
  const int nz = d->nz;
  const int w = d->blocks[0].dout;
  // in0 in1 in2 mid out0 out1 out2 widths (Diffusion_UnetA with w = 32 * nf)
  const int din[7] = {2 * nz, w, 2 * w, 2 * w, 4 * w, 4 * w, 2 * w};
  const int dout[7] = {w, 2 * w, 2 * w, 2 * w, 2 * w, w, nz};
  if (!d->bmat || !d->tw1 || !d->tb1 || !d->tw2 || !d->tb2) return DAMC_ERR_ARG;
  for (int j = 0; j < 7; ++j) {
    const damc_csq_block_t& b = d->blocks[j];
    if (b.din != din[j] || b.dout != dout[j]) return DAMC_ERR_ARG;
    if (!b.wl || !b.bl || !b.ws || !b.bs || !b.wg || !b.bg || !b.wb || !d->wctx[j] || !d->bctx[j]) return DAMC_ERR_ARG;
    // float4 fragments / staging need every width % 4 == 0 (out2's dout = nz aside: the row-resident form takes any
    // even nz); the in0 LDS image must fit
    if ((b.din & 3) || (j < 6 && (b.dout & 3))) return DAMC_ERR_UNSUPPORTED;
  }
  if (nz > 16 * EMB_G) return DAMC_ERR_UNSUPPORTED;
  // nz % 4 != 0: the per-call stages run blocks 0-5 on the skinny GEMM and out2 on its own small kernels, and the
  // chain runs row-resident, which must fit its LDS image
  if (narrow_out2(d) && ((d->ntemb & 15) || (d->nxemb & 3) || (w & 15) || !rows_fit(d))) return DAMC_ERR_UNSUPPORTED;
  return 0;
}

// DAMC_SWEEP_ROWS=1 (read per call): the row-resident form for every shape
bool rows_forced() {
  const char* e = getenv("DAMC_SWEEP_ROWS");
  return e && e[0] == '1';
}

struct TabEntry {
  int dev;
  std::vector<float> key;
  float* d;
};
std::mutex g_tab_mu;
std::vector<TabEntry> g_tabs;

}  // namespace

namespace damc {

int sum_dout(const damc_denoiser_t* d) {
  int s = 0;
  for (int j = 0; j < 7; ++j) s += lay_dout(d->blocks[j].dout);
  return s;
}

size_t carve(const damc_denoiser_t* d, int B, int n, char* base, SweepWs* w) {
  size_t off = 0;
  auto take = [&](long floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += ((size_t)floats * sizeof(float) + 255) / 256 * 256;
    return p;
  };
  const int S = sum_dout(d);
  const int nt = d->ntemb, nx = d->nxemb;
  SweepWs t;
  for (int j = 0; j < 7; ++j) {
    const damc_csq_block_t& b = d->blocks[j];
    const int ntn = (b.dout + TC - 1) / TC;
    t.w[j] = take((long)ntn * 16 * kpad(b.din));
    t.bls[j] = take((long)ntn * 16);
    t.wgb[j] = take((long)b.dout * 2 * b.dout);
    t.bg2[j] = take(2L * b.dout);
  }
  t.wctx_t = take((long)nt * S);
  t.wctx_x = take((long)nx * S);
  t.bctx = take(S);
  t.tw1t = take((long)nt * nt);
  t.tw2t = take((long)nt * nt);
  t.bmat = take((long)d->nz * (d->nz / 2));
  t.px = take((long)B * S);
  t.qt = take((long)n * S);
  t.t1 = take((long)n * nt);
  t.t2 = take((long)n * nt);
  t.xs = take((long)B * nx);
  t.cx = take((long)n * B * S);
  t.gh = take((long)n * B * 2 * S);
  t.z = take((long)B * d->nz);
  for (int j = 0; j < 7; ++j) t.outs[j] = take((long)B * d->blocks[j].dout);
  t.call = reinterpret_cast<SweepCall*>(take(64));
  // (the team sweep's rings: never used by a shape only the row-resident form takes)
  t.ring = take(narrow_out2(d) ? 0 : (long)n * B * S);
  t.zring = take(narrow_out2(d) ? 0 : (long)(n + 1) * B * d->nz);
  t.tab = take(8L * n);
  t.err = reinterpret_cast<int*>(take(1));
  t.bytes = off;
  if (w) *w = t;
  return off;
}

// the step table (c0..c4, is_last, noisy_k per step) of a schedule, uploaded once per (device, schedule) and kept:
// a sweep then copies nothing from the host, so it can be captured into a HIP graph (after one eager call with
// the same schedule, as torch.cuda.graphs' warm-up does)
int step_table(const float* coef, int n, hipStream_t s, const float** out) {
  int dev = 0;
  DAMC_CHECK(hipGetDevice(&dev));
  std::vector<float> key(coef, coef + 6 * (size_t)n);
  std::lock_guard<std::mutex> lk(g_tab_mu);
  for (const TabEntry& e : g_tabs)
    if (e.dev == dev && e.key == key) {
      *out = e.d;
      return 0;
    }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  DAMC_CHECK(hipStreamIsCapturing(s, &cs));
  if (cs != hipStreamCaptureStatusNone) return DAMC_ERR_UNSUPPORTED;  // first use of a schedule inside a capture
  std::vector<float> tab(8 * (size_t)n, 0.f);
  for (int k = 0, noisy = 0; k < n; ++k) {
    for (int i = 0; i < 6; ++i) tab[8 * k + i] = coef[6 * (size_t)k + i];
    tab[8 * k + 6] = (float)noisy;
    if (coef[6 * (size_t)k + 5] == 0.f) ++noisy;
  }
  float* d = nullptr;
  DAMC_CHECK(hipMalloc(&d, tab.size() * sizeof(float)));
  DAMC_CHECK(hipMemcpy(d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  if (g_tabs.size() >= 64) {  // a handful of schedules per process in practice
    (void)hipFree(g_tabs.front().d);
    g_tabs.erase(g_tabs.begin());
  }
  g_tabs.push_back(TabEntry{dev, std::move(key), d});
  *out = d;
  return 0;
}

}  // namespace damc

extern "C" long damc_sweep_team_failures(int device) {
  if (device < 0 || device >= 64) return -1;
  return team_failures(device);
}

extern "C" size_t damc_sweep_workspace_bytes(const damc_denoiser_t* d, int B, int n) {
  if (validate(d) || B <= 0 || n <= 0) return 0;
  if (rows_forced() && !rows_fit(d)) return 0;
  return carve(d, B, n, nullptr, nullptr);
}

// ---- 4 (row-resident, denoiser_rows.hip): one launch, each workgroup runs every step and block of its rows on the
// caller's zt in place; the call's values travel in the kernel arguments
static int rows_args(const Stages& st, damc::RowsArgs& ra, float* zt, int B, int n, const float* coef, int with_noise,
                     const float* noise, uint64_t seed, uint64_t chain_base, uint64_t step_offset, float* eps_log,
                     int eps_log_steps, const damc_draw_state_t* ds = nullptr) {
  const damc_denoiser_t* d = st.d;
  memset(&ra, 0, sizeof(ra));
  ra.ld = rows_ld(d, ra.b);
  for (int j = 0; j < 7; ++j) {
    const damc_csq_block_t& bk = d->blocks[j];
    damc::RowsBlock& p = ra.b[j];
    p.w = st.w.w[j];
    p.bls = st.w.bls[j];
    p.din = bk.din;
    p.kp = kpad(bk.din);
    p.dout = bk.dout;
    p.ntn = (bk.dout + TC - 1) / TC;
    p.ghoff = 2 * st.coloff[j];
  }
  ra.bmat = st.w.bmat;
  ra.nz = d->nz;
  ra.B = B;
  ra.n = n;
  ra.residual = d->residual;
  ra.gh = st.w.gh;
  ra.ldgh = 2L * st.S;
  ra.zt = zt;
  ra.noise = (with_noise && noise) ? noise : nullptr;
  ra.eps_log = eps_log;
  ra.eps_log_steps = eps_log ? eps_log_steps : 0;
  ra.seed = seed;
  ra.chain_base = chain_base;
  ra.step_offset = step_offset;
  ra.draws = ds;
  ra.with_noise = with_noise ? 1 : 0;
  return step_table(coef, n, st.s, &ra.tab);
}

static double rows_flops(const damc_denoiser_t* d, double rows, int n) {
  double fl = 0;
  for (int j = 0; j < 7; ++j) fl += 2.0 * rows * 2.0 * d->blocks[j].din * d->blocks[j].dout;
  return fl * n;
}

// ---- the dispatch's two decisions (damc_sweep_form asks the same two): this one, and sweep_team (sweep_team.hip)
// the row-resident form: a narrow out2 has no other, DAMC_SWEEP_ROWS=1 asks for it
static bool sweep_rows(const damc_denoiser_t* d) { return narrow_out2(d) || rows_forced(); }

// step_offset: Philox step index of the first noisy step (a single-step call continues a sweep's noise stream)
static int reverse_sweep_impl(const damc_denoiser_t* d, const float* xemb, float* zt, int B, int n,
                              const float* temb_in, const float* coef, int with_noise, const float* noise,
                              uint64_t seed, uint64_t chain_base, float* eps_log, int eps_log_steps, void* wsp,
                              size_t wsb, void* stream, uint64_t step_offset, bool allow_graph,
                              const damc_draw_state_t* ds = nullptr) {
  int rc = validate(d);
  if (rc) return rc;
  if (!xemb || !zt || !temb_in || !coef || B <= 0 || n <= 0) return DAMC_ERR_ARG;
  const size_t need = carve(d, B, n, nullptr, nullptr);
  if (!wsp || wsb < need) return DAMC_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  Stages st;
  stages_init(st, d, B, n, wsp, s);
  const SweepWs& w = st.w;
  const int S = st.S;
  const bool rows = sweep_rows(d);
  if (rows && !rows_fit(d)) return DAMC_ERR_UNSUPPORTED;

  // ---- 1-3: the weights, then everything that does not depend on zt: ctx c for every (step, row) from the time MLP
  // (n rows) and the xemb part (B rows), and every block's gate and hyper bias
  if ((rc = stage_pack(st))) return rc;
  if ((rc = stage_time(st, temb_in, n))) return rc;
  if ((rc = stage_px(st, xemb, B, w.xs, w.px))) return rc;
  if ((rc = launch_ctx(w.px, 0, w.qt, n, B, S, w.cx, s))) return rc;
  if ((rc = stage_hyper(st, w.cx, w.gh, (long)n * B))) return rc;

  // ---- 4. the dependent chain
  if (rows) {
    damc::RowsArgs ra;
    if ((rc = rows_args(st, ra, zt, B, n, coef, with_noise, noise, seed, chain_base, step_offset, eps_log,
                        eps_log_steps, ds)))
      return rc;
    ProfScope ps("denoise_chain", rows_flops(d, B, n), s);
    return damc::launch_sweep_rows(ra, s);
  }
  SweepCall call;
  call.noise = (with_noise && noise) ? noise : nullptr;
  call.eps_log = eps_log;
  call.eps_log_steps = eps_log ? eps_log_steps : 0;
  call.seed = seed;
  call.chain_base = chain_base;
  call.step_offset = step_offset;
  call.with_noise = with_noise ? 1 : 0;
  const long nzb = (long)B * d->nz;
  TsArgs ta;
  int tP = 0;
  size_t tsm = 0;
  // inside a caller's stream capture the launch chain (when it is used) records its kernels eagerly into the caller's
  // graph instead of replaying its own cached graph
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  DAMC_CHECK(hipStreamIsCapturing(s, &cap));
  const bool capturing = cap != hipStreamCaptureStatusNone;
  int dev = 0;
  DAMC_CHECK(hipGetDevice(&dev));
  const bool team = sweep_team(d, w, B, n, capturing, dev, &ta, &tP, &tsm);
  int* health = team ? team_health_word(dev, capturing) : nullptr;
  // the data-driven hand-off's sentinels: every ring slot of the sweep (TS_SENT)
  const long nzero = team ? 1 : 0, ns1 = team ? (long)n * B * S / 4 : 0, ns2 = team ? (long)n * nzb / 4 : 0;
  const long sgrid = std::min<long>(std::max<long>(std::max(nzb, nzero), (ns1 + ns2) / 8), 1L << 16);
  hipLaunchKernelGGL(sweep_setup_kernel, dim3((unsigned)((sgrid + 255) / 256)), dim3(256), 0, s, call, w.call, zt,
                     team ? w.zring : w.z, nzb, reinterpret_cast<unsigned*>(w.err), nzero, reinterpret_cast<f32x4*>(w.ring), ns1,
                     reinterpret_cast<f32x4*>(w.zring + nzb), ns2, ds);
  DAMC_LAUNCH_CHECK();
  double flops_step = 0;
  for (int j = 0; j < 7; ++j) flops_step += 2.0 * B * 2.0 * d->blocks[j].din * d->blocks[j].dout;
  {
    ProfScope ps("denoise_chain", flops_step * n, s);
    if (team) {
      if ((rc = run_chain_team(ta, tP, tsm, coef, s))) return rc;
    } else if (allow_graph && graphs_enabled() && !capturing) {
      if ((rc = run_chain_graph(d, w, wsp, wsb, B, n, coef, s))) return rc;
      chain_trace_dump(s);
    } else {
      if ((rc = run_chain_eager(d, w, B, n, coef, s))) return rc;
    }
  }
  if (team)
    launch_team_finish(ta, zt, health, s);
  else
    hipLaunchKernelGGL(copy_kernel, dim3((unsigned)((nzb + 255) / 256)), dim3(256), 0, s,
                       w.z, zt, nzb);
  return (int)hipGetLastError();
}

extern "C" int damc_reverse_sweep(const damc_denoiser_t* d, const float* xemb, float* zt, int B, int n,
                                  const float* temb_in, const float* coef, int with_noise, const float* noise,
                                  uint64_t seed, uint64_t chain_base, float* eps_log, int eps_log_steps,
                                  void* wsp, size_t wsb, void* stream) {
  return reverse_sweep_impl(d, xemb, zt, B, n, temb_in, coef, with_noise, noise, seed, chain_base, eps_log,
                            eps_log_steps, wsp, wsb, stream, 0, true);
}

// the drawn form: seed and counter (added to the sweep's step offset 0) from the device-resident state; the same
// launches, the state read by sweep_setup_kernel (team, launch chain) or by the row-resident kernel itself
extern "C" int damc_reverse_sweep_ds(const damc_denoiser_t* d, const float* xemb, float* zt, int B, int n,
                                     const float* temb_in, const float* coef, int with_noise, const float* noise,
                                     const damc_draw_state_t* state, uint64_t chain_base, float* eps_log,
                                     int eps_log_steps, void* wsp, size_t wsb, void* stream) {
  if (!state) return DAMC_ERR_ARG;
  return reverse_sweep_impl(d, xemb, zt, B, n, temb_in, coef, with_noise, noise, 0, chain_base, eps_log,
                            eps_log_steps, wsp, wsb, stream, 0, true, state);
}

// SURVEY.md §8b names
extern "C" int damc_q_reverse_sweep(const damc_denoiser_t* d, const float* xemb, float* zt, int B, int n,
                                    const float* temb_in, const float* coef, int with_noise, const float* noise,
                                    uint64_t seed, uint64_t chain_base, float* eps_log, int eps_log_steps,
                                    void* wsp, size_t wsb, void* stream) {
  return reverse_sweep_impl(d, xemb, zt, B, n, temb_in, coef, with_noise, noise, seed, chain_base, eps_log,
                            eps_log_steps, wsp, wsb, stream, 0, true);
}

extern "C" int damc_denoise_step(const damc_denoiser_t* d, const float* xemb, float* zt, int B, const float* temb_row,
                                 const float* coef_row, int with_noise, const float* noise, uint64_t seed,
                                 uint64_t noise_step, uint64_t chain_base, float* eps, void* wsp, size_t wsb,
                                 void* stream) {
  return reverse_sweep_impl(d, xemb, zt, B, 1, temb_row, coef_row, with_noise, noise, seed, chain_base, eps,
                            eps ? 1 : 0, wsp, wsb, stream, noise_step, false);
}

// what the per-call stages of this denoiser run on, by shape alone (pointers taken as 16-byte aligned, no environment
// switch read): the predicates stages_init and stage_hyper branch on
extern "C" int damc_sweep_stages(const damc_denoiser_t* d) {
  const int rc = validate(d);
  if (rc) return -rc;
  const bool narrow = narrow_out2(d);
  int coloff[7];
  for (int j = 0, o = 0; j < 7; ++j) {
    coloff[j] = o;
    o += lay_dout(d->blocks[j].dout);
  }
  return (stages_skinny(d) ? 1 : 0) | (narrow ? 2 : 0) | (rows_fit(d) ? 4 : 0) |
         (hyper_limb_blocks(d, narrow ? 6 : 7, coloff) << 8);
}

// the form reverse_sweep_impl would take now for (d, batch, n_steps) on the current device, outside a capture:
// 0 none (the sweep would refuse), 1 row-resident, 2 team on the generic kernel, 3 team on sweep_fast_kernel,
// 4 launch chain.  The environment switches are read as the sweep reads them; nothing is launched.
extern "C" int damc_sweep_form(const damc_denoiser_t* d, int B, int n) {
  if (validate(d) || B <= 0 || n <= 0) return 0;
  if (sweep_rows(d)) return rows_fit(d) ? 1 : 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  SweepWs w;
  carve(d, B, n, nullptr, &w);
  TsArgs ta;
  int tP = 0;
  size_t tsm = 0;
  if (!sweep_team(d, w, B, n, false, dev, &ta, &tP, &tsm)) return 4;
  return ta.fast ? 3 : 2;
}

// ------------------------------------------------------------------------------------- the guided sweep
// Classifier-free guidance (_netQ_U.forward with cond_w > 0, workspace/src/diffusion_net.py:595-620) as one sweep: the
// reference evaluates the denoiser twice per step, on the encoder's xemb and on a fresh prior_emb(randn), and steps on
// (1 + w) eps_c - w eps_u.  The conditional planes (px, cx, gh) are the reverse sweep's.  The unconditional context
// changes every step, so its planes are per (step, row) throughout: px_u (n B, S) by the same GEMM with M = n B, cx_u
// by the same ctx kernel with px strided per step, gh_u by the same hyper stage; the same kernels for both branches,
// each computing a row by itself, so a row's gate does not depend on the plane or batch it sits in.  The chain is the
// twin-row form of denoiser_rows.hip: always row-resident, no team, no launch chain.
// Workspace beyond the reverse sweep's: px_u, cx_u (S each) and gh_u (2 S) floats per (step, row), plus nxemb for
// SiLU(xemb_unc) where the skinny GEMM does not apply: 4 S = 5632 floats at the CIFAR widths, ~0.3 GB at B = 128,
// n = 100 (xemb_unc itself, the caller's, is another n B nxemb floats).
namespace {
struct GuidedWs {
  float *px_u, *cx_u, *gh_u, *xs_u;
};

bool guided_ok(const damc_denoiser_t* d) { return !validate(d) && !narrow_out2(d) && rows_fit(d); }

size_t carve_guided(const damc_denoiser_t* d, int B, int n, char* base, GuidedWs* g) {
  size_t off = carve(d, B, n, nullptr, nullptr);
  auto take = [&](long floats) -> float* {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += ((size_t)floats * sizeof(float) + 255) / 256 * 256;
    return p;
  };
  const long S = sum_dout(d), M = (long)n * B;
  const bool skinny = stages_skinny(d);  // (guided_ok: never narrow, all 7 blocks)
  GuidedWs t;
  t.px_u = take(M * S);
  t.cx_u = take(M * S);
  t.gh_u = take(M * 2 * S);
  t.xs_u = take(skinny ? 0 : M * d->nxemb);
  if (g) *g = t;
  return off;
}
}  // namespace

extern "C" size_t damc_guided_sweep_workspace_bytes(const damc_denoiser_t* d, int B, int n) {
  if (B <= 0 || n <= 0 || !guided_ok(d)) return 0;
  return carve_guided(d, B, n, nullptr, nullptr);
}

extern "C" int damc_guided_sweep(const damc_denoiser_t* d, const float* xemb, const float* xemb_unc, float cond_w,
                                 float* zt, int B, int n, const float* temb_in, const float* coef, int with_noise,
                                 const float* noise, uint64_t seed, uint64_t chain_base, float* eps_log,
                                 int eps_log_steps, void* wsp, size_t wsb, void* stream) {
  int rc = validate(d);
  if (rc) return rc;
  if (!xemb || !xemb_unc || !zt || !temb_in || !coef || B <= 0 || n <= 0 || !(cond_w > 0.f)) return DAMC_ERR_ARG;
  if (!guided_ok(d)) return DAMC_ERR_UNSUPPORTED;
  if ((long)n * B > (1L << 30)) return DAMC_ERR_UNSUPPORTED;  // the planes' row count as the GEMMs' int M
  const size_t need = carve_guided(d, B, n, nullptr, nullptr);
  if (!wsp || wsb < need) return DAMC_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  Stages st;
  stages_init(st, d, B, n, wsp, s);
  GuidedWs gw;
  carve_guided(d, B, n, reinterpret_cast<char*>(wsp), &gw);
  const SweepWs& w = st.w;
  const int S = st.S;
  const int M = n * B;

  if ((rc = stage_pack(st))) return rc;
  if ((rc = stage_time(st, temb_in, n))) return rc;
  // the conditional planes, as the reverse sweep's
  if ((rc = stage_px(st, xemb, B, w.xs, w.px))) return rc;
  if ((rc = launch_ctx(w.px, 0, w.qt, n, B, S, w.cx, s))) return rc;
  if ((rc = stage_hyper(st, w.cx, w.gh, M))) return rc;
  // the unconditional planes: a context per (step, row)
  if ((rc = stage_px(st, xemb_unc, M, gw.xs_u, gw.px_u))) return rc;
  if ((rc = launch_ctx(gw.px_u, (long)B * S, w.qt, n, B, S, gw.cx_u, s))) return rc;
  if ((rc = stage_hyper(st, gw.cx_u, gw.gh_u, M))) return rc;

  damc::RowsArgs ra;
  if ((rc = rows_args(st, ra, zt, B, n, coef, with_noise, noise, seed, chain_base, 0, eps_log, eps_log_steps)))
    return rc;
  ra.gh_u = gw.gh_u;
  ra.gw = cond_w;
  ra.gw1 = 1.f + cond_w;  // the reference's (1 + cond_w), rounded to fp32 once
  ProfScope ps("denoise_chain", rows_flops(d, 2.0 * B, n), s);
  return damc::launch_sweep_rows_guided(ra, s);
}
