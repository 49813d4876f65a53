// sweep_chain.hip — the launch chain of the reverse sweep (denoiser.hip): chain_kernel, one launch per block and
// step, and the per-schedule HIP graph that replays them.  The form a sweep takes when the team launch
// (sweep_team.hip) is switched off, does not fit, or has needed its rescue once in this process.
//
// After the per-call stages (sweep_stages.hip) what stays in the chain is x Wl^T and x Ws^T of the 7 blocks plus the
// reverse-step update: 7 dependent launches per step (block j+1 needs every column of block j for its rows).  They
// are kept short:
//   * one workgroup = 16 rows x 8 output columns of BOTH products (one 16 x 16 v_mfma_f32_16x16x4_f32 tile: 8 Wl
//     rows + 8 Ws rows of the packed weight), 4 waves splitting K in quarters; each lane's x and weight fragments
//     are f32x4 global loads issued together up front through the k-permutation of the MFMA steps (step s of
//     k-group g reads k = 16 g + 4 (lane >> 4) + s on both operands), so a launch costs one memory round trip;
//   * the epilogue operands (gate, hyper bias, biases, zt, the Philox draw) are fetched before the main loop;
//   * N tiles are the fastest grid index: with dout / 8 a multiple of 8 an N tile stays on one XCD for every step,
//     so each XCD keeps 1/8 of the chain's weights in its L2;
//   * the 7n launches are captured once into a HIP graph (cached per workspace / shape / schedule) and replayed:
//     eager launches cost the host ~3.5 us each, more than these kernels take on the GPU.
// The last block's epilogue applies eps = z + out, pred_x_from_eps and the reverse step with Philox noise in place.
//
// Process-wide host state defined here: the graph cache with its mutex, and the chain trace buffer (tools only).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "sweep_impl.h"

using namespace damc;

namespace {

struct ChainArgs {
  const float* srcA;  // block input = lrelu(cat(srcA, srcB), 0.01) (not in0)
  const float* srcB;
  int wa, wb;
  int emb;            // in0: input = [sin 2pi zB, cos 2pi zB, z]
  const float* z;     // (B, nz) current zt (the workspace copy)
  const float* bmat;  // B^T (nz/2, nz), packed per call
  int nz;
  int din, kp, dout, B;
  const float* w;     // [ntn][16][kp]: rows 0-7 Wl, 8-15 Ws of the tile's columns (zero-padded)
  const float* bls;   // [ntn][16]: bl, bs
  const float* gh;    // this step's rows: gate at gh[b * ldgh + n], hyper bias at gh[b * ldgh + dout + n]
  long ldgh;
  float* out;         // (B, dout)
  // last block
  int final_, residual, last, k, noisy_k;
  float c0, c1, c2, c3, c4;
  float* zt;          // == z
  const SweepCall* call;
  uint64_t* trace;  // tools only (DAMC_CHAIN_TRACE): [launch][512][2] 100 MHz stamps {block start, block end}
  int li;           // launch index in the sweep (trace row)
  int dbg;  // timing experiments only (DAMC_CHAIN_DBG, wrong results): 1 no x loads, 2 no weight loads, 4 no MFMA,
            // 8 no epilogue prefetch, 16 no output stores; in0: 32 no sin/cos, 64 no B loads, 128 no zB MFMA
};

// EMB: the in0 block (Fourier embedding, sin / cos with their large-argument path) is its own instantiation, so
// the six other blocks' kernels carry no scratch segment
template <bool EMB>
__global__ __launch_bounds__(CH_THREADS) void chain_kernel(ChainArgs a) {
  __shared__ __attribute__((aligned(16))) float red[CH_WAVES][TM][16];
  extern __shared__ __attribute__((aligned(16))) float embs[];  // in0: [TM][emb_ld(kp)]
  if (a.trace && threadIdx.x == 0) { a.trace[((long)a.li * 512 + blockIdx.x) * 8] = __builtin_amdgcn_s_memrealtime(); a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 2] = __builtin_amdgcn_s_memtime(); }
  if (a.trace && (threadIdx.x == 64 || threadIdx.x == 192)) a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 6 + (threadIdx.x >> 7)] = __builtin_amdgcn_s_memtime();
  if (a.dbg & 512) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntn = (a.dout + TC - 1) / TC;
  const int tn = blockIdx.x % ntn, tm = blockIdx.x / ntn;
  const int r0 = tm * TM, n0 = tn * TC;
  const int m = lane & 15, q = lane >> 4;

  // ---- epilogue operands first (independent of the main loop): thread (row er, column ec)
  const int er = tid >> 3, ec = tid & 7;
  const int erow = r0 + er, ecol = n0 + ec;
  const bool eok = tid < TM * TC && erow < a.B && ecol < a.dout;
  float gate = 0.f, hb = 0.f, bl = 0.f, bs = 0.f, zv = 0.f, xi = 0.f;
  const SweepCall* call = a.call;
  if (eok && !(a.dbg & 8)) {
    gate = a.gh[(long)erow * a.ldgh + ecol];
    hb = a.gh[(long)erow * a.ldgh + a.dout + ecol];
    bl = a.bls[tn * 16 + ec];
    bs = a.bls[tn * 16 + 8 + ec];
    if (a.final_) {
      zv = a.zt[(long)erow * a.nz + ecol];
      // every per-call field in one round trip (not three dependent ones)
      const int with_noise = call->with_noise;
      const float* noise = call->noise;
      const uint64_t seed = call->seed, chain_base = call->chain_base, step_offset = call->step_offset;
      if (!a.last && with_noise) {
        if (noise) {
          xi = noise[((long)a.noisy_k * a.B + erow) * a.nz + ecol];
        } else {
          float n4[4];
          philox_normal4(seed, chain_base + erow, step_offset + a.noisy_k, (uint32_t)(ecol >> 2),
                         DAMC_STREAM_SWEEP, n4);
          xi = pick4(n4, ecol);
        }
      }
    }
  }

  // ---- this wave's K range and, for in0, its first weight chunk now: the embedding below is a dependent
  // load -> MFMA -> sin/cos phase, so the weights' memory round trip overlaps it instead of following it
  const int kq = a.kp / CH_WAVES;
  const int ng = kq >> 4;
  const int kbase = wave * kq;
  const float* wrow = a.w + ((long)tn * 16 + m) * a.kp + kbase + 4 * q;
  f32x4 wpre[CH_CHUNK];
  if (EMB) {
#pragma unroll
    for (int c = 0; c < CH_CHUNK; ++c)
      wpre[c] = (c < ng && !(a.dbg & 2)) ? *reinterpret_cast<const f32x4*>(wrow + 16 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- in0: the Fourier input embedding of the 16 rows into LDS (zB on MFMA, wave w -> 16-column tiles w, w+4..)
  const int ld = emb_ld(a.kp);
  if (EMB) {
    const int nz = a.nz, half = nz >> 1;
    const int row = r0 + m;
    const bool rok = row < a.B;
    // all of a lane's z and B operands are loaded before the first MFMA (one memory round trip; nz <= 128)
    f32x4 zv4[EMB_G];
#pragma unroll
    for (int g = 0; g < EMB_G; ++g) {
      const int k = 16 * g + 4 * q;
      zv4[g] = (rok && k < nz) ? *reinterpret_cast<const f32x4*>(a.z + (long)row * nz + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int t = wave; t * 16 < half; t += CH_WAVES) {
      const int col = t * 16 + m;
      const bool cok = col < half;
      f32x4 bv[EMB_G];  // a.bmat is B^T (half, nz): lane (m, q) reads B[16 g + 4 q + s][col] as one f32x4
#pragma unroll
      for (int g = 0; g < EMB_G; ++g) {
        const int k = 16 * g + 4 * q;
        bv[g] = (cok && k < nz && !(a.dbg & 64)) ? *reinterpret_cast<const f32x4*>(a.bmat + (long)col * nz + k)
                                                  : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (!(a.dbg & 128)) acc = emb_zb(zv4, bv);
      // sin / cos (2 pi zB) on the hardware units, whose argument is in revolutions: t = zB - rint(zB) is exact,
      // so the only rounding is the unit's (the reference rounds 2 pi zB to fp32 first, ~4e-6 rad at |zB| ~ 10;
      // both are below the spread of zB itself between summation orders)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 4 * q + r;
        if (cok) {
          const float t = acc[r] - rintf(acc[r]);
          const bool ok = r0 + rr < a.B;
          embs[rr * ld + col] = ok ? ((a.dbg & 32) ? t : __builtin_amdgcn_sinf(t)) : 0.f;
          embs[rr * ld + half + col] = ok ? ((a.dbg & 32) ? t : __builtin_amdgcn_cosf(t)) : 0.f;
        }
      }
    }
    // z itself from the registers that already hold it (wave 0: lane (m, q) has z[row m][16 g + 4 q + s]),
    // then zeros up to kp (no global loads here: a strided load loop would serialise its memory latencies)
    if (wave == 0) {
#pragma unroll
      for (int g = 0; g < EMB_G; ++g)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = 16 * g + 4 * q + s;
          if (k < nz) embs[m * ld + 2 * half + k] = zv4[g][s];
        }
    }
    for (int c = 2 * half + nz + tid; c < a.kp; c += CH_THREADS)
#pragma unroll
      for (int rr = 0; rr < TM; ++rr) embs[rr * ld + c] = 0.f;
    __syncthreads();
  }

  // ---- main loop: wave w covers k in [w kq, (w+1) kq) of the padded K
  const int xrow = r0 + m;
  const bool xok = xrow < a.B;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int g0 = 0; g0 < ng; g0 += CH_CHUNK) {
    f32x4 xa[CH_CHUNK], wb[CH_CHUNK];
#pragma unroll
    for (int c = 0; c < CH_CHUNK; ++c) {
      const int g = g0 + c;
      const int k = kbase + 16 * g + 4 * q;
      f32x4 wv = {0.f, 0.f, 0.f, 0.f}, xv = {0.f, 0.f, 0.f, 0.f};
      if (g < ng) {
        if (EMB && g0 == 0) wv = wpre[c];
        else if (!(a.dbg & 2)) wv = *reinterpret_cast<const f32x4*>(wrow + 16 * g);
        if (EMB) {
          xv = *reinterpret_cast<const f32x4*>(embs + m * ld + k);
        } else if (xok && k < a.din && !(a.dbg & 1)) {
          xv = k < a.wa ? *reinterpret_cast<const f32x4*>(a.srcA + (long)xrow * a.wa + k)
                        : *reinterpret_cast<const f32x4*>(a.srcB + (long)xrow * a.wb + (k - a.wa));
        }
      }
      wb[c] = wv;
      xa[c] = xv;
    }
    if ((a.dbg & 1024) && g0 == 0) {
      __builtin_amdgcn_s_waitcnt(0);
      if (a.trace && tid == 0) a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 3] = __builtin_amdgcn_s_memtime();
    }
#pragma unroll
    for (int c = 0; c < CH_CHUNK; ++c) {
      f32x4 x = xa[c];
      if (!EMB) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] > 0.f ? x[e] : 0.01f * x[e];
      }
      if (a.dbg & 4) {
        acc[0] += x[0] * wb[c][0] + x[1] * wb[c][1] + x[2] * wb[c][2] + x[3] * wb[c][3];
        continue;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s], wb[c][s], acc, 0, 0, 0);
    }
  }
  if (a.dbg & 256) {
    if (acc[0] == 12345.f) a.out[0] = acc[1];
    return;
  }
  // C layout 16x16x4: column = lane & 15 (0-7 Wl, 8-15 Ws), rows 4 (lane >> 4) + r
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * q + r][m] = acc[r];
  __syncthreads();
  if (a.trace && tid == 0) a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 4] = __builtin_amdgcn_s_memtime();

  if (!eok) return;
  float l = 0.f, sk = 0.f;
#pragma unroll
  for (int w = 0; w < CH_WAVES; ++w) {  // fixed order: deterministic
    l += red[w][er][ec];
    sk += red[w][er][8 + ec];
  }
  // ConcatSquashLinearSkipCtx.forward: ret = layer(x) * gate + bias; ret + skip(x)
  const float o = __builtin_fmaf(l + bl, gate, hb) + (sk + bs);  // the fma spelled out: every sweep form rounds alike
  if (!a.final_) {
    if (!(a.dbg & 16)) a.out[(long)erow * a.dout + ecol] = o;
    if (a.trace && tid == 0) { a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 1] = __builtin_amdgcn_s_memrealtime(); a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 5] = __builtin_amdgcn_s_memtime(); }
    return;
  }
  // reverse step (diffusion_net.py:601-620): eps = z + out; pred = c0 (z - eps c1)
  const long zi = (long)erow * a.nz + ecol;
  const float eps = a.residual ? zv + o : o;
  if (call->eps_log && a.k < call->eps_log_steps) call->eps_log[(long)a.k * a.B * a.nz + zi] = eps;
  const float pred = mul_rn(a.c0, sub_rn(zv, mul_rn(eps, a.c1)));
  float zn;
  if (a.last) {
    zn = pred;
  } else {
    zn = add_rn(mul_rn(a.c2, zv), mul_rn(a.c3, pred));
    if (call->with_noise) zn = add_rn(zn, mul_rn(a.c4, xi));
  }
  a.zt[zi] = zn;
  if (a.trace && tid == 0) { a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 1] = __builtin_amdgcn_s_memrealtime(); a.trace[((long)a.li * 512 + blockIdx.x) * 8 + 5] = __builtin_amdgcn_s_memtime(); }
}

struct Launch {
  ChainArgs a;
  unsigned grid;
  size_t smem;
};

// tools only: DAMC_CHAIN_TRACE=<file> gives every chain launch a stamp row; chain_trace_dump writes them after the
// sweep (host sync) as {launches, then [launch][512][2] stamps}
uint64_t* g_trace = nullptr;
long g_trace_rows = 0;
uint64_t* chain_trace_buffer(long rows) {
  static const bool on = getenv("DAMC_CHAIN_TRACE") != nullptr;
  if (!on || rows > 4096) return nullptr;
  if (!g_trace) {
    if (hipMalloc(&g_trace, 4096L * 512 * 8 * sizeof(uint64_t)) != hipSuccess) g_trace = nullptr;
  }
  g_trace_rows = rows;
  return g_trace;
}

// the chain launches of one sweep (n steps from step index k0), in order
void chain_launches(const damc_denoiser_t* d, const SweepWs& w, int B, int n, const float* coef,
                    std::vector<Launch>& out) {
  const int S = sum_dout(d);
  int coloff[7];
  for (int j = 0, o = 0; j < 7; ++j) {
    coloff[j] = o;
    o += d->blocks[j].dout;
  }
  float* const* O = w.outs;
  const float* srcA[7] = {nullptr, O[0], O[1], O[2], O[3], O[4], O[5]};
  const float* srcB[7] = {nullptr, nullptr, nullptr, nullptr, O[2], O[1], O[0]};
  const int wa[7] = {0, d->blocks[0].dout, d->blocks[1].dout, d->blocks[2].dout, d->blocks[3].dout,
                     d->blocks[4].dout, d->blocks[5].dout};
  const int wbw[7] = {0, 0, 0, 0, d->blocks[2].dout, d->blocks[1].dout, d->blocks[0].dout};
  out.clear();
  static const int dbg = [] {
    const char* e = getenv("DAMC_CHAIN_DBG");
    return e ? atoi(e) : 0;
  }();
  uint64_t* trace = chain_trace_buffer(7L * n);
  int noisy_k = 0;
  for (int k = 0; k < n; ++k) {
    const float* c = coef + 6 * (size_t)k;
    const bool last = c[5] != 0.f;
    for (int j = 0; j < 7; ++j) {
      const damc_csq_block_t& b = d->blocks[j];
      Launch L;
      ChainArgs& a = L.a;
      memset(&a, 0, sizeof(a));
      a.srcA = srcA[j];
      a.srcB = srcB[j];
      a.wa = wa[j];
      a.wb = wbw[j];
      a.emb = j == 0;
      a.z = w.z;
      a.bmat = w.bmat;
      a.nz = d->nz;
      a.din = b.din;
      a.kp = kpad(b.din);
      a.dout = b.dout;
      a.B = B;
      a.w = w.w[j];
      a.bls = w.bls[j];
      a.gh = w.gh + (size_t)k * B * 2 * S + 2 * coloff[j];
      a.ldgh = 2L * S;
      a.out = O[j];
      a.final_ = j == 6;
      a.zt = w.z;
      a.call = w.call;
      a.dbg = dbg;
      a.trace = trace;
      a.li = 7 * k + j;
      if (a.final_) {
        a.residual = d->residual;
        a.last = last;
        a.k = k;
        a.noisy_k = noisy_k;
        a.c0 = c[0];
        a.c1 = c[1];
        a.c2 = c[2];
        a.c3 = c[3];
        a.c4 = c[4];
      }
      L.grid = (unsigned)(((b.dout + TC - 1) / TC) * ((B + TM - 1) / TM));
      L.smem = a.emb ? (size_t)TM * emb_ld(a.kp) * sizeof(float) : 0;
      out.push_back(L);
    }
    if (!last) ++noisy_k;
  }
}

void launch_one(const Launch& L, hipStream_t s) {
  if (L.a.emb) hipLaunchKernelGGL(chain_kernel<true>, dim3(L.grid), dim3(CH_THREADS), L.smem, s, L.a);
  else hipLaunchKernelGGL(chain_kernel<false>, dim3(L.grid), dim3(CH_THREADS), L.smem, s, L.a);
}

int launch_chain(const std::vector<Launch>& ls, hipStream_t s) {
  for (const Launch& L : ls) launch_one(L, s);
  return (int)hipGetLastError();
}

// ---- graph cache: the chain of one sweep depends only on workspace addresses, shapes and the schedule scalars
struct GraphEntry {
  int dev;
  const void* wsp;
  size_t wsb;
  int B, n;
  std::vector<char> key;  // shapes + schedule bytes
  hipGraph_t graph;
  hipGraphExec_t exec;
  unsigned long stamp;
};
std::mutex g_mu;
std::vector<GraphEntry> g_cache;
unsigned long g_clock = 0;
constexpr size_t kMaxGraphs = 16;

std::vector<char> graph_key(const damc_denoiser_t* d, int n, const float* coef) {
  std::vector<char> k;
  auto put = [&](const void* p, size_t nb) { k.insert(k.end(), (const char*)p, (const char*)p + nb); };
  int dims[4] = {d->nz, d->ntemb, d->nxemb, d->residual};
  put(dims, sizeof(dims));
  for (int j = 0; j < 7; ++j) put(&d->blocks[j].din, 2 * sizeof(int));
  put(coef, sizeof(float) * 6 * (size_t)n);
  return k;
}

}  // namespace

namespace damc {

void chain_trace_dump(hipStream_t s) {
  if (!g_trace) return;
  std::vector<uint64_t> h((size_t)g_trace_rows * 512 * 8);
  if (hipStreamSynchronize(s) != hipSuccess) return;
  if (hipMemcpy(h.data(), g_trace, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return;
  if (FILE* f = fopen(getenv("DAMC_CHAIN_TRACE"), "wb")) {
    const long rows = g_trace_rows;
    fwrite(&rows, sizeof(rows), 1, f);
    fwrite(h.data(), sizeof(uint64_t), h.size(), f);
    fclose(f);
  }
  (void)hipMemsetAsync(g_trace, 0, h.size() * sizeof(uint64_t), s);
}

bool graphs_enabled() {
  static const bool on = [] {
    const char* e = getenv("DAMC_SWEEP_GRAPH");
    return !(e && e[0] == '0');
  }();
  return on;
}

// replay (capturing on first use) the chain of a sweep; returns 0 or a hip error
int run_chain_graph(const damc_denoiser_t* d, const SweepWs& w, void* wsp, size_t wsb, int B, int n, const float* coef,
                    hipStream_t s) {
  int dev = 0;
  DAMC_CHECK(hipGetDevice(&dev));
  std::vector<char> key = graph_key(d, n, coef);
  std::lock_guard<std::mutex> lk(g_mu);
  for (GraphEntry& e : g_cache) {
    if (e.dev == dev && e.wsp == wsp && e.wsb == wsb && e.B == B && e.n == n && e.key == key) {
      e.stamp = ++g_clock;
      return (int)hipGraphLaunch(e.exec, s);
    }
  }
  std::vector<Launch> ls;
  chain_launches(d, w, B, n, coef, ls);
  hipStream_t cs;
  DAMC_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipError_t err = hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed);
  if (err == hipSuccess) {
    for (const Launch& L : ls) launch_one(L, cs);
    err = hipStreamEndCapture(cs, &graph);
  }
  if (err == hipSuccess) err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipStreamDestroy(cs);
  if (err != hipSuccess) {
    if (graph) (void)hipGraphDestroy(graph);
    return (int)err;
  }
  if (g_cache.size() >= kMaxGraphs) {
    auto old = std::min_element(g_cache.begin(), g_cache.end(),
                                [](const GraphEntry& x, const GraphEntry& y) { return x.stamp < y.stamp; });
    (void)hipGraphExecDestroy(old->exec);
    (void)hipGraphDestroy(old->graph);
    g_cache.erase(old);
  }
  g_cache.push_back(GraphEntry{dev, wsp, wsb, B, n, std::move(key), graph, exec, ++g_clock});
  return (int)hipGraphLaunch(exec, s);
}

// the same launches straight into the stream (inside a caller's capture, a single step, DAMC_SWEEP_GRAPH=0)
int run_chain_eager(const damc_denoiser_t* d, const SweepWs& w, int B, int n, const float* coef, hipStream_t s) {
  std::vector<Launch> ls;
  chain_launches(d, w, B, n, coef, ls);
  return launch_chain(ls, s);
}

}  // namespace damc
