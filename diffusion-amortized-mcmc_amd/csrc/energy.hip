// energy.hip — per-sample terms of the posterior energy U(z) = |G(z)-x|^2 + E(z) + |z|^2/2 at a fixed z
// (workspace/eval_anomaly_det.py:114-117, train_anomaly_det.py:223-226: the anomaly score), with a fixed summation
// order and no atomics: a row's result depends on that row's data and on the row length alone, never on the batch
// size, the row's index or its neighbours, so any sharding of a batch reproduces the whole batch bit for bit.
//
//   recon_rows_kernel     one workgroup per (row, chunk of RR_CHUNK elements): sum (xhat - x)^2 -> partial (B, nchunk)
//   energy_finish_kernel  one thread per row: chunk partials in chunk order, |z|^2/2 in index order, E(z) from a
//                         buffer -> terms (B, 3), score (B)
#include "common.h"

namespace {

// The chunk length is a constant, so the partition of a row follows from its length alone.  3*256*256 = 12 chunks.
constexpr int RR_CHUNK = 16384;
constexpr int RR_THREADS = 256;
constexpr int RR_WAVES = RR_THREADS / 64;

// Element j of a chunk belongs to thread (j / 4) % RR_THREADS, which adds its elements in index order.  VEC4 reads
// a thread's 4 neighbours as one 16-byte load (row length % 4 == 0 and 16-byte aligned bases: every quad of every
// row is then aligned and whole); the scalar instantiation reads the same elements one by one and masks the ragged
// tail.  Both add the same values in the same order with the same fma, so they give the same bits.
template <bool VEC4>
__global__ __launch_bounds__(RR_THREADS) void recon_rows_kernel(const float* __restrict__ xhat,
                                                                const float* __restrict__ x, long n, int nchunk,
                                                                float* __restrict__ partial) {
  const long row = blockIdx.x / nchunk;
  const int chunk = (int)(blockIdx.x - row * nchunk);
  const long c0 = (long)chunk * RR_CHUNK;
  const int len = (int)(n - c0 < RR_CHUNK ? n - c0 : RR_CHUNK);  // ragged last chunk
  const float* a = xhat + row * n + c0;
  const float* b = x + row * n + c0;
  float acc = 0.f;
  for (int j = threadIdx.x * 4; j < len; j += RR_THREADS * 4) {
    if constexpr (VEC4) {  // len % 4 == 0: j < len implies j + 3 < len
      const float4 u = *reinterpret_cast<const float4*>(a + j);
      const float4 v = *reinterpret_cast<const float4*>(b + j);
      const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
      acc = fmaf(d0, d0, acc);
      acc = fmaf(d1, d1, acc);
      acc = fmaf(d2, d2, acc);
      acc = fmaf(d3, d3, acc);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < len) {
          const float d = a[j + k] - b[j + k];
          acc = fmaf(d, d, acc);
        }
    }
  }
  acc = wave_sum(acc);  // xor butterfly: every lane holds the same, order-fixed sum
  __shared__ float wsum[RR_WAVES];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = wsum[0];
#pragma unroll
    for (int w = 1; w < RR_WAVES; ++w) t += wsum[w];  // waves in wave order
    partial[blockIdx.x] = t;
  }
}

// rows: out[b] = recon (the per-op hook).  terms: {recon, e, |z|^2/2}; score = (rw * recon + e) + |z|^2/2 with every
// operation rounded on its own, the value the same expression on the fp32 terms gives anywhere.
__global__ void energy_finish_kernel(const float* __restrict__ partial, int nchunk, const float* __restrict__ z, int nz,
                                     const float* __restrict__ ebm_e, float rw, int B, float* __restrict__ rows,
                                     float* __restrict__ terms, float* __restrict__ score) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float recon = 0.f;
  for (int c = 0; c < nchunk; ++c) recon += partial[(long)b * nchunk + c];
  if (rows) rows[b] = recon;
  if (!terms) return;
  // one thread adds the row's nz squares in index order; the running error is carried along (Kahan), so the sum is
  // as close to the exact one as a tree reduction's at any nz
  float zz = 0.f, comp = 0.f;
  for (int d = 0; d < nz; ++d) {
    const float v = z[(long)b * nz + d];
    const float y = fmaf(v, v, -comp), t = zz + y;
    comp = (t - zz) - y;
    zz = t;
  }
  const float hz = 0.5f * zz, e = ebm_e ? ebm_e[b] : 0.f;
  terms[3 * (long)b + 0] = recon;
  terms[3 * (long)b + 1] = e;
  terms[3 * (long)b + 2] = hz;
  if (score) score[b] = add_rn(add_rn(mul_rn(rw, recon), e), hz);
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline long rr_nchunk(long n) { return (n + RR_CHUNK - 1) / RR_CHUNK; }

// B rows of n elements are within what one launch covers: one workgroup per (row, chunk), a 31-bit grid
inline bool rr_shape_ok(int B, long n) {
  return B > 0 && n > 0 && n <= (1L << 60) / B && (long)B * rr_nchunk(n) <= 0x7fffffffL;
}

int launch_recon_rows(const float* xhat, const float* x, int B, long n, float* partial, hipStream_t s) {
  const int nchunk = (int)rr_nchunk(n);
  const dim3 grid((unsigned)((long)B * nchunk)), blk(RR_THREADS);
  const bool vec4 = n % 4 == 0 && (uintptr_t)xhat % 16 == 0 && (uintptr_t)x % 16 == 0;
  ProfScope ps("recon_rows", 3.0 * (double)B * (double)n, s);
  if (vec4)
    hipLaunchKernelGGL(recon_rows_kernel<true>, grid, blk, 0, s, xhat, x, n, nchunk, partial);
  else
    hipLaunchKernelGGL(recon_rows_kernel<false>, grid, blk, 0, s, xhat, x, n, nchunk, partial);
  return (int)hipGetLastError();
}

int launch_finish(const float* partial, int nchunk, const float* z, int nz, const float* ebm_e, float rw, int B,
                  float* rows, float* terms, float* score, hipStream_t s) {
  ProfScope ps("energy_finish", (double)B * (nchunk + 2.0 * nz), s);
  hipLaunchKernelGGL(energy_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, partial, nchunk, z, nz, ebm_e,
                     rw, B, rows, terms, score);
  return (int)hipGetLastError();
}

inline long gen_row_elems(const damc_generator_t* g) { return (long)g->nc * g->h * g->w; }

// the carve of damc_posterior_energy's workspace: the generator forward's own, x_hat, chunk partials, E(z), grad E(z)
struct EnergyWs {
  size_t gen, xhat, partial, ebm_e, ebm_g, total;
};

bool energy_carve(const damc_generator_t* g, int B, EnergyWs* w) {
  if (!g || B <= 0) return false;
  const size_t gen = damc_posterior_workspace_bytes(g, B);  // 0: the descriptor is not one the library runs
  if (!gen) return false;
  const long n = gen_row_elems(g);
  if (!rr_shape_ok(B, n) || g->nz <= 0) return false;
  w->gen = gen;
  w->xhat = up256(gen);
  w->partial = w->xhat + up256(sizeof(float) * (size_t)B * (size_t)n);
  w->ebm_e = w->partial + up256(sizeof(float) * (size_t)B * (size_t)rr_nchunk(n));
  w->ebm_g = w->ebm_e + up256(sizeof(float) * (size_t)B);
  w->total = w->ebm_g + up256(sizeof(float) * (size_t)B * (size_t)g->nz);
  return true;
}

}  // namespace

extern "C" size_t damc_recon_rows_workspace_bytes(int B, long n) {
  if (!rr_shape_ok(B, n)) return 0;
  return sizeof(float) * (size_t)B * (size_t)rr_nchunk(n);
}

extern "C" int damc_recon_rows(const float* xhat, const float* x, int B, long n, float* out, void* wsp, size_t wsb,
                               void* stream) {
  if (!xhat || !x || !out || !rr_shape_ok(B, n)) return DAMC_ERR_ARG;
  if (!wsp || wsb < damc_recon_rows_workspace_bytes(B, n)) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  float* partial = reinterpret_cast<float*>(wsp);
  int rc = launch_recon_rows(xhat, x, B, n, partial, s);
  if (rc) return rc;
  return launch_finish(partial, (int)rr_nchunk(n), nullptr, 0, nullptr, 1.f, B, out, nullptr, nullptr, s);
}

extern "C" size_t damc_posterior_energy_workspace_bytes(const damc_generator_t* g, int B) {
  EnergyWs w;
  return energy_carve(g, B, &w) ? w.total : 0;
}

extern "C" int damc_posterior_energy(const damc_generator_t* g, const damc_ebm_t* ebm, const float* z, const float* x,
                                     int B, float recon_weight, float* terms, float* score, float* xhat, void* wsp,
                                     size_t wsb, void* stream) {
  if (!g || !z || !x || !terms || B <= 0) return DAMC_ERR_ARG;
  EnergyWs w;
  if (!energy_carve(g, B, &w)) return DAMC_ERR_ARG;
  if (ebm && ebm->nz != g->nz) return DAMC_ERR_ARG;
  if (!wsp || wsb < w.total) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  char* base = reinterpret_cast<char*>(wsp);
  float* xh = xhat ? xhat : reinterpret_cast<float*>(base + w.xhat);
  float* partial = reinterpret_cast<float*>(base + w.partial);
  float* ee = ebm ? reinterpret_cast<float*>(base + w.ebm_e) : nullptr;
  int rc = damc_generator_forward(g, z, B, xh, base, w.gen, stream);
  if (rc) return rc;
  if (ebm && (rc = damc_ebm_energy_grad(ebm, z, B, ee, reinterpret_cast<float*>(base + w.ebm_g), stream))) return rc;
  const long n = gen_row_elems(g);
  if ((rc = launch_recon_rows(xh, x, B, n, partial, s))) return rc;
  return launch_finish(partial, (int)rr_nchunk(n), z, g->nz, ee, recon_weight, B, nullptr, terms, score, s);
}
