// specnorm.hip — nn.utils.spectral_norm's compute_weight and its gradient for every spectral-norm layer of a net in
// grouped launches (the G and E updates of use_spc_norm=True generators and e_sn=True EBMs: workspace/src/
// diffusion_net.py:8-16, 21-44, 208-210; torch/nn/utils/spectral_norm.py SpectralNorm.compute_weight).
//
// A layer's weight_orig is read in place as [A][R][K]: matrix row = the middle index, column = a * K + k (Linear:
// [1][out][in]; ConvTranspose2d: [cin][cout][kh * kw], the hook's weight.permute(1, 0, 2, 3).reshape(cout, -1) without
// the copy).  For a fixed a the [R][K] slab is contiguous, so both products walk the same tiles:
//
//   tile = (a chunk, row chunk, column chunk); 256 threads = AL slab lanes x RL row lanes x CG column lanes, a lane
//   owns one VEC-wide column group (VEC = 4: 16-byte loads along K; 1 when K % 4 != 0 or a pointer is misaligned),
//   kRpl rows RL apart and kApl slabs AL apart.  CG = the power of two covering K / VEC (at most 256), RL = what is
//   left of the 256 lanes (at most the power of two covering R), AL = the rest.
//
// Forward, per power iteration (launch, grid):
//   1. sn_tile<W^T u>   every tile of every layer: row-chunk partials of W^T u          -> pt [row chunks][A K]
//   2. sn_finish_v      one block per layer: fixed-order sum of the partials, |.| in fp64, v <- t / max(|t|, eps)
//   3. sn_tile<W v>     every tile: (a chunk, column chunk) partials of W v             -> ps [a x column chunks][R]
//   4. sn_finish_u      one block per layer: s = sum of partials, u <- s / max(|s|, eps), sigma = u . s in fp64,
//                       and the copies u_used, v_used
// then 5. sn_scale: w_hat = w_orig / sigma (IEEE divide), every layer in one grid.  With no power iteration (eval
// mode) the launches are 3, 4 (u kept), 5.  One iteration: 5 launches for the whole net; the weights are read three
// times and written once (CIFAR ngf = 128: 4 x 76 MB, Infinity-Cache resident after the first pass).
// Backward: sn_bdot (per-block fp64 partials of <G, w_hat>), sn_bdot_finish (one block per layer), sn_bapply
// (G <- (G - <G, w_hat> u v^T) / sigma in place): 3 launches, G read twice and written once, w_hat read once.
//
// Every sum has a fixed order (lanes, then LDS in index order, then the partials in index order); nothing is atomic.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRpl = 8;             // rows per row lane of a tile
constexpr int kApl = 4;             // slabs per slab lane of a tile
constexpr int kFin = 1024;          // threads of the per-layer finishing blocks
constexpr int kEpb = kThreads * 16; // elements per block of the elementwise kernels

struct SnL {
  const float* w;
  float *u, *v, *what, *sigma, *uu, *vu, *g;
  float *pt, *ps, *sb;
  double* dp;
  int A, R, K;
  float eps;
  int vec, cg, rl, al, nrc, ncc, nac, tile0;  // tile decomposition; tile0: first tile of the layer in the grid
  int evec, eb0, neb;                         // elementwise kernels: 16-B accesses, first block, block count
};
struct SnTab {
  int n;
  int pad;
  SnL l[DAMC_SPECNORM_MAX_LAYERS];
};
static_assert(sizeof(SnTab) <= 2048, "kernel argument block");

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the block's total in every thread: lanes by xor shuffles, then the waves in index order
template <int NT>
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) t += sh[i];
  return t;
}

template <int VEC>
__device__ __forceinline__ void load_vec(const float* p, float (&o)[VEC]) {
  if constexpr (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    o[0] = t[0];
    o[1] = t[1];
    o[2] = t[2];
    o[3] = t[3];
  } else {
    o[0] = p[0];
  }
}

// MODE 0: row-chunk partials of W^T u.  MODE 1: (a chunk, column chunk) partials of W v.
template <int VEC, int MODE>
__device__ __forceinline__ void sn_tile_body(const SnL& L, int tb, float* lds) {
  const int CG = L.cg, RL = L.rl, AL = L.al, A = L.A, R = L.R, K = L.K;
  const int cc = tb % L.ncc;
  const int t2 = tb / L.ncc;
  const int rc = t2 % L.nrc;
  const int ac = t2 / L.nrc;
  const int tid = threadIdx.x;
  const int cg = tid & (CG - 1);
  const int t3 = tid / CG;
  const int rl = t3 & (RL - 1);
  const int al = t3 / RL;
  const int k0 = (cc * CG + cg) * VEC;
  const bool kok = k0 < K;  // VEC = 4 only with K % 4 == 0: the whole group is inside
  const int r0 = rc * RL * kRpl + rl;
  const int a0 = ac * AL * kApl + al;
  const float* __restrict__ W = L.w;
  if constexpr (MODE == 0) {
    float uv[kRpl];
#pragma unroll
    for (int j = 0; j < kRpl; ++j) {
      const int r = r0 + j * RL;
      uv[j] = r < R ? L.u[r] : 0.f;
    }
    const int nout = AL * CG * VEC;  // outputs of one pass: AL slabs x the tile's columns
    const long C = (long)A * K;
    for (int ai = 0; ai < kApl; ++ai) {
      const int a = a0 + ai * AL;
      float acc[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
      if (a < A && kok) {
#pragma unroll
        for (int j = 0; j < kRpl; ++j) {
          const int r = r0 + j * RL;
          if (r < R) {
            float wv[VEC];
            load_vec<VEC>(W + ((long)a * R + r) * K + k0, wv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = fmaf(wv[e], uv[j], acc[e]);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) lds[tid * VEC + e] = acc[e];
      __syncthreads();
      for (int o = tid; o < nout; o += kThreads) {
        const int alo = o / (CG * VEC);
        const int rem = o - alo * CG * VEC;
        float s = 0.f;
        for (int q = 0; q < RL; ++q) s += lds[(alo * RL + q) * CG * VEC + rem];
        const int aa = ac * AL * kApl + ai * AL + alo;
        const int kk = cc * CG * VEC + rem;
        if (aa < A && kk < K) L.pt[(long)rc * C + (long)aa * K + kk] = s;
      }
      __syncthreads();
    }
  } else {
    float acc[kRpl];
#pragma unroll
    for (int j = 0; j < kRpl; ++j) acc[j] = 0.f;
    if (kok) {
      for (int ai = 0; ai < kApl; ++ai) {
        const int a = a0 + ai * AL;
        if (a >= A) break;
        float vv[VEC];
        load_vec<VEC>(L.v + (long)a * K + k0, vv);
#pragma unroll
        for (int j = 0; j < kRpl; ++j) {
          const int r = r0 + j * RL;
          if (r < R) {
            float wv[VEC];
            load_vec<VEC>(W + ((long)a * R + r) * K + k0, wv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[j] = fmaf(wv[e], vv[e], acc[j]);
          }
        }
      }
    }
    // the column lanes of a row are adjacent lanes: xor shuffles inside the wave, LDS across the rest
    const int width = CG < 64 ? CG : 64;
    for (int o = width >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int j = 0; j < kRpl; ++j) acc[j] += __shfl_xor(acc[j], o, 64);
    }
    const int G = kThreads / width;  // groups = (al, rl, column wave)
    const int CGW = CG / width;
    if ((tid & (width - 1)) == 0) {
      const int gi = tid / width;
#pragma unroll
      for (int j = 0; j < kRpl; ++j) lds[j * G + gi] = acc[j];
    }
    __syncthreads();
    for (int o = tid; o < RL * kRpl; o += kThreads) {
      const int rlo = o & (RL - 1);
      const int j = o / RL;
      float s = 0.f;
      for (int alo = 0; alo < AL; ++alo)
        for (int q = 0; q < CGW; ++q) s += lds[j * G + (alo * RL + rlo) * CGW + q];
      const int r = rc * RL * kRpl + rlo + j * RL;
      if (r < R) L.ps[(long)(ac * L.ncc + cc) * R + r] = s;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void sn_tile_kernel(SnTab t) {
  __shared__ float lds[kThreads * kRpl];
  int i = 0;
  while (i + 1 < t.n && (int)blockIdx.x >= t.l[i + 1].tile0) ++i;
  const SnL& L = t.l[i];
  const int tb = (int)blockIdx.x - L.tile0;
  if (L.vec == 4)
    sn_tile_body<4, MODE>(L, tb, lds);
  else
    sn_tile_body<1, MODE>(L, tb, lds);
}

__global__ __launch_bounds__(kFin) void sn_finish_v_kernel(SnTab t) {
  __shared__ double sh[kFin / 64];
  const SnL& L = t.l[blockIdx.x];
  const int C = L.A * L.K;
  const int tid = threadIdx.x;
  double ss = 0.0;
  for (int c = tid; c < C; c += kFin) {
    double s = 0.0;
    for (int q = 0; q < L.nrc; ++q) s += (double)L.pt[(long)q * C + c];
    const float tf = (float)s;
    L.v[c] = tf;
    ss += (double)tf * (double)tf;
  }
  const double tot = block_sum_d<kFin>(ss, sh);
  const float den = fmaxf((float)sqrt(tot), L.eps);
  for (int c = tid; c < C; c += kFin) L.v[c] = L.v[c] / den;  // the thread's own stores
}

__global__ __launch_bounds__(kFin) void sn_finish_u_kernel(SnTab t, int update) {
  __shared__ double sh[kFin / 64];
  const SnL& L = t.l[blockIdx.x];
  const int R = L.R, C = L.A * L.K;
  const int np = L.nac * L.ncc;
  const int tid = threadIdx.x;
  double ss = 0.0;
  for (int r = tid; r < R; r += kFin) {
    double s = 0.0;
    for (int q = 0; q < np; ++q) s += (double)L.ps[(long)q * R + r];
    const float sf = (float)s;
    L.sb[r] = sf;
    ss += (double)sf * (double)sf;
  }
  if (update) {
    const double tot = block_sum_d<kFin>(ss, sh);
    const float den = fmaxf((float)sqrt(tot), L.eps);
    for (int r = tid; r < R; r += kFin) L.u[r] = L.sb[r] / den;
  }
  double dot = 0.0;
  for (int r = tid; r < R; r += kFin) {
    const float ur = L.u[r];
    L.uu[r] = ur;
    dot += (double)ur * (double)L.sb[r];
  }
  const double sig = block_sum_d<kFin>(dot, sh);
  if (tid == 0) L.sigma[0] = (float)sig;
  for (int c = tid; c < C; c += kFin) L.vu[c] = L.v[c];
}

__device__ __forceinline__ const SnL& elem_layer(const SnTab& t, int& lb) {
  int i = 0;
  while (i + 1 < t.n && (int)blockIdx.x >= t.l[i + 1].eb0) ++i;
  lb = (int)blockIdx.x - t.l[i].eb0;
  return t.l[i];
}

__global__ __launch_bounds__(kThreads) void sn_scale_kernel(SnTab t) {
  int lb;
  const SnL& L = elem_layer(t, lb);
  const int n = L.A * L.R * L.K;
  const int base = lb * kEpb;
  const float sig = L.sigma[0];
  if (L.evec) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = base + (it * kThreads + (int)threadIdx.x) * 4;
      if (i < n) {
        f32x4 w = *reinterpret_cast<const f32x4*>(L.w + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = w[e] / sig;
        *reinterpret_cast<f32x4*>(L.what + i) = w;
      }
    }
  } else {
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int i = base + it * kThreads + (int)threadIdx.x;
      if (i < n) L.what[i] = L.w[i] / sig;
    }
  }
}

__global__ __launch_bounds__(kThreads) void sn_bdot_kernel(SnTab t) {
  __shared__ double sh[kThreads / 64];
  int lb;
  const SnL& L = elem_layer(t, lb);
  const int n = L.A * L.R * L.K;
  const int base = lb * kEpb;
  float acc = 0.f;
  if (L.evec) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = base + (it * kThreads + (int)threadIdx.x) * 4;
      if (i < n) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(L.g + i);
        const f32x4 w = *reinterpret_cast<const f32x4*>(L.what + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(g[e], w[e], acc);
      }
    }
  } else {
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int i = base + it * kThreads + (int)threadIdx.x;
      if (i < n) acc = fmaf(L.g[i], L.what[i], acc);
    }
  }
  const double tot = block_sum_d<kThreads>((double)acc, sh);
  if (threadIdx.x == 0) L.dp[lb] = tot;
}

__global__ __launch_bounds__(kThreads) void sn_bdot_finish_kernel(SnTab t) {
  __shared__ double sh[kThreads / 64];
  const SnL& L = t.l[blockIdx.x];
  double s = 0.0;
  for (int i = threadIdx.x; i < L.neb; i += kThreads) s += L.dp[i];
  const double tot = block_sum_d<kThreads>(s, sh);
  if (threadIdx.x == 0) L.dp[L.neb] = tot;
}

__device__ __forceinline__ float bapply_elem(float g, float du, float v, float sig) { return (g - du * v) / sig; }

__global__ __launch_bounds__(kThreads) void sn_bapply_kernel(SnTab t) {
  int lb;
  const SnL& L = elem_layer(t, lb);
  const int R = L.R, K = L.K;
  const int n = L.A * R * K;
  const int base = lb * kEpb;
  const float d = (float)L.dp[L.neb];
  const float sig = L.sigma[0];
  if (L.evec) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = base + (it * kThreads + (int)threadIdx.x) * 4;
      if (i < n) {
        const int ar = i / K, k = i - ar * K;  // K % 4 == 0: the four elements share a and r
        const int a = ar / R, r = ar - a * R;
        const float du = d * L.uu[r];
        const f32x4 v = *reinterpret_cast<const f32x4*>(L.vu + (long)a * K + k);
        f32x4 g = *reinterpret_cast<const f32x4*>(L.g + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = bapply_elem(g[e], du, v[e], sig);
        *reinterpret_cast<f32x4*>(L.g + i) = g;
      }
    }
  } else {
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int i = base + it * kThreads + (int)threadIdx.x;
      if (i < n) {
        const int ar = i / K, k = i - ar * K;
        const int a = ar / R, r = ar - a * R;
        L.g[i] = bapply_elem(L.g[i], d * L.uu[r], L.vu[(long)a * K + k], sig);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------- host side
int pow2_cover(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

struct TilePlan {
  int cg, rl, al, nrc, ncc, nac;
};

TilePlan tile_plan(int A, int R, int K, int vec) {
  TilePlan p;
  const int kg = (K + vec - 1) / vec;
  p.cg = pow2_cover(kg) < kThreads ? pow2_cover(kg) : kThreads;
  const int left = kThreads / p.cg;
  p.rl = pow2_cover(R) < left ? pow2_cover(R) : left;
  p.al = left / p.rl;
  p.nrc = (R + p.rl * kRpl - 1) / (p.rl * kRpl);
  p.ncc = (kg + p.cg - 1) / p.cg;
  p.nac = (A + p.al * kApl - 1) / (p.al * kApl);
  return p;
}

bool al16h(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

bool table_ok(const damc_specnorm_layer_t* l, int n) {
  if (!l || n < 1 || n > DAMC_SPECNORM_MAX_LAYERS) return false;
  for (int i = 0; i < n; ++i) {
    if (l[i].a < 1 || l[i].r < 1 || l[i].k < 1) return false;
    if ((long long)l[i].a * l[i].r * l[i].k > 0x7fffffffLL - 2 * kEpb) return false;  // flat int indices
    if (!l[i].w_hat || !l[i].sigma || !l[i].u_used || !l[i].v_used) return false;
  }
  return true;
}

struct WsLayer {
  size_t dp, pt, ps, sb;
};

// per layer: the <G, w_hat> partials and total (fp64), the W^T u and W v partials sized for either VEC, and W v.
// The layout goes by the extents alone, so the forward, the backward and the size query agree whatever the pointers.
size_t ws_layout(const damc_specnorm_layer_t* l, int n, WsLayer* out) {
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    const int A = l[i].a, R = l[i].r, K = l[i].k;
    const size_t neb = ((size_t)A * R * K + kEpb - 1) / kEpb;
    size_t pt = 0, ps = 0;
    for (int vec = 1; vec <= ((K % 4 == 0) ? 4 : 1); vec += 3) {
      const TilePlan p = tile_plan(A, R, K, vec);
      const size_t a = (size_t)p.nrc * A * K, b = (size_t)p.nac * p.ncc * R;
      pt = a > pt ? a : pt;
      ps = b > ps ? b : ps;
    }
    WsLayer w;
    w.dp = off;
    off += up16((neb + 1) * sizeof(double));
    w.pt = off;
    off += up16(pt * sizeof(float));
    w.ps = off;
    off += up16(ps * sizeof(float));
    w.sb = off;
    off += up16((size_t)R * sizeof(float));
    if (out) out[i] = w;
  }
  return off;
}

// fills the kernels' table; forward: vec / evec from w_orig, v, w_hat; backward: evec from g, w_hat, v_used
int build_table(const damc_specnorm_layer_t* l, int n, float* const* g, void* ws, size_t ws_bytes, SnTab* t,
                int* ntiles, int* nebs) {
  if (!table_ok(l, n) || !ws) return DAMC_ERR_ARG;
  if (!al16h(ws)) return DAMC_ERR_ARG;
  WsLayer wl[DAMC_SPECNORM_MAX_LAYERS];
  if (ws_layout(l, n, wl) > ws_bytes) return DAMC_ERR_WORKSPACE;
  char* base = static_cast<char*>(ws);
  int tile0 = 0, eb0 = 0;
  t->n = n;
  t->pad = 0;
  for (int i = 0; i < n; ++i) {
    SnL& L = t->l[i];
    L.w = l[i].w_orig;
    L.u = l[i].u;
    L.v = l[i].v;
    L.what = l[i].w_hat;
    L.sigma = l[i].sigma;
    L.uu = l[i].u_used;
    L.vu = l[i].v_used;
    L.g = g ? g[i] : nullptr;
    L.dp = reinterpret_cast<double*>(base + wl[i].dp);
    L.pt = reinterpret_cast<float*>(base + wl[i].pt);
    L.ps = reinterpret_cast<float*>(base + wl[i].ps);
    L.sb = reinterpret_cast<float*>(base + wl[i].sb);
    L.A = l[i].a;
    L.R = l[i].r;
    L.K = l[i].k;
    L.eps = l[i].eps;
    const bool k4 = L.K % 4 == 0;
    if (g) {
      L.vec = 1;
      L.evec = k4 && al16h(L.g) && al16h(L.what) && al16h(L.vu);
    } else {
      if (!L.w || !L.u || !L.v) return DAMC_ERR_ARG;
      L.vec = (k4 && al16h(L.w) && al16h(L.v)) ? 4 : 1;
      L.evec = k4 && al16h(L.w) && al16h(L.what);
    }
    const TilePlan p = tile_plan(L.A, L.R, L.K, L.vec);
    L.cg = p.cg;
    L.rl = p.rl;
    L.al = p.al;
    L.nrc = p.nrc;
    L.ncc = p.ncc;
    L.nac = p.nac;
    L.tile0 = tile0;
    tile0 += p.nac * p.nrc * p.ncc;
    L.eb0 = eb0;
    L.neb = (g && !L.g) ? 0 : (int)(((size_t)L.A * L.R * L.K + kEpb - 1) / kEpb);
    eb0 += L.neb;
  }
  *ntiles = tile0;
  *nebs = eb0;
  return 0;
}

}  // namespace

extern "C" size_t damc_specnorm_workspace_bytes(const damc_specnorm_layer_t* layers, int n) {
  if (!table_ok(layers, n)) return 0;
  return ws_layout(layers, n, nullptr);
}

extern "C" int damc_specnorm_forward(const damc_specnorm_layer_t* layers, int n, int power_iterations, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  DAMC_REQUIRE(power_iterations >= 0);
  SnTab t;
  int ntiles = 0, nebs = 0;
  const int rc = build_table(layers, n, nullptr, workspace, workspace_bytes, &t, &ntiles, &nebs);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  for (int it = 0; it < power_iterations; ++it) {
    hipLaunchKernelGGL(sn_tile_kernel<0>, dim3(ntiles), dim3(kThreads), 0, s, t);
    hipLaunchKernelGGL(sn_finish_v_kernel, dim3(n), dim3(kFin), 0, s, t);
    hipLaunchKernelGGL(sn_tile_kernel<1>, dim3(ntiles), dim3(kThreads), 0, s, t);
    hipLaunchKernelGGL(sn_finish_u_kernel, dim3(n), dim3(kFin), 0, s, t, 1);
  }
  if (power_iterations == 0) {
    hipLaunchKernelGGL(sn_tile_kernel<1>, dim3(ntiles), dim3(kThreads), 0, s, t);
    hipLaunchKernelGGL(sn_finish_u_kernel, dim3(n), dim3(kFin), 0, s, t, 0);
  }
  hipLaunchKernelGGL(sn_scale_kernel, dim3(nebs), dim3(kThreads), 0, s, t);
  DAMC_LAUNCH_CHECK();
  return 0;
}

extern "C" int damc_specnorm_backward(const damc_specnorm_layer_t* layers, int n, float* const* g, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  DAMC_REQUIRE(g != nullptr);
  SnTab t;
  int ntiles = 0, nebs = 0;
  const int rc = build_table(layers, n, g, workspace, workspace_bytes, &t, &ntiles, &nebs);
  if (rc) return rc;
  if (nebs == 0) return 0;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(sn_bdot_kernel, dim3(nebs), dim3(kThreads), 0, s, t);
  hipLaunchKernelGGL(sn_bdot_finish_kernel, dim3(n), dim3(kThreads), 0, s, t);
  hipLaunchKernelGGL(sn_bapply_kernel, dim3(nebs), dim3(kThreads), 0, s, t);
  DAMC_LAUNCH_CHECK();
  return 0;
}
