// mlp.hip — a small MLP of nn.Linear layers as one launch (damc_mlp_forward): the toy amortizer's encoder
// (_netQ_U_toy.encoder, workspace/toy_example/src/diffusion_net.py:166-174: Linear(2,128)-ReLU x3, Linear(128, nxemb))
// and its prior_emb (:180-184: Linear(nz,128)-LeakyReLU-Linear(128, nxemb)) at nz = 2.
//
// One 256-thread workgroup owns 16 rows; the activations ping-pong between two LDS images, and the weights are read
// where PyTorch keeps them ((out, in), k contiguous), so there is no packing and no workspace.  A layer whose K is a
// multiple of 16 (and whose weight is 16-B aligned) runs on v_mfma_f32_16x16x4_f32: wave w takes the 16-column tiles
// w, w + 4, ..., each on two accumulator chains (even / odd k-groups), with the k-permutation of sweep_chain.hip (MFMA
// step s of k-group g reads k = 16 g + 4 (lane >> 4) + s on both operands, one f32x4 load each).  Any other K (the
// toy's K = 2 input layers) is plain FMAs, one (row, column) per thread.
//
// Training (damc_mlp_train_forward / _backward; the same two MLPs inside calculate_loss, :241-263, six updates per
// iteration of toy_example.py:209-219): the forward kernel instantiated with SAVE keeps every hidden layer's
// post-activation rows, and the backward is two launches -- a 16-rows-per-workgroup dgrad chain through LDS
// (mlp_dgrad_kernel) and one launch for every layer's dW and db (mlp_wgrad_kernel).  No input gradient.
#include "common.h"

namespace {

constexpr int ML_TM = 16, ML_THREADS = 256, ML_MAXW = DAMC_MLP_MAX_WIDTH;
constexpr int ML_LD = ML_MAXW + 4;  // image row stride: the 16 rows of a ds_read_b128 on distinct banks

__device__ __forceinline__ float ml_act(float v, int act, float slope) {
  if (act == DAMC_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == DAMC_ACT_LRELU) return v > 0.f ? v : v * slope;
  return v;
}

// SAVE: every hidden layer's post-activation rows also go to `saved` (layer l's (B, dout_l) block at float offset
// B * (dout_0 + ... + dout_{l-1})), the training forward; the arithmetic is the same instantiation-independent code,
// so `out` is bitwise the plain forward's
template <bool SAVE>
__global__ __launch_bounds__(ML_THREADS) void mlp_kernel(damc_mlp_t d, const float* __restrict__ x, int B,
                                                         float* __restrict__ out, float* __restrict__ saved) {
  __shared__ __attribute__((aligned(16))) float img[2][ML_TM][ML_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * ML_TM;
  const int k0 = d.layers[0].din;
  for (int i = tid; i < ML_TM * k0; i += ML_THREADS) {
    const int r = i / k0, c = i - r * k0;
    img[0][r][c] = r0 + r < B ? x[(long)(r0 + r) * k0 + c] : 0.f;
  }
  __syncthreads();
  for (int l = 0; l < d.n_layers; ++l) {
    const damc_mlp_layer_t& L = d.layers[l];
    const float(*src)[ML_LD] = img[l & 1];
    float(*dst)[ML_LD] = img[(l + 1) & 1];
    const bool last = l + 1 == d.n_layers;
    const int K = L.din, N = L.dout;
    float* sv = nullptr;  // this layer's block of `saved`
    if (SAVE && !last) {
      long o = 0;
      for (int j = 0; j < l; ++j) o += d.layers[j].dout;
      sv = saved + (long)B * o;
    }
    if ((K & 15) == 0 && ((uintptr_t)L.w & 15) == 0) {
      for (int t = wave; t * 16 < N; t += 4) {
        const int col = t * 16 + m;
        const bool cok = col < N;
        const float* wrow = L.w + (long)(cok ? col : 0) * K + 4 * q;
        const float* xr = &src[m][4 * q];
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < K; g += 32) {
          const bool two = g + 16 < K;
          f32x4 w0 = *reinterpret_cast<const f32x4*>(wrow + g);
          f32x4 w1 = *reinterpret_cast<const f32x4*>(wrow + (two ? g + 16 : g));
          const f32x4 x0 = *reinterpret_cast<const f32x4*>(xr + g);
          const f32x4 x1 = *reinterpret_cast<const f32x4*>(xr + (two ? g + 16 : g));
          if (!cok) w0 = w1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[e], w0[e], a0, 0, 0, 0);
            if (two) a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[e], w1[e], a1, 0, 0, 0);
          }
        }
        // C layout 16x16x4: column = lane & 15, rows 4 (lane >> 4) + r
        const f32x4 s = a0 + a1;
        const float bias = (cok && L.bias) ? L.bias[col] : 0.f;
        if (cok) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int lr = 4 * q + r;
            const float v = ml_act(s[r] + bias, L.act, L.slope);
            if (!last) dst[lr][col] = v;
            else if (r0 + lr < B) out[(long)(r0 + lr) * N + col] = v;
            if (SAVE && !last && r0 + lr < B) sv[(long)(r0 + lr) * N + col] = v;
          }
        }
      }
    } else {
      for (int i = tid; i < ML_TM * N; i += ML_THREADS) {
        const int r = i / N, c = i - r * N;
        const float* wrow = L.w + (long)c * K;
        float v = 0.f;
        for (int k = 0; k < K; ++k) v = __builtin_fmaf(src[r][k], wrow[k], v);
        if (L.bias) v += L.bias[c];
        v = ml_act(v, L.act, L.slope);
        if (!last) dst[r][c] = v;
        else if (r0 + r < B) out[(long)(r0 + r) * N + c] = v;
        if (SAVE && !last && r0 + r < B) sv[(long)(r0 + r) * N + c] = v;
      }
    }
    __syncthreads();
  }
}

int mlp_validate(const damc_mlp_t* d) {
  if (!d || d->n_layers < 1 || d->n_layers > DAMC_MLP_MAX_LAYERS) return DAMC_ERR_ARG;
  for (int l = 0; l < d->n_layers; ++l) {
    const damc_mlp_layer_t& L = d->layers[l];
    if (L.din < 1 || L.dout < 1 || !L.w) return DAMC_ERR_ARG;
    if (l && L.din != d->layers[l - 1].dout) return DAMC_ERR_ARG;
    if (L.act != DAMC_ACT_NONE && L.act != DAMC_ACT_RELU && L.act != DAMC_ACT_LRELU) return DAMC_ERR_ARG;
    if (L.din > ML_MAXW || L.dout > ML_MAXW) return DAMC_ERR_UNSUPPORTED;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ training
// g * act'(pre) read from the post-activation y: sign(y) is sign(pre) for RELU and for LRELU with slope >= 0 (the
// train entry points refuse a negative slope)
__device__ __forceinline__ float ml_dact(float g, float y, int act, float slope) {
  if (act == DAMC_ACT_RELU) return y > 0.f ? g : 0.f;
  if (act == DAMC_ACT_LRELU) return y > 0.f ? g : g * slope;
  return g;
}

// dgrad chain, 16 rows per workgroup: dY_{l-1} = (dY_l . W_l) * act'_{l-1}(saved_{l-1}) for l = n-1 .. 1, dY_{n-1} =
// grad_out (the last layer has no activation).  dY_l's image is in LDS; W_l (dout_l, din_l) is read where PyTorch keeps
// it: the contraction runs over its rows, so lane (m, q) of an MFMA step e reads W[o0 + 4 q + e][col m] (16 lanes on 64
// contiguous bytes) against dY[row m][o0 + 4 q + e] (one ds_read_b128), the k-permutation of the forward.  A dout_l
// that is no multiple of 16 is plain FMAs.  Every dY_l, l < n-1, goes to `dy` in saved's layout for the wgrad launch.
__global__ __launch_bounds__(ML_THREADS) void mlp_dgrad_kernel(damc_mlp_t d, const float* __restrict__ saved,
                                                               const float* __restrict__ gout, int B,
                                                               float* __restrict__ dy) {
  __shared__ __attribute__((aligned(16))) float img[2][ML_TM][ML_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * ML_TM;
  const int nl = d.n_layers, n_last = d.layers[nl - 1].dout;
  for (int i = tid; i < ML_TM * n_last; i += ML_THREADS) {
    const int r = i / n_last, c = i - r * n_last;
    img[0][r][c] = r0 + r < B ? gout[(long)(r0 + r) * n_last + c] : 0.f;
  }
  __syncthreads();
  int pp = 0;
  for (int l = nl - 1; l >= 1; --l) {
    const damc_mlp_layer_t& L = d.layers[l];
    const damc_mlp_layer_t& P = d.layers[l - 1];
    const int N = L.dout, K = L.din;  // contraction over N; K columns out
    long o = 0;
    for (int j = 0; j + 1 < l; ++j) o += d.layers[j].dout;
    const float* sv = saved + (long)B * o;  // layer l-1's post-activation rows (B, K)
    float* dg = dy + (long)B * o;
    const float(*src)[ML_LD] = img[pp];
    float(*dst)[ML_LD] = img[pp ^ 1];
    if ((N & 15) == 0) {
      for (int t = wave; t * 16 < K; t += 4) {
        const int col = t * 16 + m;
        const bool cok = col < K;
        const float* wc = L.w + (cok ? col : 0);
        const float* gr = &src[m][4 * q];
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < N; g += 32) {
          const bool two = g + 16 < N;
          const int g1 = two ? g + 16 : g;
          const f32x4 x0 = *reinterpret_cast<const f32x4*>(gr + g);
          const f32x4 x1 = *reinterpret_cast<const f32x4*>(gr + g1);
          f32x4 w0, w1;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            w0[e] = wc[(long)(g + 4 * q + e) * K];
            w1[e] = wc[(long)(g1 + 4 * q + e) * K];
          }
          if (!cok) w0 = w1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[e], w0[e], a0, 0, 0, 0);
            if (two) a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[e], w1[e], a1, 0, 0, 0);
          }
        }
        const f32x4 s = a0 + a1;
        if (cok) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int lr = 4 * q + r;
            const bool rok = r0 + lr < B;
            const float y = rok ? sv[(long)(r0 + lr) * K + col] : 0.f;
            const float v = ml_dact(s[r], y, P.act, P.slope);
            dst[lr][col] = v;
            if (rok) dg[(long)(r0 + lr) * K + col] = v;
          }
        }
      }
    } else {
      for (int i = tid; i < ML_TM * K; i += ML_THREADS) {
        const int r = i / K, c = i - r * K;
        float v = 0.f;
        for (int k = 0; k < N; ++k) v = __builtin_fmaf(src[r][k], L.w[(long)k * K + c], v);
        const bool rok = r0 + r < B;
        v = ml_dact(v, rok ? sv[(long)(r0 + r) * K + c] : 0.f, P.act, P.slope);
        dst[r][c] = v;
        if (rok) dg[(long)(r0 + r) * K + c] = v;
      }
    }
    __syncthreads();
    pp ^= 1;
  }
}

// every layer's dW_l (dout_l, din_l) = dY_l^T . X_l and db_l = column sums of dY_l in ONE launch: a 4-wave workgroup
// owns one 16 x 16 tile of one layer's dW, the B rows split over the waves in four contiguous runs and walked in order,
// the wave partials summed ((w0 + w1) + w2) + w3 -- no atomics, the same bits every run.  Lane (m, q) of MFMA step e
// reads dY[n0 + 4 q + e][o0 + m] and X[n0 + 4 q + e][i0 + m] (scalar loads: any B, any din, no alignment asked); the
// i0 = 0 tiles carry a second chain against ones for db.
struct MlpWgrad {
  int n;
  int tile_end[DAMC_MLP_MAX_LAYERS];
  int dout[DAMC_MLP_MAX_LAYERS], din[DAMC_MLP_MAX_LAYERS], nti[DAMC_MLP_MAX_LAYERS];
  const float* dy[DAMC_MLP_MAX_LAYERS];
  const float* x[DAMC_MLP_MAX_LAYERS];
  float* dw[DAMC_MLP_MAX_LAYERS];
  float* db[DAMC_MLP_MAX_LAYERS];
};

__global__ __launch_bounds__(ML_THREADS) void mlp_wgrad_kernel(MlpWgrad g, int B) {
  __shared__ f32x4 red[3][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blk = blockIdx.x;
  int li = 0;
  while (li + 1 < g.n && blk >= g.tile_end[li]) ++li;  // workgroup-uniform
  const int tile = blk - (li ? g.tile_end[li - 1] : 0);
  const int O = g.dout[li], I = g.din[li], nti = g.nti[li];
  const int to = tile / nti, ti = tile - to * nti;
  const int m = lane & 15, q = lane >> 4;
  const int orow = to * 16 + m, icol = ti * 16 + m;
  float* dw = g.dw[li];
  float* db = ti == 0 ? g.db[li] : nullptr;
  const bool ook = orow < O, iok = dw && icol < I;
  const float* ac = g.dy[li] + (ook ? orow : 0);
  const float* bc = g.x[li] + (iok ? icol : 0);
  const int k16 = (B + 15) >> 4, per = (k16 + 3) >> 2;
  const int kb = wave * per * 16, ke = min(B, kb + per * 16);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += 16) {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // loads from clamped (valid) addresses, then zeroed: no load sits in a branch
      const int n = k0 + 4 * q + e;
      const bool in = n < ke;
      const long nn = in ? n : 0;
      a[e] = ac[nn * O];
      b[e] = bc[nn * I];
      if (!(in && ook)) a[e] = 0.f;
      if (!(in && iok)) b[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
      if (db) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], 1.f, accb, 0, 0, 0);
    }
  }
  if (wave) {
    red[wave - 1][0][lane] = acc;
    red[wave - 1][1][lane] = accb;
  }
  __syncthreads();
  if (wave) return;
  acc = ((acc + red[0][0][lane]) + red[1][0][lane]) + red[2][0][lane];
  accb = ((accb + red[0][1][lane]) + red[1][1][lane]) + red[2][1][lane];
  // C layout 16x16x4: column = lane & 15 (i), rows 4 (lane >> 4) + r (o)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = to * 16 + 4 * q + r;
    if (row >= O) continue;
    if (iok) dw[(long)row * I + icol] = acc[r];
    if (db && m == 0) db[row] = accb[r];
  }
}

// what the training entry points take: mlp_validate's descriptors whose last layer has no activation (dY of the last
// layer is grad_out itself) and whose LRELU slopes are >= 0 (act' from the sign of the saved post-activation)
int mlp_train_validate(const damc_mlp_t* d) {
  const int rc = mlp_validate(d);
  if (rc) return rc;
  for (int l = 0; l < d->n_layers; ++l)
    if (d->layers[l].act == DAMC_ACT_LRELU && !(d->layers[l].slope >= 0.f)) return DAMC_ERR_ARG;
  if (d->layers[d->n_layers - 1].act != DAMC_ACT_NONE) return DAMC_ERR_UNSUPPORTED;
  return 0;
}

// floats of the hidden layers' (batch, dout_l) blocks, l < n-1: the layout of `saved` and of the backward's dY scratch
size_t mlp_hidden_floats(const damc_mlp_t* d, int batch) {
  size_t n = 0;
  for (int l = 0; l + 1 < d->n_layers; ++l) n += (size_t)batch * d->layers[l].dout;
  return n ? n : 1;
}

}  // namespace

extern "C" size_t damc_mlp_train_saved_floats(const damc_mlp_t* d, int batch) {
  if (mlp_train_validate(d) || batch <= 0) return 0;
  return mlp_hidden_floats(d, batch);
}

extern "C" size_t damc_mlp_train_workspace_bytes(const damc_mlp_t* d, int batch) {
  if (mlp_train_validate(d) || batch <= 0) return 0;
  return mlp_hidden_floats(d, batch) * sizeof(float);
}

extern "C" int damc_mlp_train_forward(const damc_mlp_t* d, const float* x, int batch, float* saved, float* out,
                                      void* stream) {
  const int rc = mlp_train_validate(d);
  if (rc) return rc;
  if (!x || !out || !saved || batch <= 0) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  double flops = 0.0;
  for (int l = 0; l < d->n_layers; ++l) flops += 2.0 * batch * d->layers[l].din * d->layers[l].dout;
  ProfScope ps("mlp_train_fwd", flops, s);
  hipLaunchKernelGGL(mlp_kernel<true>, dim3((unsigned)((batch + ML_TM - 1) / ML_TM)), dim3(ML_THREADS), 0, s, *d, x, batch,
                     out, saved);
  return (int)hipGetLastError();
}

extern "C" int damc_mlp_train_backward(const damc_mlp_t* d, const float* x, const float* saved, const float* grad_out,
                                       int batch, const damc_mlp_grads_t* grads, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  const int rc = mlp_train_validate(d);
  if (rc) return rc;
  if (!x || !saved || !grad_out || !grads || batch <= 0) return DAMC_ERR_ARG;
  if (!workspace || workspace_bytes < mlp_hidden_floats(d, batch) * sizeof(float)) return DAMC_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  float* dy = reinterpret_cast<float*>(workspace);
  const int nl = d->n_layers;
  double flops = 0.0;
  for (int l = 0; l < nl; ++l) flops += 2.0 * batch * d->layers[l].din * d->layers[l].dout;
  ProfScope ps("mlp_train_bwd", 2.0 * flops, s);
  if (nl > 1)
    hipLaunchKernelGGL(mlp_dgrad_kernel, dim3((unsigned)((batch + ML_TM - 1) / ML_TM)), dim3(ML_THREADS), 0, s, *d, saved,
                       grad_out, batch, dy);
  MlpWgrad g{};
  int tot = 0;
  size_t off = 0;  // floats before layer l's hidden block
  for (int l = 0; l < nl; ++l) {
    const damc_mlp_layer_t& L = d->layers[l];
    const size_t prev = l ? off - (size_t)batch * d->layers[l - 1].dout : 0;
    if (grads->w[l] || grads->b[l]) {
      const int i = g.n++;
      g.dout[i] = L.dout;
      g.din[i] = L.din;
      g.nti[i] = grads->w[l] ? (L.din + 15) / 16 : 1;
      g.dy[i] = l + 1 == nl ? grad_out : dy + off;
      g.x[i] = l ? saved + prev : x;
      g.dw[i] = grads->w[l];
      g.db[i] = grads->b[l];
      tot += ((L.dout + 15) / 16) * g.nti[i];
      g.tile_end[i] = tot;
    }
    off += (size_t)batch * L.dout;
  }
  if (g.n) hipLaunchKernelGGL(mlp_wgrad_kernel, dim3((unsigned)tot), dim3(ML_THREADS), 0, s, g, batch);
  return (int)hipGetLastError();
}

extern "C" int damc_mlp_forward(const damc_mlp_t* d, const float* x, int batch, float* out, void* stream) {
  const int rc = mlp_validate(d);
  if (rc) return rc;
  if (!x || !out || batch <= 0) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  double flops = 0.0;
  for (int l = 0; l < d->n_layers; ++l) flops += 2.0 * batch * d->layers[l].din * d->layers[l].dout;
  ProfScope ps("mlp", flops, s);
  hipLaunchKernelGGL(mlp_kernel<false>, dim3((unsigned)((batch + ML_TM - 1) / ML_TM)), dim3(ML_THREADS), 0, s, *d, x, batch,
                     out, (float*)nullptr);
  return (int)hipGetLastError();
}
