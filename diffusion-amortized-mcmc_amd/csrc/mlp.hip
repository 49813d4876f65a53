// mlp.hip — a small MLP of nn.Linear layers as one launch (damc_mlp_forward): the toy amortizer's encoder
// (_netQ_U_toy.encoder, workspace/toy_example/src/diffusion_net.py:166-174: Linear(2,128)-ReLU x3, Linear(128, nxemb))
// and its prior_emb (:180-184: Linear(nz,128)-LeakyReLU-Linear(128, nxemb)) at nz = 2.
//
// One 256-thread workgroup owns 16 rows; the activations ping-pong between two LDS images, and the weights are read
// where PyTorch keeps them ((out, in), k contiguous), so there is no packing and no workspace.  A layer whose K is a
// multiple of 16 (and whose weight is 16-B aligned) runs on v_mfma_f32_16x16x4_f32: wave w takes the 16-column tiles
// w, w + 4, ..., each on two accumulator chains (even / odd k-groups), with the k-permutation of denoiser.hip (MFMA
// step s of k-group g reads k = 16 g + 4 (lane >> 4) + s on both operands, one f32x4 load each).  Any other K (the
// toy's K = 2 input layers) is plain FMAs, one (row, column) per thread.
#include "common.h"

namespace {

constexpr int ML_TM = 16, ML_THREADS = 256, ML_MAXW = DAMC_MLP_MAX_WIDTH;
constexpr int ML_LD = ML_MAXW + 4;  // image row stride: the 16 rows of a ds_read_b128 on distinct banks

__device__ __forceinline__ float ml_act(float v, int act, float slope) {
  if (act == DAMC_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == DAMC_ACT_LRELU) return v > 0.f ? v : v * slope;
  return v;
}

__global__ __launch_bounds__(ML_THREADS) void mlp_kernel(damc_mlp_t d, const float* __restrict__ x, int B,
                                                         float* __restrict__ out) {
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

}  // namespace

extern "C" int damc_mlp_forward(const damc_mlp_t* d, const float* x, int batch, float* out, void* stream) {
  const int rc = mlp_validate(d);
  if (rc) return rc;
  if (!x || !out || batch <= 0) return DAMC_ERR_ARG;
  hipStream_t s = as_stream(stream);
  double flops = 0.0;
  for (int l = 0; l < d->n_layers; ++l) flops += 2.0 * batch * d->layers[l].din * d->layers[l].dout;
  ProfScope ps("mlp", flops, s);
  hipLaunchKernelGGL(mlp_kernel, dim3((unsigned)((batch + ML_TM - 1) / ML_TM)), dim3(ML_THREADS), 0, s, *d, x, batch, out);
  return (int)hipGetLastError();
}
