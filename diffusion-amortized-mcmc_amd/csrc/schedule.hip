// schedule.hip — the glue of a training iteration that the reference driver runs on the host, as device-gated launches:
// the iteration counter, the EMA of the amortizer's target network and the learning-rate decay.
//
// The reference (train_gen_recon.py:247-261) decays its three learning rates every 1000th iteration
// (lr = max(lr * 0.99, 1e-5), Python doubles) and every 10th iteration moves the frozen target towards Q,
//   target.data.copy_(rho * param.data + (1 - rho) * target.data)
// one parameter at a time (a mul, a mul, an add and a copy per tensor), each behind a host `if (iteration + 1) % N == 0`.
// A recorded graph takes such a branch always or never.  Here the iteration count is one uint64 word in device memory;
// the EMA and the decay read it and leave their outputs untouched when they are not due, so a graph that ends with
// damc_iteration_advance runs the next iteration on its next replay.  The word is written by that call alone, in a
// launch of its own: no launch that reads it writes it.
//
// EMA: a multi-tensor pass over optim.hip's chunk tables (tensor, offset, length <= DAMC_ADAM_CHUNK; one workgroup per
// chunk), the tensors' pointers in the kernel arguments.  t = fl(fl(rho p) + fl(omr t)): two rounded products and one
// rounded add, torch's three kernels bit for bit.  12 B per element (read p, read t, write t): HBM-bound.
#include "common.h"

namespace {

struct EmaChunk {  // optim.hip's AdamChunk
  long long off;
  int tensor;
  int n;
};
static_assert(sizeof(EmaChunk) == 16, "chunk layout");

struct EmaPtrs {
  float* t[DAMC_ADAM_MAX_TENSORS];
  const float* p[DAMC_ADAM_MAX_TENSORS];
};
static_assert(sizeof(EmaPtrs) + 64 <= 4096, "kernel argument block");

constexpr int kThreads = 256;

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the gate of both kernels: uniform over the grid (every thread reads the same word)
__device__ __forceinline__ bool due(const uint64_t* iteration, uint64_t period, uint64_t phase) {
  return !iteration || (*iteration + phase) % period == 0;
}

__device__ __forceinline__ float ema_elem(float p, float t, float rho, float omr) {
#pragma clang fp contract(off)
  const float a = rho * p;
  const float b = omr * t;
  return a + b;
}

__global__ __launch_bounds__(kThreads) void ema_kernel(const EmaChunk* __restrict__ chunks, EmaPtrs a, float rho,
                                                       float omr, const uint64_t* __restrict__ iteration,
                                                       uint64_t period, uint64_t phase) {
  if (!due(iteration, period, phase)) return;
  const EmaChunk c = chunks[blockIdx.x];
  float* T = a.t[c.tensor] + c.off;
  const float* P = a.p[c.tensor] + c.off;
  int i0 = 0;
  if (al16(T) && al16(P)) {
    const int n4 = c.n >> 2;
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      const f32x4 p = reinterpret_cast<const f32x4*>(P)[i];
      f32x4 t = reinterpret_cast<const f32x4*>(T)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = ema_elem(p[e], t[e], rho, omr);
      reinterpret_cast<f32x4*>(T)[i] = t;
    }
    i0 = n4 << 2;
  }
  for (int i = i0 + threadIdx.x; i < c.n; i += kThreads) T[i] = ema_elem(P[i], T[i], rho, omr);
}

__global__ void lr_decay_kernel(double* lr64, float* lr32, int n, double factor, double floor_,
                                const uint64_t* iteration, uint64_t period, uint64_t phase) {
  if (!due(iteration, period, phase)) return;
  const int i = threadIdx.x;
  if (i >= n) return;
  const double v = fmax(lr64[i] * factor, floor_);  // Python's max(lr * factor, floor): one rounded product
  lr64[i] = v;
  lr32[i] = (float)v;
}

__global__ void iteration_advance_kernel(uint64_t* iteration, uint64_t delta) { *iteration += delta; }

}  // namespace

extern "C" {

int damc_iteration_advance(uint64_t* iteration, uint64_t delta, void* stream) {
  if (!iteration) return -DAMC_ERR_ARG;
  iteration_advance_kernel<<<1, 1, 0, as_stream(stream)>>>(iteration, delta);
  DAMC_LAUNCH_CHECK();
  return 0;
}

int damc_ema_update(const void* dev_chunks, int nchunks, float* const* target, const float* const* source,
                    int ntensors, float rho, float one_minus_rho, const uint64_t* iteration, uint64_t period,
                    uint64_t phase, void* stream) {
  if (!dev_chunks || !target || !source || nchunks < 0 || ntensors < 1 || ntensors > DAMC_ADAM_MAX_TENSORS ||
      period == 0)
    return -DAMC_ERR_ARG;
  EmaPtrs a;
  for (int i = 0; i < DAMC_ADAM_MAX_TENSORS; ++i) {
    a.t[i] = i < ntensors ? target[i] : nullptr;
    a.p[i] = i < ntensors ? source[i] : nullptr;
    if (i < ntensors && (!a.t[i] || !a.p[i])) return -DAMC_ERR_ARG;
  }
  if (nchunks == 0) return 0;
  ema_kernel<<<nchunks, kThreads, 0, as_stream(stream)>>>(static_cast<const EmaChunk*>(dev_chunks), a, rho,
                                                          one_minus_rho, iteration, period, phase);
  DAMC_LAUNCH_CHECK();
  return 0;
}

int damc_lr_decay(double* lr64, float* lr32, int n, double factor, double floor, const uint64_t* iteration,
                  uint64_t period, uint64_t phase, void* stream) {
  if (!lr64 || !lr32 || n < 1 || n > DAMC_LR_DECAY_MAX || period == 0) return -DAMC_ERR_ARG;
  lr_decay_kernel<<<1, 64, 0, as_stream(stream)>>>(lr64, lr32, n, factor, floor, iteration, period, phase);
  DAMC_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
