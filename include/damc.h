/*
 * damc.h — C ABI of libdamc.so, the MI355X (gfx950) diffusion-amortized Langevin inner loop.
 *
 * The reference (yuPeiyu98/Diffusion-Amortized-MCMC) has no native/FFI layer: its hot path is
 * the Python call surface of workspace/src/MCMC.py and workspace/src/diffusion_net.py.  Each
 * entry point below replaces the device work behind one of those Python functions; the
 * Python mirror (diffusion-amortized-mcmc_amd/damc, bound with ctypes)
 * keeps the reference's names and signatures.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer to caller-owned fp32 memory unless noted;
 *   - images are NCHW exactly as the caller holds them; latents z are (B, nz) row-major;
 *   - weights are passed once per call to damc_pack_* in PyTorch layouts and re-laid out
 *     into caller-allocated packed buffers (no allocation inside the library);
 *   - `stream` is a hipStream_t passed as void*; no host synchronisation happens inside
 *     any call (everything is stream-ordered and graph-capturable);
 *   - return 0 on success, otherwise a hipError_t value or one of DAMC_ERR_* (the Python
 *     side raises RuntimeError with damc_error_string()).
 *   - step sizes / sigma are the reference's Python floats (double): the updates use float32(0.5 step^2) and
 *     float32(step) (and float32(1 / sigma^2)), the values PyTorch's fp32 scalar ops round them to;
 *   - noise: with_noise != 0 and noise == NULL draws xi ~ N(0,1) in-kernel from
 *     Philox4x32-10 keyed by (seed) with counter (dim/4, step + step_offset,
 *     chain_base + chain, stream_id): a chain's noise depends on its GLOBAL index only, so
 *     results are identical for any sharding of the batch over GPUs.  noise != NULL
 *     injects (n_steps, B, nz) values instead (parity tests).  Stream ids: 0x51 posterior chains, 0x52 prior
 *     chains, 0x53 the reverse sweep, 0x54 the guided sweep's prior-embedding noise, and for the seeded Q update
 *     (step = the update's draw_index) 0x55 DAMC_STREAM_QU the schedule's u, 0x56 DAMC_STREAM_QEPS the forward
 *     diffusion's eps, 0x57 DAMC_STREAM_QPE the prior-embedding noise of Q.calculate_loss.
 */
#ifndef DAMC_H
#define DAMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAMC_ABI_VERSION 3
#define DAMC_MAX_LAYERS 10

enum {
  DAMC_OK = 0,
  DAMC_ERR_ARG = 1001,       /* invalid shape / argument */
  DAMC_ERR_WORKSPACE = 1002, /* workspace too small */
  DAMC_ERR_UNSUPPORTED = 1003
};

/* Generator layer kinds (workspace/src/diffusion_net.py:20-203, toy_example.py:22-47) */
enum {
  DAMC_LAYER_PROJ = 1,   /* ConvTranspose2d on a 1x1 input (first layer): a GEMM z·W        */
  DAMC_LAYER_UP2 = 2,    /* ConvTranspose2d k4 s2 p1 with Cout >= 8: phase-split implicit GEMM */
  DAMC_LAYER_SMALLC = 3, /* last ConvTranspose2d with Cout <= 4 (to RGB / gray)             */
  DAMC_LAYER_LINEAR = 4  /* nn.Linear (toy MLP generator)                                  */
};
enum { DAMC_ACT_NONE = 0, DAMC_ACT_LRELU = 1, DAMC_ACT_TANH = 2, DAMC_ACT_SILU = 3, DAMC_ACT_RELU = 4 /* damc_mlp_forward */ };
/* Convolution engine of a generator layer (every layer of one generator must name the same one):
 *   DAMC_ENGINE_LIMB: layers whose gathered channel count is a multiple of 32 run on the limb engine —
 *     fp32 operands split into 3 bf16 limbs, 6 limb products per fp32 product on bf16 MFMA, fp32
 *     accumulation (error vs fp64 equal to fp32 MFMA's); the other layers on the fp32 MFMA engine;
 *   DAMC_ENGINE_FP32: every convolution on the fp32 MFMA engine (v_mfma_f32_32x32x2_f32).
 * Packed weights and workspaces are sized for either engine. */
enum { DAMC_ENGINE_LIMB = 0, DAMC_ENGINE_FP32 = 1 };

typedef struct {
  int kind;
  int cin, cout, k, stride, pad;
  int hin, win, hout, wout;  /* spatial sizes (1 for PROJ input / LINEAR)                 */
  int act;                   /* activation after this layer                               */
  float slope;               /* LeakyReLU slope (ReLU = 0)                                */
  const float* w_fwd;        /* packed forward weights  (damc_pack_generator_layer)       */
  const float* w_bwd;        /* packed dgrad weights                                      */
  const float* bias;         /* (cout) or NULL                                            */
  int engine;                /* DAMC_ENGINE_* (0 = limb engine, the default)              */
} damc_layer_t;

typedef struct {
  int n_layers;
  int nz;                     /* latent size                                               */
  int nc, h, w;               /* image shape (for LINEAR generators: nc = out features, h = w = 1) */
  damc_layer_t layers[DAMC_MAX_LAYERS];
} damc_generator_t;

/* Latent EBM _netE: Linear(nz,nh) LReLU Linear(nh,nh) LReLU Linear(nh,1) (diffusion_net.py:207-223) */
typedef struct {
  int nz, nh;
  float slope;
  const float *w1, *b1, *w2, *b2, *w3, *b3;  /* PyTorch layouts: w1 (nh,nz), w2 (nh,nh), w3 (1,nh) */
  const float *w1t, *w2t;                     /* packed transposes (damc_pack_ebm)                  */
} damc_ebm_t;

/* Draw state: a Philox key in DEVICE memory (16 bytes, 8-B aligned), for callers that capture the seeded entry points
 * in a HIP graph.  A host seed and offset are kernel arguments, fixed at capture, so a replay would draw the same
 * noise again; the drawn variants (suffix _ds) below take `const damc_draw_state_t* state` where the entry point of
 * the same name takes `seed`, and their kernels read the two words from device memory at run time:
 *   result == the seeded entry point called with seed = state->seed and
 *             step_offset (step_index, draw_index; 0 for the sweep) = the host value + state->counter, bit for bit.
 * They launch the kernels the seeded entry points launch (which pass a null state) and nothing else: no extra launch,
 * no host read, no synchronisation; the state is read once per launch or workgroup (team sweep and launch chain: by
 * the setup kernel that writes the sweep's device-resident call record).  A drawn variant never advances the state:
 * the caller enqueues damc_draw_state_advance after the calls that share a counter value.  state == NULL returns
 * DAMC_ERR_ARG before any launch.  The guided sweep has no drawn variant. */
typedef struct {
  uint64_t seed;
  uint64_t counter;
} damc_draw_state_t;
/* counter += delta, by a one-thread kernel on `stream` (stream-ordered and capturable like every other call) */
int damc_draw_state_advance(damc_draw_state_t* state, uint64_t delta, void* stream);

/* ---------------------------------------------------------------- library / packing */
int damc_abi_version(void);
const char* damc_error_string(int code);

/* floats needed by the packed forward / dgrad buffers of one generator layer */
int damc_generator_layer_packed_sizes(const damc_layer_t* layer, size_t* fwd_floats, size_t* bwd_floats);
/* re-lay PyTorch weight (ConvT: (Cin,Cout,k,k); Linear: (out,in)) into layer->w_fwd / w_bwd */
int damc_pack_generator_layer(const damc_layer_t* layer, const float* w_torch, float* w_fwd, float* w_bwd,
                              void* stream);
/* w1t (nz,nh) and w2t (nh,nh) from the PyTorch w1/w2 */
int damc_pack_ebm(const damc_ebm_t* ebm, float* w1t, float* w2t, void* stream);

/* ------------------------------------------------------------- posterior Langevin (a1) */
/* workspace bytes for damc_posterior_langevin / damc_likelihood_grad / damc_generator_forward */
size_t damc_posterior_workspace_bytes(const damc_generator_t* g, int batch);

/* sample_langevin_post_z_with_prior (workspace/src/MCMC.py:48-74):
 *   for i < n_steps:  z <- z - 0.5*step^2 * grad U(z) (+ step*xi),
 *   U = |G(z)-x|^2/(2 sigma^2) + sum E(z) + |z|^2/2     (E omitted when ebm == NULL)
 * z (B,nz) updated in place; x (B,nc,h,w) NCHW; diag (optional, n_steps*4 floats, zeroed by
 * the call): per step {sum E, |G(z)-x|^2/(2sigma^2), |z|^2/2, mean(grad)} before the update. */
int damc_posterior_langevin(const damc_generator_t* g, const damc_ebm_t* ebm, float* z, const float* x,
                            int batch, int n_steps, double sigma, double step, int with_noise,
                            const float* noise, uint64_t seed, uint64_t step_offset, uint64_t chain_base,
                            float* diag, void* workspace, size_t workspace_bytes, void* stream);

/* the drawn variant (damc_draw_state_t above): step i draws at step_offset + state->counter + i */
int damc_posterior_langevin_ds(const damc_generator_t* g, const damc_ebm_t* ebm, float* z, const float* x, int batch,
                               int n_steps, double sigma, double step, int with_noise, const float* noise,
                               const damc_draw_state_t* state, uint64_t step_offset, uint64_t chain_base, float* diag,
                               void* workspace, size_t workspace_bytes, void* stream);

/* per-op hooks (parity tests): grad_z |G(z)-x|^2/(2 sigma^2) -> grad (B,nz) */
int damc_likelihood_grad(const damc_generator_t* g, const float* z, const float* x, int batch, double sigma,
                         float* grad, void* workspace, size_t workspace_bytes, void* stream);
/* x_hat = G(z) (B,nc,h,w) NCHW — gen_samples / gen_samples_with_diffusion_prior (MCMC.py:119-150) */
int damc_generator_forward(const damc_generator_t* g, const float* z, int batch, float* x_hat,
                           void* workspace, size_t workspace_bytes, void* stream);

/* per-op hooks for ONE k4 s2 p1 ConvTranspose2d (DAMC_LAYER_UP2) layer of a generator, NHWC
 * activations, the same kernels and engine choice as inside damc_posterior_langevin:
 *   damc_convT_fwd:   out (B, hout, wout, cout) = act(conv_transpose2d(in (B, hin, win, cin), W) + bias)
 *   damc_convT_dgrad: gin (B, hin, win, cin) = conv_transpose2d^T(gout (B, hout, wout, cout), W), multiplied by
 *                     act'(mask_pre) when mask_pre != NULL (the previous layer's activated output, act = mask_act)
 * layer: packed by damc_pack_generator_layer; workspace: damc_convT_workspace_bytes (limb copy of the input). */
size_t damc_convT_workspace_bytes(const damc_layer_t* layer, int batch);
int damc_convT_fwd(const damc_layer_t* layer, const float* in, int batch, float* out, void* workspace,
                   size_t workspace_bytes, void* stream);
int damc_convT_dgrad(const damc_layer_t* layer, const float* gout, int batch, const float* mask_pre, int mask_act,
                     float mask_slope, float* gin, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------- generator training step */
/* The G update of a training iteration (workspace/train_gen_recon.py:222-231):
 *   x_hat = G(z); g_loss = sum((x_hat - x)^2, [1,2,3]).mean(); g_loss.backward()
 * damc_generator_train_forward computes x_hat (NCHW) and keeps in the workspace what the backward reads;
 * damc_generator_train_backward then maps grad_xhat = dL/dx_hat (NCHW, from the caller's autograd) to the
 * weight and bias gradients of every layer (PyTorch layouts: ConvTranspose2d (Cin, Cout, k, k), Linear
 * (out, in); WRITTEN, not accumulated; NULL entries are skipped) and, if grad_z != NULL, dL/dz (B, nz).
 * The two calls must use the same descriptor, batch and workspace, with no other call on that workspace in
 * between: train_forward records (workspace, batch, engine) and train_backward returns DAMC_ERR_ARG for a
 * descriptor or batch that disagrees.  ConvT weight gradients run on the limb engine (fp32-accurate bf16
 * MFMA) whatever the layers' engine; layer inputs and gradients with a batch that is not a multiple of 32
 * are zero-padded to one.
 * Generators the backward cannot run are refused on the host, before any launch: a k4 s2 p1 layer whose Cout, or a
 * first layer whose Cout * k * k, is not a multiple of 8 (e.g. the celeba64 topology at ngf = 4: a last hidden layer
 * of 4 channels), operands of a weight-gradient GEMM beyond 2^31 bytes, an output layer with k other than 3 or 4.
 * damc_generator_train_workspace_bytes then returns 0 and both calls return DAMC_ERR_UNSUPPORTED; the plain forward
 * (damc_generator_forward) and the Langevin entry points stay available for such a generator. */
typedef struct {
  float* w[DAMC_MAX_LAYERS];
  float* b[DAMC_MAX_LAYERS];
} damc_generator_grads_t;
size_t damc_generator_train_workspace_bytes(const damc_generator_t* g, int batch);
int damc_generator_train_forward(const damc_generator_t* g, const float* z, int batch, float* x_hat, void* workspace,
                                 size_t workspace_bytes, void* stream);
int damc_generator_train_backward(const damc_generator_t* g, const float* z, const float* x_hat,
                                  const float* grad_xhat, int batch, const damc_generator_grads_t* grads,
                                  float* grad_z, void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------- prior Langevin (a2) */
/* sample_langevin_prior_z (MCMC.py:27-46): all n_steps in ONE persistent launch.
 * diag (optional, n_steps*2 floats): {sum E, |z|^2/2} per step before the update. */
int damc_prior_langevin(const damc_ebm_t* ebm, float* z, int batch, int n_steps, double step, int with_noise,
                        const float* noise, uint64_t seed, uint64_t step_offset, uint64_t chain_base,
                        float* diag, void* stream);
/* the same with the engine chosen per call: 0 = by batch size (the default above: the 16-chain MFMA tile kernel
 * from DAMC_EBM_MFMA_MIN_B = 2048 chains up, where the FC layers are real GEMMs), 1 = register-resident VALU
 * (one chain per workgroup), 2 = MFMA (nz % 16 == 0, nh % 4 == 0, nz and nh <= 256, else DAMC_ERR_UNSUPPORTED: the
 * tile reads its weight rows as float4 runs along nh, and a run that starts inside a row must end inside it; engine 0
 * takes the VALU kernels for such a shape at any batch).
 * Engine 0 is keyed on THIS call's batch.  The two engines sum in different orders, so a sharded caller that needs
 * its shards' union bitwise equal to the unsharded block resolves the engine itself from the global chain count
 * (>= damc_ebm_mfma_min_chains() -> 2, else 1) and passes 1 or 2, as damc.langevin does. */
/* the threshold engine 0 uses: DAMC_EBM_MFMA_MIN_B, read once per process (default 2048) */
int damc_ebm_mfma_min_chains(void);
int damc_prior_langevin_engine(const damc_ebm_t* ebm, float* z, int batch, int n_steps, double step, int with_noise,
                               const float* noise, uint64_t seed, uint64_t step_offset, uint64_t chain_base,
                               float* diag, int engine, void* stream);
/* the drawn variant of damc_prior_langevin_engine (damc_draw_state_t above) */
int damc_prior_langevin_ds(const damc_ebm_t* ebm, float* z, int batch, int n_steps, double step, int with_noise,
                           const float* noise, const damc_draw_state_t* state, uint64_t step_offset,
                           uint64_t chain_base, float* diag, int engine, void* stream);
/* per-op hook: energy (B) and grad_z sum E (B,nz) */
int damc_ebm_energy_grad(const damc_ebm_t* ebm, const float* z, int batch, float* energy, float* grad,
                         void* stream);
/* the same under SURVEY.md §8b's name */
int damc_ebm_grad(const damc_ebm_t* ebm, const float* z, int batch, float* energy, float* grad, void* stream);
/* per-op hook: z <- z - 0.5 step^2 (g + z) (+ step xi) ; g (B,nz) */
int damc_z_update(float* z, const float* g, int batch, int nz, double step, int with_noise, const float* noise,
                  uint64_t seed, uint64_t step_index, uint64_t chain_base, void* stream);
int damc_z_update_ds(float* z, const float* g, int batch, int nz, double step, int with_noise, const float* noise,
                     const damc_draw_state_t* state, uint64_t step_index, uint64_t chain_base, void* stream);
/* Which kernel of csrc/ebm.hip a call runs, by shape, engine and batch alone (host only, no launch):
 *   1 = register-resident VALU (nz <= 128 and nh <= 208), 2 = MFMA tile, 3 = streaming (every other shape whose
 *   rows fit 64 KB of LDS), 0 = none: the call returns DAMC_ERR_UNSUPPORTED.
 * engine 0 / 1 / 2: a prior chain of damc_prior_langevin_engine with that engine and batch.  engine -1: the choice of
 * damc_ebm_energy_grad and of the posterior update (1, 3 or 0; batch is not read; nh = 0 asks for the update without
 * an EBM).  The entry points dispatch through this function. */
int damc_ebm_kernel(int nz, int nh, int engine, int batch);
/* per-op hook: the update kernel of one posterior Langevin step, exactly what damc_posterior_langevin launches after
 * the likelihood gradient and nothing else:
 *   g = sum_k glik_slabs[k * slab_stride + i] (+ grad_z E(z) when ebm != NULL) + z ; z <- z - 0.5 step^2 g (+ step xi)
 * z (batch, nz) in place; glik_slabs: nslab >= 1 slabs of (batch, nz), slab k at glik_slabs + k * slab_stride
 * (slab_stride >= batch * nz when nslab > 1).  The register-resident kernel adds the slabs in 16 groups of every 16th
 * slab and then the groups in order, the streaming kernel in slab order.  xi: noise (batch, nz) when given, else the
 * Philox draw of (seed, chain_base + row, step_index) on the posterior stream.  diag (optional, 4 floats, zeroed by
 * the call): {sum E, untouched (0), |z|^2/2, mean(g)} before the update.  z_limbs (optional, batch * nz * 3 bf16): the
 * new z as x3 limbs [batch][nz / 8][3][8]; *limbs_written (required) is 1 when the kernel wrote them (the
 * register-resident kernel at nz % 8 == 0), else 0 and z_limbs is untouched.  NULL z, glik_slabs or limbs_written,
 * batch, nz or nslab < 1, an ebm whose nz differs, that lacks a pointer, or a slab_stride below batch * nz with
 * nslab > 1 return DAMC_ERR_ARG before any launch; a shape with damc_ebm_kernel(nz, nh, -1, 0) == 0 returns
 * DAMC_ERR_UNSUPPORTED. */
int damc_posterior_update(const damc_ebm_t* ebm, float* z, const float* glik_slabs, int nslab, long slab_stride,
                          int batch, int nz, double step, int with_noise, const float* noise, uint64_t seed,
                          uint64_t step_index, uint64_t chain_base, float* diag, unsigned short* z_limbs,
                          int* limbs_written, void* stream);
/* Philox N(0,1) draw used by every Langevin kernel (statistical tests) -> out (n_steps,B,nz) */
int damc_philox_normal(float* out, int n_steps, int batch, int nz, uint64_t seed, uint64_t step_offset,
                       uint64_t chain_base, uint32_t stream_id, void* stream);
/* One U[0, 1) value per (step, row) -> out (n_steps, B): word 0 of the Philox block damc_philox_normal draws for
 * (seed, chain_base + row, step_offset + step, quad 0, stream_id), as (float)(word >> 8) * 2^-24 -- torch.rand's
 * half-open interval on the 2^-24 grid (the normals keep their (0, 1] uniforms). */
int damc_philox_uniform(float* out, int n_steps, int batch, uint64_t seed, uint64_t step_offset, uint64_t chain_base,
                        uint32_t stream_id, void* stream);
/* the drawn variants of the two (damc_draw_state_t above) */
int damc_philox_normal_ds(float* out, int n_steps, int batch, int nz, const damc_draw_state_t* state,
                          uint64_t step_offset, uint64_t chain_base, uint32_t stream_id, void* stream);
int damc_philox_uniform_ds(float* out, int n_steps, int batch, const damc_draw_state_t* state, uint64_t step_offset,
                           uint64_t chain_base, uint32_t stream_id, void* stream);

/* ------------------------------------------------- per-sample posterior energy (anomaly score) */
/* The anomaly drivers' score (workspace/eval_anomaly_det.py:114-117, train_anomaly_det.py:223-226) per sample, with
 * a fixed summation order and no atomics: a row's result depends on that row's data and on the row length only --
 * not on the batch size, the row's index or the other rows -- so shards of a batch reproduce the whole batch bit
 * for bit.  Each row is cut into chunks of a fixed 16384 elements, one workgroup per (row, chunk); the chunk sums
 * are added in chunk order.  A NULL or inconsistent argument and a workspace shorter than the query's answer both
 * return DAMC_ERR_ARG on the host, before any launch. */
/* per-op hook: out[b] = sum_j (xhat[b,j]-x[b,j])^2, fixed summation order, independent of batch composition */
size_t damc_recon_rows_workspace_bytes(int batch, long row_elems);
int damc_recon_rows(const float* xhat, const float* x, int batch, long row_elems, float* out, void* workspace,
                    size_t workspace_bytes, void* stream);
/* per-sample terms of U at a fixed z (z and x are read, never written):
 *   terms (batch,3) = {|G(z)-x|^2, sum E(z) (0 if ebm == NULL), |z|^2/2};
 *   score (batch) optional = recon_weight*terms[0] + terms[1] + terms[2], each operation rounded on its own;
 *   xhat optional (G(z), forward layout).
 * Runs damc_generator_forward's kernels (x_hat into the workspace when xhat == NULL), damc_ebm_energy_grad's
 * per-chain energy, and the two kernels above. */
size_t damc_posterior_energy_workspace_bytes(const damc_generator_t* g, int batch);
int damc_posterior_energy(const damc_generator_t* g, const damc_ebm_t* ebm, const float* z, const float* x, int batch,
                          float recon_weight, float* terms, float* score, float* xhat, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- Q amortizer (a8-a11) */
/* generic fp32 MFMA implicit-GEMM conv (NHWC) + bias: encoder building block.  workspace (floats, may be
 * NULL / 0): split-K slabs for convolutions whose output tiles would not fill the chip, sized by
 * damc_conv2d_workspace_floats (0 = no split for that shape) */
size_t damc_conv2d_workspace_floats(int batch, int hin, int win, int cin, int cout, int k, int stride, int pad);
int damc_conv2d_nhwc(const float* x, int batch, int hin, int win, int cin, const float* w_packed, const float* bias,
                     int cout, int k, int stride, int pad, float* y, float* workspace, size_t workspace_floats,
                     void* stream);
/* pack Conv2d weight (Cout,Cin,k,k) into the engine's layout (same element count; opaque to callers):
 * (Cout, k,k,Cin) for the K-major engine when Cin % 32 == 0, else (k,k,Cin,Cout) */
int damc_pack_conv2d(const float* w_torch, int cout, int cin, int k, float* w_packed, void* stream);
/* InstanceNorm2d(affine, eps) + LeakyReLU(slope), in place on NHWC (Welford partials merged with
 * Chan's formula, taken relative to each (sample, channel)'s first pixel so that a large common offset costs no
 * accuracy; each element as ((y - mean) * rstd) * gamma + beta, the bits of the training call's h);
 * workspace: damc_instnorm_workspace_floats() floats (the partials and one pivot per (sample, channel)) */
size_t damc_instnorm_workspace_floats(int batch, int hw, int c);
int damc_instnorm_lrelu_nhwc(float* y, int batch, int hw, int c, const float* gamma, const float* beta, float eps,
                             float slope, float* workspace, void* stream);
/* Encoder training (the Q update's encoder backward; Encoder_* diffusion_net.py:227-413):
 * InstanceNorm2d(affine) + LeakyReLU keeping the conv output y: h = lrelu(IN(y)) into its own buffer and
 * stats (B, c, 2) = {mean, rstd}; workspace as damc_instnorm_workspace_floats */
int damc_instnorm_lrelu_train_nhwc(const float* y, int batch, int hw, int c, const float* gamma, const float* beta,
                                   float eps, float slope, float* h, float* stats, float* workspace, void* stream);
size_t damc_instnorm_bwd_workspace_floats(int batch, int hw, int c);
/* dh (grad of h) -> dy (grad of the conv output y), dgamma, dbeta (c) (either may be NULL) */
int damc_instnorm_lrelu_backward_nhwc(const float* y, const float* stats, const float* dh, int batch, int hw, int c,
                                      const float* gamma, const float* beta, float slope, float* dy, float* dgamma,
                                      float* dbeta, float* workspace, void* stream);
/* Conv2d backward on NHWC activations, weight in PyTorch (Cout, Cin, k, k): dx (NHWC, may be NULL), dw, db (may
 * be NULL).  Supported: k4 s2 p1 with H = 2 Ho (limb engine), the first k3 s1 p1 conv with Cin <= 4 (no dx), and
 * a last conv covering its whole input (p0, 1x1 output).  workspace bytes: 0 = shape not supported. */
size_t damc_conv2d_backward_workspace_bytes(int batch, int hin, int win, int cin, int cout, int k, int stride,
                                            int pad);
int damc_conv2d_backward_nhwc(const float* x, const float* dy, const float* w, int batch, int hin, int win, int cin,
                              int cout, int k, int stride, int pad, float* dx, float* dw, float* db, void* workspace,
                              size_t workspace_bytes, void* stream);

/* NCHW -> NHWC transpose (encoder input) */
int damc_nchw_to_nhwc(const float* x, int batch, int c, int hw, float* y, void* stream);

/* The whole Encoder_* forward of _netQ_U (SURVEY.md §8b damc_q_encoder_fwd; diffusion_net.py:227-372, a10):
 * [Conv2d -> InstanceNorm2d(affine) -> LeakyReLU]* -> Conv2d on the kernels above, x (B, nc, h, w) NCHW ->
 * xemb (B, nemb) with nemb = cout * ho * wo of the last conv (1 x 1 in every Encoder_*, where the NHWC and
 * the reference's NCHW flattening agree; other output sizes return DAMC_ERR_UNSUPPORTED).
 * engine DAMC_ENGINE_LIMB: the convolutions whose input channel count is a multiple of 32 (every one but the
 * first 3x3 at the reference's nif) run on the limb engine (fp32-accurate, bf16 MFMA; see DAMC_ENGINE_*), the
 * input activation split into limbs per call; w_x3 = damc_pack_conv2d_x3 of the layer's weight (then w_packed
 * may be NULL for that layer), or w_src = the weight itself (packed by the library per call, see below), or neither
 * (the library splits w_packed into the workspace per call). */
#define DAMC_MAX_ENC_LAYERS 8
typedef struct {
  int cin, cout, k, stride, pad;
  const float* w_packed;          /* damc_pack_conv2d layout (NULL allowed for a limb layer with w_x3) */
  const float* bias;              /* (cout) or NULL                                                   */
  const float *in_gamma, *in_beta; /* InstanceNorm2d affine (cout); NULL: no norm / activation after it */
  float in_eps, slope;
  const void* w_x3;               /* the limb B operand (damc_pack_conv2d_x3) or NULL                 */
  const float* w_src;             /* or the PyTorch Conv2d weight (cout, cin, k, k) of a limb layer, 16-B aligned:
                                     the library packs every such layer into the workspace per call, as extra
                                     workgroups of the first layer's launch (w_x3 and w_packed then unused)   */
} damc_enc_layer_t;
typedef struct {
  int n_layers, nc, h, w;
  damc_enc_layer_t layers[DAMC_MAX_ENC_LAYERS];
  int engine; /* DAMC_ENGINE_* */
} damc_encoder_t;
/* bytes of the limb copy of a packed conv weight (0: the layer does not run on the limb engine) */
size_t damc_conv2d_x3_bytes(int cout, int cin, int k);
/* k per sign block of the limb engine's weight operands (odd blocks stored negated; = its MFMA accumulation block
 * and its split-K granule) for the encoder's convs (damc_pack_conv2d_x3): the build's DAMC_X3_NEGK, 512 by default */
int damc_x3_sign_block(void);
/* 1 when a k x k Conv2d on cin channels has its limb weight operand (damc_pack_conv2d_x3) and its encoder GEMMs in the
 * 4 x 4 conv walk (k = 4, cin % 32 == 0: K index = (ci / 32) 512 + p 32 + ci % 32 with p the parity-grouped position of
 * tap (ky, kx): ((ky % 2) 2 + kx % 2) 4 + (ky / 2) 2 + kx / 2; sign blocks counted in that order), 0 when tap-major
 * [(ky, kx, ci)]; opt-in: DAMC_ENC_WALK=1 (read per call) selects the walk, tap-major otherwise */
int damc_x3_conv_walk(int k, int cin);
/* the sign block of a generator UP2 layer's limb weights (damc_pack_generator_layer), forward (input_grad = 0,
 * K = 4 Cin) or input gradient (1, K = 16 Cout): 512 or 1024 by the layer's shape alone (gemm.h x3_conv_negk);
 * 0 for a layer without limb weights */
int damc_x3_layer_sign_block(const damc_layer_t* L, int input_grad);
/* the K order of those limb weights and of every limb-engine launch that reads them, by the layer's shape alone: 1 =
 * channel-slice-major (K tile kt of 32 k = channels 32 (kt / 4) .. of the phase's tap kt % 4 in the forward; channels
 * 32 (kt / 16) .. of the 4 x 4 tap at parity-grouped position kt % 16 in the input gradient), 0 = tap-major or no
 * limb weights.  The fp32 packings keep their tap-major layout */
int damc_x3_layer_walk(const damc_layer_t* L, int input_grad);
/* K tile kt of that walk -> its first channel and its tap (forward: ty * 2 + tx of the phase's 2 x 2 conv; input
 * gradient: ky * 4 + kx).  Groups of four consecutive K tiles share a channel slice and, in the input gradient, the
 * taps' (ky, kx) parity */
int damc_x3_walk_ktile(int input_grad, int kt, int* channel0, int* tap);
/* 1 when the layer's fp32-gathering limb GEMMs (forward / input gradient) stage one input image per group of four K
 * tiles (gemm.hip X3_TAPSHARE: the layer walks slice-major and its hin x win grid tiles the 256-row block: hin * win
 * divides 256); 0: one image per tap, the same bits.  DAMC_X3_TAPSHARE=0 (read per call) forces per-tap staging */
int damc_x3_layer_tapshare(const damc_layer_t* L, int input_grad);
/* launches that ran with the shared staging since the library was loaded */
unsigned long long damc_x3_tapshare_launches(void);
/* diagnostics: while buf (n_slots * 4 uint64, device memory) is set, every k4 s2 ConvT forward on the limb engine
 * stores, per workgroup w at buf[4 (w % n_slots)], {s_memtime, s_memrealtime} before and after its K loop: the
 * clock the chip holds in that loop is d(memtime) / d(realtime) x 100 MHz.  buf = NULL switches it off.  Not
 * thread-safe; keep it off in timed work (bench.py runs it on one extra block). */
int damc_clock_probe(unsigned long long* buf, int n_slots);
/* a Conv2d weight in its PyTorch layout (cout, cin, k, k), cin % 32 == 0 -> the limb engine's B operand of the
 * conv (damc_conv2d_x3_bytes bytes), in one pass */
int damc_pack_conv2d_x3(const float* w, int cout, int cin, int k, void* w_x3, void* stream);
/* one Conv2d (+ bias) on the limb engine, NHWC fp32 in and out (the Q update's encoder forward, which keeps every conv
 * output for its backward): w_x3 = damc_pack_conv2d_x3 of the weight; k4 s2 p1 convs stage x as fp32, other shapes
 * split it into limbs in the workspace (damc_conv2d_x3_workspace_bytes; 0 = the shape has no limb-engine form) */
size_t damc_conv2d_x3_workspace_bytes(int batch, int hin, int win, int cin, int cout, int k, int stride, int pad);
int damc_conv2d_x3_nhwc(const float* x, int batch, int hin, int win, int cin, const void* w_x3, const float* bias,
                        int cout, int k, int stride, int pad, float* y, void* workspace, size_t workspace_bytes,
                        void* stream);
size_t damc_q_encoder_workspace_bytes(const damc_encoder_t* enc, int batch);
int damc_q_encoder_fwd(const damc_encoder_t* enc, const float* x, int batch, float* xemb, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The encoder of the Q update in two calls (round 5; Encoder_* forward and backward inside Q.calculate_loss,
 * diffusion_net.py:624-645, train_gen_recon.py:211-220): every layer's w_src = its PyTorch Conv2d weight, bias set,
 * in_gamma / in_beta on every layer but the last, whose output is 1 x 1 (xemb (B, cout)); engine as for
 * damc_q_encoder_fwd.  The forward keeps in `saved` (damc_encoder_train_saved_floats floats) the NHWC input, every
 * conv output, InstanceNorm statistics and activation; the backward maps grad_xemb (B, nemb) to the gradients
 * (written, not accumulated; NULL entries skipped).  One workspace size serves both calls; 0 = not supported. */
typedef struct {
  float *w[DAMC_MAX_ENC_LAYERS], *b[DAMC_MAX_ENC_LAYERS], *gamma[DAMC_MAX_ENC_LAYERS], *beta[DAMC_MAX_ENC_LAYERS];
} damc_encoder_grads_t;
size_t damc_encoder_train_saved_floats(const damc_encoder_t* enc, int batch);
size_t damc_encoder_train_workspace_bytes(const damc_encoder_t* enc, int batch);
int damc_encoder_train_forward(const damc_encoder_t* enc, const float* x, int batch, float* saved, float* xemb,
                               void* workspace, size_t workspace_bytes, void* stream);
int damc_encoder_train_backward(const damc_encoder_t* enc, const float* saved, const float* grad_xemb, int batch,
                                const damc_encoder_grads_t* grads, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Dense fp32 MFMA GEMM: C(M,N) = act(A(M,K) · B(K,N) + bias) with B row-major (K,N); bias (N) or NULL; act any
 * DAMC_ACT_* (slope: DAMC_ACT_LRELU's), any other value DAMC_ERR_ARG, as lda < k, ldb < n or ldc < n.  Any m, n, k >= 1
 * and any 4-B aligned operands: K % 4, lda % 4 or a 16-B misaligned A (N % 4, ldb % 4 or B likewise) take scalar loads.
 * Only C[i * ldc + j], i < m, j < n is written. */
int damc_gemm(const float* a, int lda, const float* b, int ldb, const float* bias, float* c, int ldc, int m,
              int n, int k, int act, float slope, void* stream);

/* A small MLP of nn.Linear layers in ONE launch: the toy amortizer's encoder (workspace/toy_example/src/
 * diffusion_net.py:166-174, Linear(2,128)-ReLU x3 then Linear(128, nxemb), used at :193 and :245) and its prior_emb
 * (:180-184, used at :196, :215, :248, :251) at nz = 2.  Weights are the caller's live PyTorch tensors ((out, in),
 * k contiguous; bias (out) or NULL), read in place: no packing, no workspace.  Each layer applies act in
 * {DAMC_ACT_NONE, DAMC_ACT_RELU, DAMC_ACT_LRELU(slope)}; layers chain (din of layer i = dout of layer i - 1); every
 * width is at most DAMC_MLP_MAX_WIDTH.  16 rows per workgroup, activations in LDS; a layer with K % 16 == 0 runs on
 * the fp32 MFMA, any other K (K = 2) as plain FMAs.  x (batch, layers[0].din), out (batch, last dout). */
#define DAMC_MLP_MAX_LAYERS 8
#define DAMC_MLP_MAX_WIDTH 256
typedef struct {
  int din, dout, act;
  float slope;
  const float *w, *bias;
} damc_mlp_layer_t;
typedef struct {
  int n_layers;
  damc_mlp_layer_t layers[DAMC_MLP_MAX_LAYERS];
} damc_mlp_t;
int damc_mlp_forward(const damc_mlp_t* mlp, const float* x, int batch, float* out, void* stream);

/* The same MLP under training: the toy amortizer's encoder and prior_emb inside calculate_loss (workspace/toy_example/
 * src/diffusion_net.py:166-184 as used at :241-263, six times per iteration by toy_example.py:209-219).  The training
 * calls take what damc_mlp_forward takes with two more conditions: the last layer has DAMC_ACT_NONE, and an LRELU slope
 * is >= 0 (the backward reads act' from the sign of the saved post-activation).
 * damc_mlp_train_saved_floats / _workspace_bytes: sizes of `saved` (floats) and of the backward's workspace (bytes) at
 * this batch; 0 for a descriptor or batch the library does not take. */
typedef struct {
  float* w[DAMC_MLP_MAX_LAYERS]; /* dL/dW (out, in) per layer, written (not accumulated); NULL: skipped */
  float* b[DAMC_MLP_MAX_LAYERS]; /* dL/db (out) per layer; NULL: skipped                                */
} damc_mlp_grads_t;
size_t damc_mlp_train_saved_floats(const damc_mlp_t* mlp, int batch);
size_t damc_mlp_train_workspace_bytes(const damc_mlp_t* mlp, int batch);
/* Forward of diffusion_net.py:166-184 keeping activations: damc_mlp_forward's kernel (out is bitwise its out), which
 * also stores every hidden layer's post-activation rows in saved: layer l's (batch, dout_l) block at float offset
 * batch * (dout_0 + ... + dout_{l-1}), l < n_layers - 1.  One launch. */
int damc_mlp_train_forward(const damc_mlp_t* mlp, const float* x, int batch, float* saved, float* out, void* stream);
/* Backward of the same (the encoder's and prior_emb's share of diffusion_net.py:241-263's loss.backward(),
 * toy_example.py:213): grad_out (batch, last dout) -> every non-NULL grads->w[l], grads->b[l].  No input gradient (x is
 * data or a fresh draw).  Two launches: a 16-rows-per-workgroup dgrad chain through LDS, and one launch for every
 * layer's dW and db with the batch walked in a fixed order (no atomics: bitwise reproducible).  Any batch >= 1;
 * allocates and synchronises nothing. */
int damc_mlp_train_backward(const damc_mlp_t* mlp, const float* x, const float* saved, const float* grad_out,
                            int batch, const damc_mlp_grads_t* grads, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Denoiser Diffusion_UnetA (diffusion_net.py:417-533) and its reverse sweep (diffusion_net.py:595-622).
 * Seven ConcatSquashLinearSkipCtx blocks (in0 in1 in2 mid0 out0 out1 out2).  Every weight is the caller's
 * PyTorch tensor in its own layout (nn.Linear (out, in)); the library re-lays them out into its workspace per
 * call (the nets train between calls), so the caller does no per-call packing. */
typedef struct {
  int din, dout;
  /* PyTorch nn.Linear layout (out, in), k contiguous */
  const float *wl, *bl; /* _layer.0     (dout, din), (dout)  */
  const float *ws, *bs; /* _skip        (dout, din), (dout)  */
  const float *wg, *bg; /* _hyper_gate  (dout, dout), (dout) */
  const float* wb;      /* _hyper_bias  (dout, dout), no bias */
} damc_csq_block_t;

typedef struct {
  int nz, ntemb, nxemb, residual;
  const float* bmat;                  /* p.B (nz, nz/2)                                  */
  const float *tw1, *tb1, *tw2, *tb2; /* time_mlp[1], time_mlp[3]: (out, in), (out)      */
  damc_csq_block_t blocks[7];         /* in0 in1 in2 mid0 out0 out1 out2                 */
  const float* wctx[7];               /* _layer_ctx[1].weight (dout, ntemb + nxemb)       */
  const float* bctx[7];               /* _layer_ctx[1].bias (dout)                       */
} damc_denoiser_t;

/* workspace bytes for damc_reverse_sweep */
size_t damc_sweep_workspace_bytes(const damc_denoiser_t* d, int batch, int n_steps);
/* The reverse sweep (n_steps = n_interval denoiser evaluations, i = n_steps-1 .. 0, k = n_steps-1-i).
 * Per call the library packs the weights, then evaluates everything that does not depend on zt for all
 * steps at once: the time MLP (batch-invariant), the ctx Linear's xemb part (step-invariant), and for every
 * (step, row) a block's ctx c = SiLU(Lc(SiLU(cat(temb, xemb)))), its gate sigmoid(c Wg^T + bg) and hyper
 * bias c Wb^T (limb-product MFMA GEMMs over n*B rows).  The dependent chain — per step the 7 blocks'
 * x Wl^T / x Ws^T products plus the reverse-step update — then runs as ONE team launch (weights LDS-resident,
 * data-driven hand-offs between the workgroups of a team; at the reference's widths, nf = 4 with nz 128 or 100, a
 * kernel with those shapes compiled in, DAMC_SWEEP_FAST=0 the generic one, bitwise the same); DAMC_SWEEP_TEAM=0
 * runs it as 7 launches per step replayed from a HIP graph cached per (workspace, shapes, schedule).  The launch chain
 * is also what a sweep takes by itself when a team's share of the weights does not fit a workgroup's LDS (in0's dout
 * of 160 and more on a 256-CU device), when the device's CUs do not split into 8 groups, and after a rescue (below);
 * damc_sweep_form tells which.  Accepted shapes: nz even, 4 <= nz <= 128 for these forms; in0's dout w % 4 == 0 with
 * the block widths (din 2nz w 2w 2w 4w 4w 2w, dout w 2w 2w 2w 2w w nz); any ntemb, nxemb >= 1.  The per-call stages
 * run on the skinny GEMM only when ntemb % 16 == 0, nxemb % 4 == 0 and every dout, nz included, is a multiple of 16
 * (nz = 100 is not), and the hyper GEMMs on the limb product only when every dout, nz included, is a multiple of 32
 * and at most 512 (damc_sweep_stages); otherwise on the fp32 GEMM.
 * A denoiser whose nz is no multiple of 4 (the toy's _netQ_U_toy, workspace/toy_example/src/diffusion_net.py:141-239,
 * nz = 2; any even nz <= 128) runs the chain in its row-resident form instead: one workgroup per 16 rows runs all
 * steps and blocks for them with the activations in LDS and nothing handed between workgroups (denoiser_rows.hip);
 * DAMC_SWEEP_ROWS=1 (read per call) takes that form for every shape whose 16-row LDS image fits (16 x (kpad(2 nz) +
 * 8 w + max(w + pad64(w), pad64(2 w)) + 4) floats within 156 KB; otherwise DAMC_ERR_UNSUPPORTED and a workspace size
 * of 0 while the switch is set).  A denoiser with nz % 4 != 0 needs ntemb % 16 == 0, nxemb % 4 == 0, a width (in0's
 * dout) that is a multiple of 16 and an image that fits: w <= 224 at nz = 10 (DAMC_ERR_UNSUPPORTED otherwise).
 *   eps = p(zt, l_t, xemb); pred = c0 * (zt - eps * c1); zt <- last ? pred : c2*zt + c3*pred (+ c4*xi)
 * temb_in (n_steps, ntemb): SinusoidalPosEmb of the step's logsnr input (host, fp32, as the reference);
 * coef (n_steps, 6), a HOST pointer: {sqrt(1+e^-lt), rsqrt(1+e^lt), r*alpha_st, (1-r)*alpha_s, std,
 * is_last} (diffusion_helper_func.py:36-70, evaluated on the host in fp32 like the reference; the
 * scalars travel by value in each step's kernel arguments);
 * noise (n_steps-1, B, nz) injected or NULL for Philox; eps_log (optional) receives eps of the
 * first eps_log_steps steps. zt (B, nz) is updated in place; xemb (B, nxemb). */
int damc_reverse_sweep(const damc_denoiser_t* d, const float* xemb, float* zt, int batch, int n_steps,
                       const float* temb_in, const float* coef, int with_noise, const float* noise, uint64_t seed,
                       uint64_t chain_base, float* eps_log, int eps_log_steps, void* workspace,
                       size_t workspace_bytes, void* stream);
/* the drawn variant (damc_draw_state_t above): noisy step k draws at state->counter + k, in every form of the sweep
 * (team launch, launch chain, row-resident) */
int damc_reverse_sweep_ds(const damc_denoiser_t* d, const float* xemb, float* zt, int batch, int n_steps,
                          const float* temb_in, const float* coef, int with_noise, const float* noise,
                          const damc_draw_state_t* state, uint64_t chain_base, float* eps_log, int eps_log_steps,
                          void* workspace, size_t workspace_bytes, void* stream);
/* the same under SURVEY.md §8b's name */
int damc_q_reverse_sweep(const damc_denoiser_t* d, const float* xemb, float* zt, int batch, int n_steps,
                         const float* temb_in, const float* coef, int with_noise, const float* noise, uint64_t seed,
                         uint64_t chain_base, float* eps_log, int eps_log_steps, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The team reverse sweep (default) needs all its workgroups resident at once.  If a member never starts (another
 * process or stream holding CUs), its bounded waits give up and the library recomputes the affected sweep on the
 * device (bitwise the team's arithmetic; never NaN), flags the device, and runs later sweeps on the launch chain.
 * damc_sweep_team_failures: how many such rescued launches this process has seen on a device (a rescue still in
 * flight is counted once it completes). */
long damc_sweep_team_failures(int device);
/* Two host queries of the sweep's dispatch, computed by the predicates the sweep itself branches on; neither launches
 * anything.
 * damc_sweep_stages: what the per-call stages run on, by shape alone (pointers taken as 16-byte aligned, no environment
 * switch read).  A refused denoiser gives minus its error code (-DAMC_ERR_ARG, -DAMC_ERR_UNSUPPORTED); otherwise a mask:
 *   bit 0      the time MLP and ctx Linears run on the skinny GEMM (ntemb % 16 == 0, nxemb % 4 == 0 and every block's
 *              dout % 16 == 0, out2 aside when nz % 4 != 0); clear: on the fp32 GEMM over transposed copies
 *   bit 1      nz % 4 != 0: out2's columns of the stages come from the narrow kernels, the chain is row-resident
 *   bit 2      the row-resident form's LDS image of 16 rows fits (DAMC_SWEEP_ROWS=1 is available)
 *   bits 8-14  block j's gate / hyper-bias GEMM runs on the limb product.  The blocks go in one grouped launch, so
 *              these are all set (bits 8-13 when bit 1 is set) or none: every block needs dout % 32 == 0 and
 *              dout <= 512, or the whole stage runs on the fp32 engine.
 * damc_sweep_form: the form damc_reverse_sweep would take now for (batch, n_steps), on the current device, outside a
 * stream capture, with DAMC_SWEEP_ROWS / _TEAM / _FAST read as the sweep reads them: 0 none (the sweep refuses),
 * 1 row-resident, 2 team launch on the generic kernel, 3 team launch on the shape-specialised kernel, 4 launch chain
 * (the team disabled, this device flagged after a rescue, or the weights too wide for a team's LDS). */
int damc_sweep_stages(const damc_denoiser_t* d);
int damc_sweep_form(const damc_denoiser_t* d, int batch, int n_steps);
/* per-op hook (SURVEY.md §8b damc_denoise_step): ONE reverse step = damc_reverse_sweep with n_steps = 1 on the
 * step's temb_row (ntemb) and coef_row (6, HOST); noise (B, nz) injected or NULL for Philox at step index
 * noise_step (the k-th noisy step of a sweep uses k); eps (B, nz) receives the denoiser output or NULL.
 * workspace: damc_sweep_workspace_bytes(d, batch, 1). */
int damc_denoise_step(const damc_denoiser_t* d, const float* xemb, float* zt, int batch, const float* temb_row,
                      const float* coef_row, int with_noise, const float* noise, uint64_t seed, uint64_t noise_step,
                      uint64_t chain_base, float* eps, void* workspace, size_t workspace_bytes, void* stream);
/* The guided reverse sweep: classifier-free guidance, Q(x, cond_w = w > 0) (workspace/src/diffusion_net.py:595-620), as
 * ONE stream-ordered call.  Per step the reference evaluates the denoiser on the encoder's xemb and on a fresh
 * prior_emb(randn) and steps on eps = (1 + w) eps_c - w eps_u (each op rounded to fp32).  xemb (B, nxemb) is the
 * conditional embedding; xemb_unc (n_steps, B, nxemb) the unconditional one of every step, step-major in sweep order
 * (k = n_steps-1-i), made by the caller.  A seeded caller draws its noise from damc_philox_normal with stream_id
 * 0x54 (DAMC_STREAM_GUIDE; keyed seed, chain_base + row, step k) and passes it through prior_emb as n_steps * B rows;
 * the library draws only the step noise, from the sweep's own stream (0x53), keyed by the latent row as
 * damc_reverse_sweep keys it, so shards by chain_base reproduce their rows bit for bit.
 * The per-call stages are the reverse sweep's, run for both branches by the same kernels (the unconditional planes per
 * (step, row)); the chain runs row-resident with each latent row held twice: a workgroup owns 8 latent rows, its MFMA
 * rows 0-7 their conditional and 8-15 their unconditional evaluation, every weight fragment serving both, and the two
 * eps meet by one cross-lane move in the last block's epilogue (denoiser_rows.hip).  No allocation, no
 * synchronisation; zt (B, nz) is updated in place; coef is a HOST pointer; temb_in, coef, with_noise, noise
 * (n_steps-1, B, nz), seed, chain_base, eps_log (the guided eps of the first eps_log_steps steps) as
 * damc_reverse_sweep's.
 * workspace: damc_guided_sweep_workspace_bytes, the reverse sweep's plus 4 S floats per (step, row) for the
 * unconditional planes (S = the blocks' summed widths: ~0.3 GB more at B = 128, 100 steps, the CIFAR widths).  It is 0
 * where the 16-row LDS image does not fit the CU or nz % 4 != 0; the sweep then returns DAMC_ERR_UNSUPPORTED.
 * DAMC_ERR_ARG: a null xemb, xemb_unc, zt, temb_in or coef, a non-positive size, cond_w <= 0. */
size_t damc_guided_sweep_workspace_bytes(const damc_denoiser_t* d, int batch, int n_steps);
int damc_guided_sweep(const damc_denoiser_t* d, const float* xemb, const float* xemb_unc, float cond_w, float* zt,
                      int batch, int n_steps, const float* temb_in, const float* coef, int with_noise,
                      const float* noise, uint64_t seed, uint64_t chain_base, float* eps_log, int eps_log_steps,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------- Q training: denoiser loss step */
/* The denoiser of Q.calculate_loss (workspace/src/diffusion_net.py:624-645, Diffusion_UnetA :463-533) as
 * trained by the Q update of every iteration (workspace/train_gen_recon.py:211-220): eps_pred =
 * p(zt, logsnr, xemb) with every intermediate kept, then the backward from dL/deps_pred to every parameter
 * of p, to zt and to xemb (which the caller's autograd carries into the encoder / prior_emb).  All weights
 * in PyTorch layouts (the damc_denoiser_t of the sweep).  temb_in (B, ntemb) is SinusoidalPosEmb of the
 * per-sample logsnr input, evaluated by the caller with the reference's op sequence (diffusion_net.py:447-461,
 * 490-491).  nz is even.  A multiple of 4 runs every Linear on the fp32 GEMM engine; any other even nz (the toy
 * amortizer's Diffusion_Unet at nz = 2, workspace/toy_example/src/diffusion_net.py:63-139 as trained by :241-263 and
 * toy_example.py:209-219) lays out2 out padded to the next multiple of 4 inside the workspace, with zero weights and
 * biases there, and runs the K = nz products around the Fourier embedding as small kernels of their own.
 * Alignment: the workspace is 16-B aligned (DAMC_ERR_UNSUPPORTED otherwise, on the host before any launch); nothing
 * else is required.  zt, temb_in, xemb, grad_eps, eps_pred, grad_zt, grad_xemb, every weight of d and every entry of
 * grads are plain float pointers (4-B aligned): the kernels read and write them one float at a time, but for zt, the A
 * operand of the z B product, which leaves the grouped float4 kernel for the engine's scalar gather when zt is not 16-B
 * aligned (as the backward's K = nz / 2 product does when nz / 2 is no multiple of 4).  Any batch >= 1; a batch that is
 * no multiple of 4 runs every weight and bias gradient (K = batch) on the tiled engine's scalar gather, split over K from
 * 97 rows on.
 * Returns, all on the host before any launch: DAMC_ERR_ARG for a descriptor damc_denoiser_train_workspace_bytes gives
 * 0 for (odd nz or ntemb, a NULL weight, widths that are not Diffusion_UnetA's wiring), batch <= 0 or a NULL zt,
 * temb_in, xemb, eps_pred, grad_eps or grads; DAMC_ERR_WORKSPACE for a NULL or short workspace. */
typedef damc_denoiser_t damc_denoiser_train_t;
typedef struct { /* gradients, same layouts (written, not accumulated; NULL entries are skipped) */
  float* bmat;
  float *tw1, *tb1, *tw2, *tb2;
  float *wl[7], *bl[7], *ws[7], *bs[7], *wg[7], *bg[7], *wb[7], *wctx[7], *bctx[7];
} damc_denoiser_grads_t;
size_t damc_denoiser_train_workspace_bytes(const damc_denoiser_train_t* d, int batch);
int damc_denoiser_train_forward(const damc_denoiser_train_t* d, const float* zt, const float* temb_in,
                                const float* xemb, int batch, float* eps_pred, void* workspace, size_t workspace_bytes,
                                void* stream);
/* after damc_denoiser_train_forward on the same workspace: grad_eps (B, nz) -> grads, grad_zt (B, nz) and
 * grad_xemb (B, nxemb) (either may be NULL) */
int damc_denoiser_train_backward(const damc_denoiser_train_t* d, const float* grad_eps, int batch,
                                 const damc_denoiser_grads_t* grads, float* grad_zt, float* grad_xemb,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The rest of Q.calculate_loss around the denoiser (round 5; workspace/src/diffusion_net.py:633-642, no gradient
 * flows through any of it): from u (B) ~ U[0,1) (the caller's torch.rand, :633) and eps (B, nz) (torch.randn_like,
 * :636), logsnr (B) = logsnr_schedule_fn(u) (diffusion_helper_func.py:41-50; may be NULL), zt (B, nz) = the
 * diffusion_forward mean + std * eps (:72-78), temb_in (B, ntemb) = SinusoidalPosEmb of Diffusion_UnetA's logsnr input
 * (diffusion_net.py:447-461, 490-491) with freqs (ntemb / 2) the host's fp32 frequency table; one launch for what the
 * reference issues as ~25 elementwise ops, each op rounded as PyTorch's ROCm kernels round it. */
int damc_q_noise_glue(const float* u, const float* z, const float* eps, int batch, int nz, float logsnr_min,
                      float logsnr_max, const float* freqs, int ntemb, float* logsnr, float* zt, float* temb_in,
                      void* stream);
/* damc_q_noise_glue with its draws made in the same launch (the data-parallel Q update): u (B) from stream 0x55 as
 * damc_philox_uniform gives it, eps (B, nz) from stream 0x56 as damc_philox_normal gives it, both keyed (seed,
 * chain_base + row, step draw_index), so a row's noise depends on its GLOBAL index and the update's index only.  eps is
 * written (the loss reads it); u and logsnr are written when non-NULL.  zt, temb_in and logsnr are bitwise what
 * damc_q_noise_glue gives when fed the u and eps this call returns.  Any nz damc_q_noise_glue takes; bad arguments
 * return DAMC_ERR_ARG. */
int damc_q_noise_glue_seeded(const float* z, int batch, int nz, float logsnr_min, float logsnr_max, const float* freqs,
                             int ntemb, uint64_t seed, uint64_t draw_index, uint64_t chain_base, float* u, float* eps,
                             float* logsnr, float* zt, float* temb_in, void* stream);
/* the drawn variant (damc_draw_state_t above): the update's index is draw_index + state->counter */
int damc_q_noise_glue_seeded_ds(const float* z, int batch, int nz, float logsnr_min, float logsnr_max,
                                const float* freqs, int ntemb, const damc_draw_state_t* state, uint64_t draw_index,
                                uint64_t chain_base, float* u, float* eps, float* logsnr, float* zt, float* temb_in,
                                void* stream);
/* loss (B) = 0.5 * sum_j (eps - eps_pred)^2 (diffusion_net.py:642), and grad_eps_pred (B, nz) from grad_loss (B, element
 * stride grad_stride: 0 for the broadcast gradient of a .mean()) */
int damc_q_loss_forward(const float* eps, const float* eps_pred, int batch, int nz, float* loss, void* stream);
int damc_q_loss_backward(const float* eps, const float* eps_pred, const float* grad_loss, long grad_stride, int batch,
                         int nz, float* grad_eps_pred, void* stream);

/* ------------------------------------------------------- E update (round 5; SURVEY §8f, train_gen_recon.py:233-241)
 * E(z) of _netE (diffusion_net.py:207-223, e's PyTorch-layout w1..b3; w1t / w2t unused) keeping the hidden activations
 * h1, h2 (B, nh) for the backward; energy (B).  Batch and the layer widths multiples of 4, a LeakyReLU slope >= 0 (the
 * backward takes LReLU' from the sign of the saved activation), w1, w2, w3 16-B aligned; the forward's z, h1, h2 and the
 * backward's workspace 16-B aligned too (the float4 rows of the products).  DAMC_ERR_UNSUPPORTED otherwise (the caller
 * keeps PyTorch), returned on the host before the first launch: nothing has been written.  A descriptor that is refused
 * has a workspace size of 0.  Biases, grad_energy, the entries of grads and grad_z need no more than a float's 4 B. */
typedef struct { /* gradients, PyTorch layouts (written, not accumulated; NULL entries are skipped) */
  float *w1, *b1, *w2, *b2, *w3, *b3;
} damc_ebm_grads_t;
size_t damc_ebm_train_workspace_bytes(const damc_ebm_t* e, int batch);
int damc_ebm_train_forward(const damc_ebm_t* e, const float* z, int batch, float* h1, float* h2, float* energy,
                           void* stream);
/* grad_energy (B, element stride grad_stride: 0 for a .mean()'s broadcast) -> grads and grad_z (B, nz) or NULL */
int damc_ebm_train_backward(const damc_ebm_t* e, const float* z, const float* h1, const float* h2,
                            const float* grad_energy, long grad_stride, int batch, const damc_ebm_grads_t* grads,
                            float* grad_z, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------- Q update: prior embedding (round 6; SURVEY §8f, diffusion_net.py:624-641)
 * Q.prior_emb = Linear(nz, nh) -> LeakyReLU(slope >= 0) -> Linear(nh, nout) (diffusion_net.py:577-581), PyTorch-layout
 * weights; the forward keeps the hidden activation h (B, nh) for the backward.  Replaces the stock modules inside
 * Q.calculate_loss (the mask's prior rows / x None).  Batch and widths multiples of 4, slope >= 0, w1 and w2 16-B
 * aligned; the forward's noise and h, the backward's grad_out and workspace 16-B aligned too (the float4 rows of the
 * products).  DAMC_ERR_UNSUPPORTED otherwise (the caller keeps PyTorch), returned on the host before the first launch:
 * nothing has been written.  A descriptor that is refused has a workspace size of 0.  Biases, out and the entries of
 * grads need no more than a float's 4 B. */
typedef struct {
  int nz, nh, nout;
  float slope;
  const float *w1, *b1, *w2, *b2;
} damc_prior_emb_t;
typedef struct { /* gradients, PyTorch layouts (written, not accumulated; NULL entries are skipped) */
  float *w1, *b1, *w2, *b2;
} damc_prior_emb_grads_t;
size_t damc_prior_emb_train_workspace_bytes(const damc_prior_emb_t* e, int batch);
int damc_prior_emb_train_forward(const damc_prior_emb_t* e, const float* noise, int batch, float* h, float* out,
                                 void* stream);
/* grad_out (B, nout) contiguous -> the four parameter gradients (the input is a fresh draw: no input gradient) */
int damc_prior_emb_train_backward(const damc_prior_emb_t* e, const float* noise, const float* h, const float* grad_out,
                                  int batch, const damc_prior_emb_grads_t* grads, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ------------------------------------------ spectral norm of a net's layers (G and E updates with use_spc_norm / e_sn)
 * One forward of torch.nn.utils.spectral_norm's SpectralNorm.compute_weight (torch/nn/utils/spectral_norm.py; the
 * reference's sn, diffusion_net.py:8-16) and its gradient, for up to DAMC_SPECNORM_MAX_LAYERS layers in grouped
 * launches (one grid covers every layer).  w_orig is read in place in its PyTorch layout as a 3-d view [a][r][k] whose
 * matrix row is the middle index and whose column is a_i * k + k_i: Linear(out, in) is [1][out][in] (the hook's
 * dim = 0), ConvTranspose2d(cin, cout, kh, kw) is [cin][cout][kh * kw] (dim = 1); no permuted copy is made.
 * Forward, per power iteration: v <- W^T u / max(|W^T u|, eps), u <- W v / max(|W v|, eps), written in place into
 * the module's own u (r) and v (a * k) buffers; then sigma = u^T (W v) and w_hat = w_orig / sigma (an IEEE divide) in
 * w_orig's layout, plus sigma (1) and the copies u_used (r), v_used (a * k) the backward reads.  Backward: g[i] holds
 * dL/dw_hat in that layout and is overwritten with dL/dw_orig = (g - <g, w_hat> u_used v_used^T) / sigma (u, v are
 * constants of the graph, as in the hook); it reads w_hat, sigma, u_used, v_used only, and a NULL g[i] skips layer i.
 * Every reduction is a fixed-order two-stage sum through the workspace (no atomics; scalars finish in fp64): results
 * are bitwise repeatable.  16-byte accesses when k % 4 == 0 and the layer's pointers are 16-B aligned, scalar ones
 * otherwise.  workspace_bytes: 0 when the table is not taken (n < 1, n > 8, a NULL layer pointer, an extent < 1). */
#define DAMC_SPECNORM_MAX_LAYERS 8
typedef struct {
  const float* w_orig;
  float *u, *v;                           /* the module's buffers, updated in place */
  float *w_hat, *sigma, *u_used, *v_used; /* per-forward outputs, the backward's inputs */
  int a, r, k;
  float eps;
} damc_specnorm_layer_t;
size_t damc_specnorm_workspace_bytes(const damc_specnorm_layer_t* layers, int n);
int damc_specnorm_forward(const damc_specnorm_layer_t* layers, int n, int power_iterations, void* workspace,
                          size_t workspace_bytes, void* stream);
int damc_specnorm_backward(const damc_specnorm_layer_t* layers, int n, float* const* g, void* workspace,
                           size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------- optimiser steps
 * Replaces the G/E/Q updates' torch.nn.utils.clip_grad_norm_ + optim.Adam / optim.AdamW.step()
 * (train_gen_recon.py:155-157, 219-231, 240-241) by multi-tensor kernels.  A launch covers up to
 * DAMC_ADAM_MAX_TENSORS fp32 tensors whose device pointers travel in the kernel arguments (host arrays
 * here), so nothing is rebuilt when autograd hands out new gradient buffers.  The chunk table depends
 * only on the tensor sizes: entry = (tensor index, element offset, length <= DAMC_ADAM_CHUNK), built on
 * the host by damc_adam_build_chunks and copied to device memory by the caller (plain bytes). */
#define DAMC_ADAM_CHUNK 8192
#define DAMC_ADAM_MAX_TENSORS 96
typedef struct { /* per-step scalars, computed by the caller exactly as torch's _multi_tensor_adam does */
  float neg_step_size;   /* -(lr / (1 - beta1^t))                                           */
  float one_minus_beta1; /* lerp weight 1 - beta1                                            */
  float beta2, one_minus_beta2;
  float bc2_sqrt;        /* (1 - beta2^t) ** 0.5                                             */
  float eps;
  float weight_decay;    /* Adam (L2 into the gradient) when decoupled == 0                  */
  float decay_mul;       /* AdamW: 1 - lr * weight_decay                                     */
  int decoupled;
} damc_adam_hparams_t;
size_t damc_adam_chunk_bytes(void);
/* host only: number of chunks for tensors of these sizes */
int damc_adam_chunk_count(const long long* numel, int ntensors);
/* host only: writes the chunk table into host_chunks (max_chunks entries); returns the count or < 0 */
int damc_adam_build_chunks(const long long* numel, int ntensors, void* host_chunks, int max_chunks);
/* clip_grad_norm_(max_norm, norm_type=2), first half: out[0] = total norm, out[1] = min(max_norm /
 * (norm + 1e-6), 1).  grads: host array of ntensors (<= DAMC_ADAM_MAX_TENSORS) device pointers.
 * workspace: nchunks floats.  Gradients are not scaled here (damc_grad_scale, or damc_adam_step's clip). */
int damc_grad_norm(const void* dev_chunks, int nchunks, float* const* grads, int ntensors, float max_norm,
                   float* workspace, float* out, void* stream);
/* the two halves of damc_grad_norm, for gradient sets of more than DAMC_ADAM_MAX_TENSORS tensors: per-chunk
 * sums of squares into partial[0, nchunks) (call once per <= 96-tensor slice, each into its own range),
 * then the fixed-order total over all n partials */
int damc_grad_sumsq(const void* dev_chunks, int nchunks, float* const* grads, int ntensors, float* partial,
                    void* stream);
int damc_grad_norm_finish(const float* partial, int n, float max_norm, float* out, void* stream);
/* grads *= clip[1] (the second half of clip_grad_norm_) */
int damc_grad_scale(const void* dev_chunks, int nchunks, float* const* grads, int ntensors, const float* clip,
                    void* stream);
/* gradient bucket of a data-parallel update: bucket[bucket_off[t] + i] = grads[t][i] * scale over the chunk table of
 * the tensors' sizes (one fp32 multiply, rounded on its own); grads[t] == NULL writes zeros.  grads and bucket_off
 * (element offsets, >= 0) are host arrays of ntensors (<= DAMC_ADAM_MAX_TENSORS) entries that travel in the kernel
 * arguments.  16-byte accesses where the source and the destination slice are both 16-byte aligned, scalar ones
 * otherwise (the same values).  Elements between the slices are not written.  The other calls of this section take
 * arbitrary pointers, so after the reduce they run on the bucket's slices: there is no unpack. */
int damc_grad_pack(const void* dev_chunks, int nchunks, const float* const* grads, const long long* bucket_off,
                   int ntensors, float scale, float* bucket, void* stream);
/* one Adam/AdamW step over every chunk (params, grads, exp_avgs, exp_avg_sqs: host arrays of device
 * pointers); clip (device, from damc_grad_norm) or NULL: when given, the gradient is scaled by clip[1]
 * first and written back, as clip_grad_norm_ would have left it */
int damc_adam_step(const void* dev_chunks, int nchunks, float* const* params, float* const* grads,
                   float* const* exp_avgs, float* const* exp_avg_sqs, int ntensors, const damc_adam_hparams_t* hp,
                   const float* clip, void* stream);

/* The same step for a caller that captures it in a HIP graph (torch.optim's capturable=True): the step count is a
 * DEVICE fp32 scalar, so nothing the host computes from it is baked into the launch.  advance != 0 first adds 1 to
 * *step (a one-thread kernel on the stream; pass 0 for the second and later <= 96-tensor slices of one step); the
 * step kernel then reads *step and evaluates 1 - beta1^t, sqrt(1 - beta2^t), lr / (1 - beta1^t) and 1 - lr wd in
 * double, rounds each to fp32 once -- what the caller of damc_adam_step does on the host -- and runs
 * damc_adam_step's element arithmetic.  lr: a device fp32 scalar read by the kernel, or NULL for hp->lr (then fixed
 * at capture).  Against damc_adam_step the results agree to the last place of the device's and the host's pow. */
typedef struct {
  double lr, beta1, beta2, eps, weight_decay;
  int decoupled; /* AdamW */
} damc_adam_capturable_t;
int damc_adam_step_capturable(const void* dev_chunks, int nchunks, float* const* params, float* const* grads,
                              float* const* exp_avgs, float* const* exp_avg_sqs, int ntensors,
                              const damc_adam_capturable_t* hp, float* step, int advance, const float* lr,
                              const float* clip, void* stream);

/* --------------------------------------------------- iteration glue: counter, EMA target, lr decay (schedule.hip)
 * What the reference driver runs on the host between its updates (train_gen_recon.py:247-261), as launches gated by an
 * iteration count in DEVICE memory, so a HIP graph of a whole iteration takes the "every Nth iteration" branches on
 * the replays that are due.  `iteration` is one uint64 word; a gated call applies when
 *   (*iteration + phase) % period == 0          (the reference's `(iteration + 1) % 10 == 0`: period 10, phase 1)
 * and otherwise writes NOTHING (a uniform early exit of the grid); iteration == NULL applies always.  The word is
 * written by damc_iteration_advance alone, in a launch of its own.  All three are stream-ordered and capturable, do not
 * allocate and do not synchronise.  They return -DAMC_ERR_ARG on the host, before any launch, for a NULL iteration
 * (advance), NULL tables or pointer arrays or entries, ntensors outside 1..DAMC_ADAM_MAX_TENSORS, n outside
 * 1..DAMC_LR_DECAY_MAX, period == 0; otherwise 0 or a hipError_t. */
#define DAMC_LR_DECAY_MAX 8
/* *iteration += delta (a one-thread kernel) */
int damc_iteration_advance(uint64_t* iteration, uint64_t delta, void* stream);
/* target[t][i] = fl(fl(rho * source[t][i]) + fl(one_minus_rho * target[t][i])) over the chunk table of the tensors'
 * sizes (damc_adam_build_chunks): two rounded products and one rounded add, bitwise torch's
 * `rho * p + (1 - rho) * t` in fp32.  target / source: host arrays of ntensors device pointers that travel in the
 * kernel arguments.  16-byte accesses where a chunk's target and source are both 16-byte aligned, scalar ones
 * otherwise and for the tail (the same values).  source is only read.  12 B per element. */
int damc_ema_update(const void* dev_chunks, int nchunks, float* const* target, const float* const* source,
                    int ntensors, float rho, float one_minus_rho, const uint64_t* iteration, uint64_t period,
                    uint64_t phase, void* stream);
/* lr64[i] = fmax(lr64[i] * factor, floor) in IEEE double (Python's max(lr * factor, floor)), then
 * lr32[i] = (float)lr64[i], for i < n: lr32[i] is the device scalar damc_adam_step_capturable reads as `lr`. */
int damc_lr_decay(double* lr64, float* lr32, int n, double factor, double floor, const uint64_t* iteration,
                  uint64_t period, uint64_t phase, void* stream);

/* ------------------------------------------------------------ FID statistics */
/* calculate_fid* (workspace/src/MCMC.py:130-176) reduce Inception pool features to (mu, sigma) before the
 * Frechet distance (pytorch-fid's calculate_frechet_distance, via pfw.fid).  Here the statistics accumulate on
 * the device in fp64: s1 (d) += sum over the n rows of feats (n, d) fp32, s2 (d, d) += feats^T feats; across
 * GPUs the caller all-reduces (s1, s2, n) once (damc.fid over RCCL).  Deterministic (fixed summation order). */
int damc_fid_accumulate(const float* feats, int n, int d, double* s1, double* s2, void* stream);
/* mu = s1 / n, sigma = (s2 - n mu mu^T) / (n - 1) (np.cov's unbiased estimate); n > 1 */
int damc_fid_mean_cov(const double* s1, const double* s2, double n, int d, double* mu, double* sigma, void* stream);

/* --------------------------------------------------------------------------- profiling */
/* optional per-kernel HIP-event timing (bench.py roofline): records events around each
 * launch of the named kernel class on the launch stream; read back after a sync. */
int damc_prof_enable(int on);
/* record only the comma-separated kernel classes in `classes` (NULL: every class) */
int damc_prof_select(const char* classes);
int damc_prof_reset(void);
/* total ms and launch count for kernel class `name` ("upconv_fwd", "upconv_dgrad", ...) */
int damc_prof_query(const char* name, double* total_ms, long* launches, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* DAMC_H */
