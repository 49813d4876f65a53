// smallc.h — the generator's output layer (DAMC_LAYER_SMALLC: to-RGB ConvT, tanh, residual), smallc.hip.
// Every choice among its kernels is made by one of the functions below; callers ask, none re-derives it.
#pragma once
#include "common.h"

namespace damc {

// 32-column tiles of the per-tap projection P[input pixel][tap * Cout + co] (packing, workspace, fused epilogue)
int smallc_ntile(const damc_layer_t& L);

// Forward stage 1.  The PROJ* paths leave per-tap projections in pbuf for the gather (stage 2); REG and GENERIC
// are single kernels.  have_pbuf: the workspace carries the projection buffer.  by_shape: the path with every
// switch at its default (what a fused epilogue may stand in for); else DAMC_SMALLC_PROJ16=0 / DAMC_SMALLC_PROJ_LDS=0
// (read per call) select the next fallback.
enum SmallcFwd { SMALLC_FWD_PROJ16, SMALLC_FWD_PROJ_LDS, SMALLC_FWD_PROJ, SMALLC_FWD_REG, SMALLC_FWD_GENERIC };
SmallcFwd smallc_fwd_path(const damc_layer_t& L, bool have_pbuf, bool by_shape = false);

// Forward stage 2 of the PROJ* paths (DAMC_SMALLC_GATHER_LDS=0, read per call: always DIRECT)
enum SmallcGather { SMALLC_GATHER_K3_LDS, SMALLC_GATHER_S2_LDS, SMALLC_GATHER_DIRECT };
SmallcGather smallc_gather_path(const damc_layer_t& L, int B);

// Input gradient.  By shape alone: its LReLU' mask can come from the producer's sign bits (the workspace then
// carries them, and a limb-engine producer writes them) ...
bool smallc_dgrad_reads_bits(const damc_layer_t& L);
// ... the form the gradient leaves in -- fp32 in place of the activation, x3 limbs only, or fp32 for a limb-engine
// dgrad that gathers fp32 (gemm_x3.hip X3_F32A).  bits: sign bits carry the mask; limbs: the dgrad below reads through
// the limb engine; f32a: that dgrad gathers fp32
enum SmallcGrad { SMALLC_GRAD_F32, SMALLC_GRAD_LIMBS, SMALLC_GRAD_F32A };
SmallcGrad smallc_grad_form(const damc_layer_t& L, bool bits, bool limbs, bool f32a);
// ... and the kernel that runs
enum SmallcDgrad { SMALLC_DGRAD_MFMA, SMALLC_DGRAD_K3, SMALLC_DGRAD_REG, SMALLC_DGRAD_GENERIC };
SmallcDgrad smallc_dgrad_kernel_of(const damc_layer_t& L, bool bits, SmallcGrad form);

// x_hat = tanh(ConvT(h) + bias) (NCHW, optional), delta = (x_hat - x) inv_s2 (1 - x_hat^2) (NHWC, optional) and
// |x_hat - x|^2 inv_s2 / 2 added to *sqerr (optional).  p_ready: pbuf already holds the projections (the layer
// before ran them in its epilogue, GemmArgs::proj_out; only where smallc_fwd_path by shape is PROJ16)
int smallc_fwd(const damc_layer_t& L, const float* h, int B, const float* x, float inv_s2, float* delta, float* xhat,
               float* sqerr, float* pbuf, hipStream_t s, bool p_ready = false);
// dh = act'(h) . ConvT^T(delta) in the form asked for (smallc_grad_form): over h, or as limbs into h3 (h stays);
// hbits: h's sign bits as the mask (smallc_dgrad_reads_bits, LReLU) or nullptr (the fp32 h itself)
int smallc_dgrad(const damc_layer_t& L, float* h, int B, const float* delta, int mask_act, float mask_slope,
                 unsigned short* h3, const unsigned char* hbits, SmallcGrad form, hipStream_t s);

}  // namespace damc
