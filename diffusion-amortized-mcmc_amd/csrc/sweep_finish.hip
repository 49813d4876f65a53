// sweep_finish.hip — what runs after a team launch (sweep_team.hip): team_finish_kernel copies the sweep's result
// out of the z ring or, when a team member's bounded wait gave up, recomputes the whole sweep row tile by row tile
// with the team's arithmetic, bitwise, and flags the failure to the host (the health word of sweep_team.hip).
#include "sweep_impl.h"

using namespace damc;

namespace {

// acc += f(x) . W^T over one input half like ts_half, with the weight fragments read from the packed global array
// (the values and order the team's LDS copy holds): wrow = the lane's weight row at the half's first column
template <bool EMB>
__device__ __forceinline__ void rs_half(f32x4& acc, const float* wrow, int kps, int wsrc, const __amdgpu_buffer_rsrc_t& rs,
                                        long soff, int row, bool rok, const float* embs, int ld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int kq = kps >> 2, ng = kq >> 4, kbase = wave * kq;
  for (int c = 0; c < ng; ++c) {
    const int k = kbase + 16 * c + 4 * q;
    f32x4 x = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (EMB) x = *reinterpret_cast<const f32x4*>(embs + m * ld + k);
    else if (rok && k < wsrc) x = ld_sc1(rs, (soff + (long)row * wsrc + k) * 4);
    if (k < wsrc) w = *reinterpret_cast<const f32x4*>(wrow + k);
    if (!EMB) {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = x[e] > 0.f ? x[e] : 0.01f * x[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[e], w[e], acc, 0, 0, 0);
  }
}

// One workgroup (4 waves) per row tile.  err == 0: copy the sweep's result (zring[n]) to zt.  err != 0 (a team
// member's bounded wait gave up: a workgroup never became resident, e.g. another process or stream held CUs): the
// workgroup recomputes its row tile's whole sweep alone — every (step, block, column tile) with the team's
// arithmetic (same fragments and MFMA order, skip half first, the same fixed-order wave sum and epilogue), so the
// result is bitwise the team's — and marks the failure in host-visible memory (the library then runs the launch
// chain for the rest of the process).  A team failure costs time, never correctness, and never NaN.
__global__ __launch_bounds__(256) void team_finish_kernel(TsArgs a, float* zt, int* hostflag) {
  __shared__ __attribute__((aligned(16))) float red[4][TM][16];
  __shared__ __attribute__((aligned(16))) float embs[TM * (256 + 8)];  // in0 image (kpa of in0 <= 256: nz <= 128)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int er = tid >> 3, ec = tid & 7;
  const int nz = a.nz, B = a.B;
  const int r0 = blockIdx.x * TM;
  const int rows = min(TM, B - r0);
  const int err = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float* const zfin = a.zring + (long)a.n * B * nz;
  if (err) {
    if (blockIdx.x == 0 && tid == 0 && hostflag) __hip_atomic_store(hostflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const SweepCall* call = a.call;
    const int with_noise = call->with_noise;
    const float* noise = call->noise;
    float* eps_log = call->eps_log;
    const int eps_log_steps = call->eps_log_steps;
    const uint64_t seed = call->seed, chain_base = call->chain_base, step_offset = call->step_offset;
    const long ring_bytes = a.ring_step * 4;
    const int half = nz >> 1, ld0 = emb_ld(a.b[0].kpa);
    const int xrow = r0 + m;
    const bool xok = xrow < B;
    // B^T tile of in0's Fourier projection (wave w: columns 16 w .. 16 w + 15), as the team holds it
    f32x4 bv[EMB_G];
#pragma unroll
    for (int g = 0; g < EMB_G; ++g) {
      const int kk = 16 * g + 4 * q, col = wave * 16 + m;
      bv[g] = (col < half && kk < nz) ? *reinterpret_cast<const f32x4*>(a.bmat + (long)col * nz + kk)
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int k = 0; k < a.n; ++k) {
      const float* tb = a.tab + 8 * k;
      const float c0 = tb[0], c1 = tb[1], c2 = tb[2], c3 = tb[3], c4 = tb[4];
      const bool last = tb[5] != 0.f;
      const int noisy_k = (int)tb[6];
      float* const rslot = a.ring + (long)k * a.ring_step;
      const float* const zk = a.zring + (long)k * B * nz;
      float* const zk1 = a.zring + (long)(k + 1) * B * nz;
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)rslot, (short)0, (int)ring_bytes, 0x00020000);
      const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)zk, (short)0, B * nz * 4, 0x00020000);
      // in0 image: [sin 2 pi zB, cos 2 pi zB, z] of the 16 rows (the team's in0 code)
      {
        f32x4 zv4[EMB_G];
#pragma unroll
        for (int g = 0; g < EMB_G; ++g) {
          const int kk = 16 * g + 4 * q;
          zv4[g] = (xok && kk < nz) ? ld_sc1(rz, ((long)xrow * nz + kk) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (wave * 16 < half) {
          const int col = wave * 16 + m;
          const f32x4 e4 = emb_zb(zv4, bv);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rrow = 4 * q + r;
            if (col < half) {
              const float t = e4[r] - rintf(e4[r]);
              const bool ok = r0 + rrow < B;
              embs[rrow * ld0 + col] = ok ? __builtin_amdgcn_sinf(t) : 0.f;
              embs[rrow * ld0 + half + col] = ok ? __builtin_amdgcn_cosf(t) : 0.f;
            }
          }
        }
        if (wave == 0) {
#pragma unroll
          for (int g = 0; g < EMB_G; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int kk = 16 * g + 4 * q + e;
              if (kk < nz) embs[m * ld0 + 2 * half + kk] = zv4[g][e];
            }
        }
        for (int c = 2 * half + nz + tid; c < a.b[0].kpa; c += 256)
#pragma unroll
          for (int r = 0; r < TM; ++r) embs[r * ld0 + c] = 0.f;
        __syncthreads();
      }
      for (int j = 0; j < 7; ++j) {
        const TsBlock& b = a.b[j];
        const bool final_ = j == 6;
        for (int tn = 0; tn < b.ntn; ++tn) {
          const int n0 = tn * TC, erow = r0 + er, ecol = n0 + ec;
          const bool eok = tid < TM * TC && erow < B && ecol < b.dout;
          float gate = 0.f, hb = 0.f, bl = 0.f, bs = 0.f, xi = 0.f;
          if (eok) {
            const float* ghr = a.gh + ((long)k * B + erow) * a.ldgh + b.ghoff;
            gate = ghr[ecol];
            hb = ghr[b.dout + ecol];
            bl = b.bls[tn * 16 + ec];
            bs = b.bls[tn * 16 + 8 + ec];
            if (final_ && !last && with_noise) {
              if (noise) {
                xi = noise[((long)noisy_k * B + erow) * nz + ecol];
              } else {
                float n4[4];
                philox_normal4(seed, chain_base + erow, step_offset + noisy_k, (uint32_t)(ecol >> 2), DAMC_STREAM_SWEEP, n4);
                xi = pick4(n4, ecol);
              }
            }
          }
          const float* wrow = b.w + ((long)tn * 16 + m) * b.kp;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          if (j == 0) {
            rs_half<true>(acc, wrow, b.kpa, b.wa, rr, 0, xrow, xok, embs, ld0);
          } else {
            if (b.kpb > 0) rs_half<false>(acc, wrow + b.wa, b.kpb, b.wb, rr, a.b[b.srcB].ooff, xrow, xok, nullptr, 0);
            rs_half<false>(acc, wrow, b.kpa, b.wa, rr, a.b[b.srcA].ooff, xrow, xok, nullptr, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) red[wave][4 * q + r][m] = acc[r];
          __syncthreads();
          if (eok) {
            float l = 0.f, sk = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              l += red[w][er][ec];
              sk += red[w][er][8 + ec];
            }
            const float o = __builtin_fmaf(l + bl, gate, hb) + (sk + bs);  // the fma spelled out: every sweep form rounds alike
            if (!final_) {
              rslot[b.ooff + (long)erow * b.dout + ecol] = o;
            } else {
              const long zi = (long)erow * nz + ecol;
              const float zv = ld_sc1_f(zk + zi);
              const float eps = a.residual ? zv + o : o;
              if (eps_log && k < eps_log_steps) eps_log[(long)k * B * nz + zi] = eps;
              const float pred = mul_rn(c0, sub_rn(zv, mul_rn(eps, c1)));
              float zn;
              if (last) {
                zn = pred;
              } else {
                zn = add_rn(mul_rn(c2, zv), mul_rn(c3, pred));
                if (with_noise) zn = add_rn(zn, mul_rn(c4, xi));
              }
              zk1[zi] = zn;
            }
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this tile's outputs are in L2 before any wave reads them
          __syncthreads();
        }
      }
    }
  }
  // copy-out of the row tile (sc1: a rescue's own stores are read back past L1)
  for (int i = tid; i < rows * nz; i += 256) zt[(long)r0 * nz + i] = ld_sc1_f(zfin + (long)r0 * nz + i);
}

}  // namespace

namespace damc {

void launch_team_finish(const TsArgs& a, float* zt, int* hostflag, hipStream_t s) {
  hipLaunchKernelGGL(team_finish_kernel, dim3((unsigned)a.G), dim3(256), 0, s, a, zt, hostflag);
}

}  // namespace damc
