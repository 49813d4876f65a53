"""Shared by tests/test_ebm_ops_cases_cpu.py and tests/test_gpu_ebm_ops.py: the case tables of the Langevin-side EBM
calls of include/damc.h (damc_ebm_energy_grad, damc_prior_langevin_engine, damc_posterior_update), the kernel of
csrc/ebm.hip each case has to reach, and their fp32 / fp64 PyTorch-CPU references.

Cases are (nz, nh, B).  csrc/ebm.hip picks a kernel by shape, engine and batch alone (damc_ebm_kernel):
  1  ebm_reg_kernel            nz <= 128 and nh <= 208: wave w owns rows 13 w .. 13 w + 12, lane l columns l + 64 i
  2  prior_chain_mfma_kernel   engine 2: nz % 16 == 0, nh % 4 == 0, nz and nh <= 256; 16-chain tiles, 16-column N tiles
  3  the streaming kernels     every other shape within 64 KB of LDS; fc_rows reads float4 columns when N % 4 == 0,
                               scalars otherwise, over G = 1024 / NQ k-groups

References: Linear-LReLU-Linear-LReLU-Linear as stock torch modules on the CPU in fp32 and fp64; grad_z from autograd on
E(z).sum(); chains by the reference's update z - float32(0.5 s^2) (g + z) + float32(s) xi.  Weights are synth.load_into's
(U[-1/sqrt(fan_in), 1/sqrt(fan_in)]), inputs synth normals of fixed seeds.

Rule (encoder_ops_util.check): |hip - fp64| <= 3 |torch fp32 - fp64| + 1e-6 in rel-L2 for the whole output, its last row
and (z, grad_z) its last column.  A diagnostic is one scalar sum: |hip - fp64| <= 3 |fp32 - fp64| + 1e-6 x the sum of
the absolute values of the terms it adds (check_scalar), the terms taken where the sum starts: w3_j h2_j and b3 for an
energy, z_i^2 / 2, g_i / (B nz).
"""
import functools

import numpy as np

from encoder_ops_util import (GUARD_WORD, KINK_REL, assert_guards_intact, check, distances, guarded,  # noqa: F401
                              is_pattern, report, reset_guards)

ERR_ARG, ERR_UNSUPPORTED = 1001, 1003
KERNEL_REG, KERNEL_MFMA, KERNEL_STREAM, KERNEL_NONE = 1, 2, 3, 0
STREAM_POSTERIOR, STREAM_PRIOR = 0x51, 0x52

SLOPE = 0.2
EXTRA_SLOPES = (0.0, -0.1)
N_STEPS = 3
PRIOR_STEP, POST_STEP = 0.4, 0.1   # the workload's prior step; a posterior step of the likelihood gradient's scale

R_CASES = {
    "R1": (1, 1, 1),        # register engine minimum
    "R2": (3, 13, 2),       # one wave's 13 rows exactly
    "R3": (63, 14, 3),      # the second wave owns one row
    "R4": (64, 64, 5),
    "R5": (65, 207, 2),     # one lane of the second column register, odd nh
    "R6": (128, 208, 3),    # the register kernel's full extent
    "R7": (100, 200, 4),    # the workload's own shape
}
S_CASES = {
    "S1": (128, 209, 3),    # first nh past the register kernel; scalar fc_rows for N = nh
    "S2": (129, 208, 3),    # odd nz: scalar fc_rows for N = nz
    "S3": (132, 212, 5),    # all float4; NQ = 53 and 33 do not divide 1024; odd B: a half-empty last workgroup
    "S4": (130, 256, 2),
    "S5": (2, 760, 3),
    "S6": None,             # (2, the largest nh the streaming kernels admit at nz = 2, 1): s6_shape()
}
# M1, M2, M4 and M5 have nh % 4 != 0: the MFMA tile's float4 runs along nh would leave their rows, so engine 2 refuses
# them and they run on engine 1 alone.  M7 - M9 keep the engine's minimum, its N and K tails and nz = 144 on the MFMA.
M_CASES = {
    "M1": (16, 1, 1),
    "M2": (16, 17, 15),
    "M3": (48, 200, 17),    # two chain tiles, ragged second; nh = 12 N tiles + 8 columns
    "M4": (128, 201, 33),
    "M5": (144, 202, 3),
    "M6": (256, 256, 16),   # the engine's full extent
    "M7": (16, 4, 1),       # MFMA minimum: one N tile of 4 live columns, K = 4 of 16
    "M8": (16, 20, 15),     # second N tile of 4 columns, K tail 4 of 16
    "M9": (144, 204, 3),    # nz past the register kernel: engine 1 streams
}
CASES = dict(R_CASES, **S_CASES, **M_CASES)
RS_IDS = list(R_CASES) + list(S_CASES)
M_IDS = list(M_CASES)
SLOPE_CASES = ("R4", "S3", "M3")

# the kernel each case reaches: (energy / gradient and posterior update, prior chain on engine 1, on engine 2)
KERNELS = {c: (1, 1, 0) for c in R_CASES}
KERNELS.update({c: (3, 3, 0) for c in S_CASES})
KERNELS.update(R4=(1, 1, 2), R6=(1, 1, 2))  # nz % 16 == 0 and nh % 4 == 0: the MFMA tile would take them as well
KERNELS.update(M1=(1, 1, 0), M2=(1, 1, 0), M3=(1, 1, 2), M4=(1, 1, 0), M5=(3, 3, 0), M6=(3, 3, 2), M7=(1, 1, 2),
               M8=(1, 1, 2), M9=(3, 3, 2))


def slopes_of(cid):
    return (SLOPE,) + (EXTRA_SLOPES if cid in SLOPE_CASES else ())


def runs(ids):
    """[(case id, slope)]: every case at 0.2, the SLOPE_CASES at 0.0 and -0.1 as well."""
    return [(c, s) for c in ids for s in slopes_of(c)]


def run_id(r):
    return "-".join(str(v) for v in r)


@functools.lru_cache(maxsize=None)
def s6_nh():
    """The largest nh with a streaming kernel at nz = 2, asked of the library (host only)."""
    from damc import _lib

    L = _lib.lib()
    ok = [nh for nh in range(1, 1100) if L.damc_ebm_kernel(2, nh, -1, 1) == KERNEL_STREAM]
    assert ok and ok == list(range(ok[0], ok[-1] + 1)) and ok[0] > 208, "the admitted nh at nz = 2 are one run past 208"
    return ok[-1]


def shape(cid):
    if cid == "S6":
        return (2, s6_nh(), 1)
    return CASES[cid]


# per-case seed offsets, moved only when a case's fp64 pre-activations come within KINK_REL of the kink
SEED_SHIFT = {}


def _seed(cid):
    return 9100 + 17 * sorted(CASES).index(cid) + SEED_SHIFT.get(cid, 0)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def net(cid, slope):
    """The case's E as a stock Sequential (fp32, CPU); the weights do not depend on the slope."""
    import torch

    from damc import synth

    nz, nh, _ = shape(cid)
    act = torch.nn.LeakyReLU(slope)
    return synth.load_into(torch.nn.Sequential(torch.nn.Linear(nz, nh), act, torch.nn.Linear(nh, nh), act,
                                               torch.nn.Linear(nh, 1)), _seed(cid))


@functools.lru_cache(maxsize=None)
def inputs(cid, nslab=1):
    """z (B, nz), noise (N_STEPS, B, nz), slabs (nslab, B, nz) of a likelihood gradient (their sum is N(0, 1)-sized)."""
    import torch

    from damc import synth

    nz, nh, B = shape(cid)
    s = _seed(cid)
    slabs = synth.normal_f32(s + 3, nslab, (nslab, B, nz)) / np.float32(np.sqrt(nslab))
    return dict(z=torch.from_numpy(synth.normal_f32(s + 1, 0, (B, nz))),
                noise=torch.from_numpy(synth.normal_f32(s + 2, 0, (N_STEPS, B, nz))),
                slabs=torch.from_numpy(slabs.astype(np.float32)))


def weights(cid, slope):
    """w1 (nh, nz), b1, w2 (nh, nh), b2, w3 (nh), b3 (1): PyTorch layouts, fp32."""
    m = net(cid, slope)
    w1, b1, w2, b2, w3, b3 = (p.detach() for p in m.parameters())
    return dict(w1=w1, b1=b1, w2=w2, b2=b2, w3=w3.reshape(-1), b3=b3.reshape(-1))


# ------------------------------------------------------------------------------------------------ references
def _eval(m, z):
    """E(z) per row, grad_z of its sum (autograd), the two pre-activations and sum |w3_j h2_j| + |b3| over the rows."""
    import torch

    zz = z.detach().clone().requires_grad_(True)
    a1 = m[0](zz)
    h1 = m[1](a1)
    a2 = m[2](h1)
    h2 = m[3](a2)
    e = m[4](h2).reshape(-1)
    (g,) = torch.autograd.grad(e.sum(), zz)
    terms = float((h2.detach() * m[4].weight.detach().reshape(1, -1)).abs().sum() +
                  z.shape[0] * m[4].bias.detach().abs().sum())
    return e.detach(), g, (a1.detach().numpy(), a2.detach().numpy()), terms


def _net_as(cid, slope, dt):
    import copy

    return copy.deepcopy(net(cid, slope)).to(dt)


@functools.lru_cache(maxsize=None)
def eg_refs(cid, slope):
    """(fp32, fp64) dicts {energy (B), grad (B, nz), pre, eterms}."""
    import torch

    out = []
    for dt in (torch.float32, torch.float64):
        e, g, pre, terms = _eval(_net_as(cid, slope, dt), inputs(cid)["z"].to(dt))
        out.append(dict(energy=e.numpy(), grad=g.numpy(), pre=list(pre), eterms=terms))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain_refs(cid, slope, with_noise=True):
    """(fp32, fp64) dicts of N_STEPS prior steps with the injected noise: z, diag (N_STEPS, 2) = {sum E, |z|^2 / 2}
    before each update, dterms (N_STEPS, 2) the sums of the diagnostics' absolute terms, pre (every step's)."""
    import torch

    c1, st = float(np.float32(0.5 * PRIOR_STEP * PRIOR_STEP)), float(np.float32(PRIOR_STEP))
    out = []
    for dt in (torch.float32, torch.float64):
        m = _net_as(cid, slope, dt)
        z = inputs(cid)["z"].to(dt)
        xi = inputs(cid)["noise"].to(dt)
        diag, dterms, pres = [], [], []
        for i in range(N_STEPS):
            e, g, pre, terms = _eval(m, z)
            zz = float((z * z).sum()) * 0.5
            diag.append([float(e.sum()), zz])
            dterms.append([terms, zz])
            pres += list(pre)
            z = z - c1 * (g + z)
            if with_noise:
                z = z + st * xi[i]
        out.append(dict(z=z.numpy(), diag=np.array(diag), dterms=np.array(dterms), pre=pres))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def post_refs(cid, slope, nslab=1, with_noise=True, use_ebm=True):
    """(fp32, fp64) dicts of one posterior update: z, diag (4) = {sum E, 0, |z|^2 / 2, mean g} and dterms (4)."""
    import torch

    c1, st = float(np.float32(0.5 * POST_STEP * POST_STEP)), float(np.float32(POST_STEP))
    out = []
    for dt in (torch.float32, torch.float64):
        z = inputs(cid)["z"].to(dt)
        xi = inputs(cid)["noise"][0].to(dt)
        sl = inputs(cid, nslab)["slabs"].to(dt)
        g = sl[0].clone()
        for k in range(1, nslab):
            g = g + sl[k]
        esum = eterms = 0.0
        if use_ebm:
            e, ge, _, eterms = _eval(_net_as(cid, slope, dt), z)
            g = g + ge
            esum = float(e.sum())
        g = g + z
        zz = float((z * z).sum()) * 0.5
        zn = z - c1 * g
        if with_noise:
            zn = zn + st * xi
        n = z.numel()
        out.append(dict(z=zn.numpy(), diag=np.array([esum, 0.0, zz, float(g.sum()) / n]),
                        dterms=np.array([eterms, 0.0, zz, float(g.abs().sum()) / n])))
    return tuple(out)


def kink_margin(pre64):
    """min |pre-activation| / rms of its layer (train_ops_util.seq_kink_margin)."""
    return min(float(np.abs(a).min() / np.sqrt(np.mean(a * a))) for a in pre64)


# ------------------------------------------------------------------------------------------------ the bound
ROW_SLICES = (("lastrow", (-1,)),)                                  # energy (B)
MAT_SLICES = (("lastrow", (-1,)), ("lastcol", (Ellipsis, -1)))      # z, grad_z (B, nz)


def scalar_rows(name, got, ref32, ref64, terms):
    """[(label, |hip - fp64|, 3 |fp32 - fp64| + 1e-6 terms)] per scalar, printed."""
    got, ref32, ref64, terms = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, ref32, ref64, terms))
    assert np.isfinite(got).all(), name + ": non-finite diagnostic"
    rows = []
    for i in range(got.size):
        e, e32 = abs(got[i] - ref64[i]), abs(ref32[i] - ref64[i])
        print("%-58s [%d]       hip-fp64 %.3e  torch32-fp64 %.3e  terms %.3e" % (name, i, e, e32, terms[i]))
        rows.append(("%s[%d]" % (name, i), e, 3.0 * e32 + 1e-6 * terms[i]))
    return rows


def check_scalar(name, got, ref32, ref64, terms):
    for label, e, bound in scalar_rows(name, got, ref32, ref64, terms):
        assert e <= bound, (label, e, bound)


def check_pair(name, a, b, ref32, ref64, slices=MAT_SLICES):
    """Two engines' results under the rule: |a - b| <= 3 |torch32 - fp64| + 1e-6, each in units of |fp64|."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    for label, e, e32 in report(name, ref64 + d, ref32, ref64, slices):
        assert e <= 3.0 * e32 + 1e-6, (name, label, e, e32)


def limbs_of(z):
    """z (B, nz) fp32 tensor -> its x3 limbs as int16 [B][nz / 8][3][8]: bf16(v), bf16(v - h), bf16(v - h - m)."""
    import torch

    B, nz = z.shape
    h = z.to(torch.bfloat16)
    r1 = z - h.float()
    m = r1.to(torch.bfloat16)
    lo = (r1 - m.float()).to(torch.bfloat16)
    return torch.stack([t.view(torch.int16).reshape(B, nz // 8, 8) for t in (h, m, lo)], dim=2).contiguous()
