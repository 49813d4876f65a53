"""Shared by tests/test_train_ops_cases_cpu.py and tests/test_gpu_train_ops.py: the case tables of the Q and E updates'
per-op training calls of include/damc.h (damc_denoiser_train_*, damc_ebm_train_*, damc_prior_emb_train_*,
damc_q_loss_*, damc_q_noise_glue), their fp32 / fp64 PyTorch-CPU references, the descriptors and the accuracy rule.

Rule (the project's per-op rule, encoder_ops_util): per tensor |hip - fp64| <= 3 |torch fp32 (CPU) - fp64| + 1e-6 in
rel-L2.  A gradient's denominator is its fp64 norm floored at 1e-3 x the largest gradient norm of the call
(test_gpu_toyq_train._errs); a forward value is measured against its own norm.

The denoiser's time embedding is evaluated ONCE, in fp32 (SinusoidalPosEmb of the logsnr input, as the library's caller
does), and that same `se` feeds the library and, cast, both references: each precision evaluating its own
sin(1000 f t) would put ~3e-5 between them that no kernel under test produces.

Denoiser cases (nz, nxemb, ntemb, nf, B, residual); weights synth.load_into(p, 31 + nz); inputs from synth streams nz of
seeds 41 (zt), 42 (xemb), 43 (logsnr, U[-5, 9]), 44 (grad_eps).  What each case reaches (csrc/denoiser_train.hip
Grp::run / gemm(), csrc/gemm.hip launch_small_gemm*, csrc/wgrad.hip launch_colsum):
  D1  B = 130, B % 4 != 0 and >= 97: every K = B member leaves the grouped kernel; weight gradients (M = 2 dout <= 256)
      run the tiled engine's scalar gather split over K (5 K tiles, 2 slices, the last 34 wide) plus the slab sum; column
      sums on launch_colsum; nz / 2 = 6: the dzp product has K % 4 != 0; activation products on launch_small_gemm with a
      2-row M tail
  D2  ntemb = 6: the time MLP's products have lda = 6; the stacked ctx GEMM has K = 18 and the scalar route; B = 37
  D3  nz = 100 (nz / 2 = 50 as N forward and K backward) at a ragged batch above 128
  D4  everything aligned: the grouped kernel for every stage; also under DAMC_DN_GROUP=0 and DAMC_DN_SMALL_GEMM=0 (the
      tiled engine with aligned split-K)
  D5  B = 514 > 512: two-stage launch_colsum, 17 K tiles in 6 slices (the last 34 wide), M = B > 256 (no slab) for the
      activation products
  D6  the smallest of everything: K = 2, M = 5, T = 4
  D7  aligned, K = B = 132: the grouped kernel's fourth wave idle (runs of 48, 48, 36, 0)
  D8  one exact M tile, K = 16: three idle waves
  D9  nz = 2, the toy amortizer's latent (nz % 4 != 0): out2 padded to 4 columns inside the workspace, the K = nz and
      K = nz / 2 products as kernels of their own, eps and grad_eps through repad_rows_kernel; at D1's ragged batch
"""
import copy
import ctypes
import functools
import math

import numpy as np

from encoder_ops_util import (KINK_REL, assert_guards_intact, check, distances, guarded, is_pattern,  # noqa: F401
                              report, reset_guards)

# ------------------------------------------------------------------------------------------------ case tables
DN_CASES = {
    "D1": (12, 8, 8, 1, 130, True),
    "D2": (8, 12, 6, 1, 37, False),
    "D3": (100, 16, 16, 1, 130, True),
    "D4": (128, 64, 32, 2, 128, True),
    "D5": (12, 8, 8, 1, 514, False),
    "D6": (4, 4, 4, 1, 5, True),
    "D7": (12, 8, 8, 1, 132, True),
    "D8": (12, 8, 8, 1, 16, True),
    "D9": (2, 8, 8, 1, 130, True),
}
DN_IDS = list(DN_CASES)
DN_ENVS = {"default": {}, "group0": {"DAMC_DN_GROUP": "0"}, "smallgemm0": {"DAMC_DN_SMALL_GEMM": "0"}}
DN_SEED_W, DN_SEED_ZT, DN_SEED_XEMB, DN_SEED_LOGSNR, DN_SEED_GRAD = 31, 41, 42, 43, 44
DN_TAIL_CASES = ("D1", "D5")
DN_TAIL_PARAMS = ("wl[4]", "wctx[6]")
DN_SPLITS = {"D1": (2, 34), "D5": (6, 34)}  # gemm()'s (slices, last slice width) of a K = B weight gradient
GROUP_RUNS = {8: (8, 0, 0, 0), 16: (16, 0, 0, 0), 132: (48, 48, 36, 0), 260: (80, 80, 80, 20),
              514: (144, 144, 144, 82)}  # the grouped kernel's per-wave K runs (514: the arithmetic; K % 4 is refused)

# E update: (B, nz, nh), slope 0.2; weights synth.load_into(seed 51), z / grad_energy from seeds 52 / 53, stream B
E_SLOPE = 0.2
E_CASES = [(4, 4, 4),
           (20, 100, 200),    # the net's own ndf = 200: a 13th column tile 8 wide
           (132, 12, 36),     # K = B = 132: an idle fourth wave
           (260, 128, 200)]
E_SEED_W, E_SEED_Z, E_SEED_G = 51, 52, 53
# prior embedding: ((B, nz, nh, nout), slope); weights seed 61, noise / grad_out from seeds 62 / 63, stream B
PE_CASES = [((4, 4, 4, 4), 0.01), ((20, 100, 128, 36), 0.01), ((132, 12, 128, 260), 0.01), ((20, 100, 128, 36), 0.0)]
PE_SEED_W, PE_SEED_X, PE_SEED_G = 61, 62, 63
QLOSS_CASES = [(1, 2), (5, 100), (3, 130)]           # (B, nz); eps / pred from seeds 71 / 72, stream nz
GLUE_CASES = [(1, 2, 128), (5, 128, 8), (3, 100, 16)]  # (B, nz, ntemb); u / z / eps from seeds 73 / 74 / 75
GLUE_LOGSNR = (-5.1, 9.8)


def case_id(t):
    return "-".join(str(v).replace(".", "p") for v in (t if isinstance(t, (tuple, list)) else (t,)))


# ------------------------------------------------------------------------------------------------ route arithmetic
def gemm_split(M, N, K, slab=True):
    """(slices, last slice width) of csrc/denoiser_train.hip gemm() on the tiled engine: 128 x 128 output tiles, K tiles
    of 32, at most 16 slices of at least 2 K tiles, only with fewer than 64 output tiles and at least 4 K tiles."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    kt = (K + 31) // 32
    S = 1
    if slab and tiles < 64 and kt >= 4:
        S = min(16, max(1, min(kt // 2, 128 // tiles)))
    if S <= 1:
        return 1, K
    kper = (kt + S - 1) // S * 32
    S = (K + kper - 1) // kper
    return S, K - (S - 1) * kper


def group_runs(K):
    """The K run of each of the four waves of small_gemm_group_kernel: ceil(ceil(K / 16) / 4) 16-k steps per wave."""
    per = ((K + 15) // 16 + 3) // 4 * 16
    return tuple(max(0, min(K, (w + 1) * per) - w * per) for w in range(4))


def dn_widths(cid):
    """(din, dout) of the seven blocks of the case's Diffusion_UnetA."""
    nz, nxemb, ntemb, nf, B, residual = DN_CASES[cid]
    w = 32 * nf
    return [(2 * nz, w), (w, 2 * w), (2 * w, 2 * w), (2 * w, 2 * w), (4 * w, 2 * w), (4 * w, w), (2 * w, nz)]


# ------------------------------------------------------------------------------------------------ denoiser
@functools.lru_cache(maxsize=None)
def dn_case(cid):
    """The case's net (CPU, fp32) and inputs: zt, xemb, se (the fp32 time embedding), grad_eps as CPU tensors."""
    import torch

    from damc import synth
    from src import diffusion_net as dn

    nz, nxemb, ntemb, nf, B, residual = DN_CASES[cid]
    p = synth.load_into(dn.Diffusion_UnetA(nz, nxemb, ntemb, residual, nf), DN_SEED_W + nz)
    zt = torch.from_numpy(synth.normal_f32(DN_SEED_ZT, nz, (B, nz)))
    xemb = torch.from_numpy(synth.normal_f32(DN_SEED_XEMB, nz, (B, nxemb)))
    logsnr = torch.from_numpy(synth.uniform_f32(DN_SEED_LOGSNR, nz, (B,), -5, 9))
    grad_eps = torch.from_numpy(synth.normal_f32(DN_SEED_GRAD, nz, (B, nz)))
    with torch.no_grad():
        t_in = torch.arctan(torch.exp(-0.5 * torch.clamp(logsnr, -20.0, 20.0))) / (0.5 * math.pi)
        se = p.time_mlp[0](t_in).contiguous()
    assert se.dtype == torch.float32 and se.shape == (B, ntemb)
    return dict(p=p, zt=zt, xemb=xemb, se=se, grad_eps=grad_eps)


def dn_param_names(p):
    """The 68 parameters in the library's order (damc.training._denoiser_params): 'tw1', 'wl[4]', ..."""
    from damc import training

    return [key if b is None else "%s[%d]" % (key, b) for key, b, _ in training._denoiser_params(p)]


def _dn_eval(cid, dt, perm=None):
    """time_mlp[1:] and Diffusion_UnetA.forward's stock body (tests/test_gpu_training._stock_denoiser) in dtype dt on
    the CPU, backward from grad_eps.  perm: the batch rows evaluated in that order (outputs returned in the case's)."""
    import torch
    import torch.nn.functional as F

    from damc import training

    c = dn_case(cid)
    p = copy.deepcopy(c["p"]).to(dt)
    idx = torch.arange(c["zt"].shape[0]) if perm is None else torch.as_tensor(np.asarray(perm), dtype=torch.long)
    z, xe = (c[k][idx].to(dt).clone().requires_grad_(True) for k in ("zt", "xemb"))
    se, g = c["se"][idx].to(dt), c["grad_eps"][idx].to(dt)
    tm = p.time_mlp
    temb = tm[3](tm[2](tm[1](se)))
    ctx = torch.cat([temb, xe], dim=1)
    skips, pre, out = [], [], p.input_emb(z)
    for layer in p.in_layers:
        out = layer(ctx=ctx, x=out)
        skips.append(out)
        pre.append(out)
        out = F.leaky_relu(out, negative_slope=0.01)
    out = p.mid_layers[0](ctx=ctx, x=out)
    pre.append(out)
    for i, layer in enumerate(p.out_layers):
        out = layer(ctx=ctx, x=F.leaky_relu(torch.cat([out, skips.pop()], dim=1), negative_slope=0.01))
        if i < 2:
            pre.append(out)
    eps = z + out if p.residual else out
    eps.backward(g)
    inv = torch.argsort(idx)
    res = dict(eps_pred=eps.detach()[inv].numpy(), grad_zt=z.grad[inv].numpy(), grad_xemb=xe.grad[inv].numpy())
    for name, (_, _, t) in zip(dn_param_names(p), training._denoiser_params(p)):
        res[name] = t.grad.numpy()
    res["_pre"] = [t.detach().numpy() for t in pre]  # the six activated blocks' outputs (LeakyReLU pre-activations)
    return res


@functools.lru_cache(maxsize=None)
def dn_refs(cid):
    """(torch fp32, fp64) dicts: eps_pred, grad_zt, grad_xemb and the 68 parameter gradients by name."""
    import torch

    return _dn_eval(cid, torch.float32), _dn_eval(cid, torch.float64)


def dn_permuted_fp32(cid):
    """The fp32 reference with the batch in another (fixed) order: another summation order of every K = B product."""
    import torch

    from damc import synth

    B = DN_CASES[cid][4]
    return _dn_eval(cid, torch.float32, perm=np.argsort(synth.uniform(45, B, B), kind="stable"))


def dn_kink_margin(cid):
    """min |pre-activation| / rms of its layer over the six activated blocks, fp64."""
    return min(float(np.abs(a).min() / np.sqrt(np.mean(a * a))) for a in dn_refs(cid)[1]["_pre"])


DN_FWD = ("eps_pred",)


def dn_tensor_names(cid):
    return ["eps_pred", "grad_zt", "grad_xemb"] + dn_param_names(dn_case(cid)["p"])


def rule_rows(names, got, ref32, ref64, fwd=()):
    """[(name, |got - fp64|, |torch32 - fp64|)] for the named tensors of the three dicts.  fwd: the forward values
    (own norm); every other tensor is a gradient, its denominator floored at 1e-3 x the largest gradient norm."""
    grads = [n for n in names if n not in fwd]
    floor = 1e-3 * max([float(np.linalg.norm(np.asarray(ref64[n], dtype=np.float64))) for n in grads] or [0.0])
    rows = []
    for n in names:
        r = np.asarray(ref64[n], dtype=np.float64)
        a, b = np.asarray(got[n], dtype=np.float64), np.asarray(ref32[n], dtype=np.float64)
        assert a.shape == r.shape == b.shape, (n, a.shape, b.shape, r.shape)
        assert np.isfinite(a).all(), n + ": non-finite output"
        den = max(float(np.linalg.norm(r)), 1e-30 if n in fwd else floor, 1e-30)
        rows.append((n, float(np.linalg.norm(a - r)) / den, float(np.linalg.norm(b - r)) / den))
    return rows


def check_rows(label, rows):
    """Print every pair of distances, then assert |got - fp64| <= 3 |torch32 - fp64| + 1e-6 for each."""
    for n, e, e32 in rows:
        print("%-34s %-12s hip-fp64 %.3e  torch32-fp64 %.3e" % (label, n, e, e32))
    bad = [(n, e, e32) for n, e, e32 in rows if not e <= 3.0 * e32 + 1e-6]
    assert not bad, (label, bad)


def dn_desc(p, addr):
    """damc_denoiser_train_t of the module p with addr(name, tensor) as each weight's address."""
    from damc import _lib, training

    d = _lib.DenoiserTrain()
    d.nz, d.ntemb, d.nxemb, d.residual = p.nz, p.ntemb, p.nxemb, int(bool(p.residual))
    for name, (key, b, t) in zip(dn_param_names(p), training._denoiser_params(p)):
        a = addr(name, t)
        if b is None:
            setattr(d, key, a)
        elif key in ("wctx", "bctx"):
            getattr(d, key)[b] = a
        else:
            setattr(d.blocks[b], key, a)
    for b, blk in enumerate(training._blocks_of(p)):
        d.blocks[b].din, d.blocks[b].dout = blk._layer[0].in_features, blk._layer[0].out_features
    return d


def dn_grads_struct(p, addr):
    """damc_denoiser_grads_t with addr(name) (an address, or None for a NULL entry) per parameter."""
    from damc import _lib, training

    g = _lib.DenoiserGrads()
    for name, (key, b, _) in zip(dn_param_names(p), training._denoiser_params(p)):
        a = addr(name)
        if a is None:
            continue
        if b is None:
            setattr(g, key, a)
        else:
            getattr(g, key)[b] = a
    return g


# ------------------------------------------------------------------------------------------------ E update
def _seq_grads(seq, x, g, dt, want_x):
    """seq(x) in dtype dt on the CPU with its hidden activations, backward from g: (activations, output, grads, dx,
    the LeakyReLUs' pre-activations)."""
    import torch

    m = copy.deepcopy(seq).to(dt)
    xx = x.to(dt).clone().requires_grad_(want_x)
    acts, pre, h = [], [], xx
    for mod in m:
        if isinstance(mod, torch.nn.LeakyReLU):
            pre.append(h.detach().numpy())
        h = mod(h)
        if isinstance(mod, torch.nn.LeakyReLU):
            acts.append(h)
    h.backward(g.to(dt).reshape(h.shape))
    return ([a.detach().numpy() for a in acts], h.detach().numpy(), [q.grad.numpy() for q in m.parameters()],
            xx.grad.numpy() if want_x else None, pre)


@functools.lru_cache(maxsize=None)
def e_case(case):
    import torch

    from damc import synth

    B, nz, nh = case
    seq = synth.load_into(torch.nn.Sequential(torch.nn.Linear(nz, nh), torch.nn.LeakyReLU(E_SLOPE),
                                              torch.nn.Linear(nh, nh), torch.nn.LeakyReLU(E_SLOPE),
                                              torch.nn.Linear(nh, 1)), E_SEED_W)
    z = torch.from_numpy(synth.normal_f32(E_SEED_Z, B, (B, nz)))
    g = torch.from_numpy(synth.normal_f32(E_SEED_G, B, (B,)))
    return seq, z, g


E_NAMES = ("h1", "h2", "energy", "w1", "b1", "w2", "b2", "w3", "b3", "grad_z")
E_FWD = ("h1", "h2", "energy")


@functools.lru_cache(maxsize=None)
def e_refs(case):
    """(torch fp32, fp64) dicts of E_NAMES: the stock nn.Linear / LeakyReLU modules on the CPU."""
    import torch

    seq, z, g = e_case(case)
    out = []
    for dt in (torch.float32, torch.float64):
        acts, e, gr, dz, pre = _seq_grads(seq, z, g, dt, True)
        d = dict(h1=acts[0], h2=acts[1], energy=e.reshape(-1), grad_z=dz, _pre=pre)
        d.update(zip(("w1", "b1", "w2", "b2", "w3", "b3"), gr))
        out.append(d)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ prior embedding
@functools.lru_cache(maxsize=None)
def pe_case(case, slope):
    import torch

    from damc import synth

    B, nz, nh, nout = case
    seq = synth.load_into(torch.nn.Sequential(torch.nn.Linear(nz, nh), torch.nn.LeakyReLU(slope),
                                              torch.nn.Linear(nh, nout)), PE_SEED_W)
    x = torch.from_numpy(synth.normal_f32(PE_SEED_X, B, (B, nz)))
    g = torch.from_numpy(synth.normal_f32(PE_SEED_G, B, (B, nout)))
    return seq, x, g


PE_NAMES = ("h", "out", "w1", "b1", "w2", "b2")
PE_FWD = ("h", "out")


@functools.lru_cache(maxsize=None)
def pe_refs(case, slope):
    import torch

    seq, x, g = pe_case(case, slope)
    out = []
    for dt in (torch.float32, torch.float64):
        acts, o, gr, _, pre = _seq_grads(seq, x, g, dt, False)
        d = dict(h=acts[0], out=o, _pre=pre)
        d.update(zip(("w1", "b1", "w2", "b2"), gr))
        out.append(d)
    return tuple(out)


def seq_kink_margin(pre64):
    """min |pre-activation| / rms of its layer over the LeakyReLUs' inputs."""
    return min(float(np.abs(a).min() / np.sqrt(np.mean(a * a))) for a in pre64)


# ------------------------------------------------------------------------------------------------ q_loss
@functools.lru_cache(maxsize=None)
def qloss_inputs(case):
    import torch

    from damc import synth

    B, nz = case
    return (torch.from_numpy(synth.normal_f32(71, nz, (B, nz))), torch.from_numpy(synth.normal_f32(72, nz, (B, nz))))


def qloss_ref(case, dt, g=None):
    """loss (B) = 0.5 * sum((eps - pred) ** 2, 1) in dtype dt on the CPU, and d loss / d pred for the upstream g (B)."""
    import torch

    eps, pred = (t.to(dt) for t in qloss_inputs(case))
    pr = pred.clone().requires_grad_(True)
    loss = 0.5 * torch.sum((eps - pr) ** 2, 1)
    if g is None:
        return loss.detach().numpy(), None
    loss.backward(g.to(dt))
    return loss.detach().numpy(), pr.grad.numpy()


def c_float(v):
    return ctypes.c_float(float(v))
