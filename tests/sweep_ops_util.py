"""Shared by tests/test_sweep_ops_cases_cpu.py and tests/test_gpu_sweep_ops.py: the case table of the reverse sweep
(damc_reverse_sweep, damc_denoise_step of include/damc.h), the form and the per-call stages each case has to reach, and
the fp32 / fp64 PyTorch-CPU reference of the sweep.

A case is (nz, w, ntemb, nxemb, B, residual), w = in0's dout; the block widths follow validate()'s table
(din 2 nz, w, 2 w, 2 w, 4 w, 4 w, 2 w; dout w, 2 w, 2 w, 2 w, 2 w, w, nz).  The weights are plain tensors, not a
Diffusion_UnetA (which only has w = 32 nf): Linear weights and biases U[-1/sqrt(fan_in), 1/sqrt(fan_in)] and p.B
N(0, 1) from damc.synth's counter hash, zt0 / xemb / injected noise synth normals of fixed seeds.

Reference: Diffusion_UnetA.forward (src/diffusion_net.py) and the reverse step restated as one plain function on the host
tables the library takes (damc.amortizer.step_tables: temb_in (n, ntemb), coef (n, 6)), so the sin / cos of ~1000 rad
stay out of the comparison; evaluated in fp32 and in fp64 on the same fp32 weights.

Rule (encoder_ops_util.check): |hip - fp64| <= 3 |torch fp32 - fp64| + 1e-6 in rel-L2 for the whole output, its last
row and its last column; for the eps of every step and for the end point zt.

Forms (damc_sweep_form): 0 none, 1 row-resident, 2 team launch on the generic kernel, 3 team launch on
sweep_fast_kernel, 4 launch chain.  Stages (damc_sweep_stages): bit 0 skinny, bit 1 narrow out2, bit 2 the row image
fits, bits 8-14 the blocks whose hyper GEMM runs on the limb product (all of a call's blocks or none).
"""
import ctypes
import functools
import math

import numpy as np

from encoder_ops_util import (GUARD_WORD, assert_guards_intact, check, distances, guarded, is_pattern,  # noqa: F401
                              report, reset_guards)

ERR_ARG, ERR_UNSUPPORTED = 1001, 1003
FORM_NONE, FORM_ROWS, FORM_TEAM, FORM_FAST, FORM_CHAIN = 0, 1, 2, 3, 4
ST_SKINNY, ST_NARROW, ST_ROWS_FIT = 1, 2, 4
LIMB7, LIMB6 = 0x7F00, 0x3F00
STREAM_SWEEP = 0x53

N_STEPS = 3
LOGSNR_MIN, LOGSNR_MAX, VAR_TYPE = -5.1, 9.8, "large"
LONG_STEPS = 257   # one more than the team kernels' LDS step table holds (TS_TAB_STEPS = 256)

T_CASES = {
    "T1": (4, 32, 32, 64, 1, 1),      # nz minimum of the float4 forms: in0 din 8, out2 one half-filled column tile; B = 1
    "T2": (8, 16, 16, 4, 17, 0),      # w < 32: fewer column tiles than team slots; second row tile of one row; no residual
    "T3": (20, 36, 32, 64, 16, 1),    # dout % 8 == 4 in every block; fp32 hyper; kpad / pad64 of 72 and 144; a full row tile
    "T4": (36, 48, 24, 10, 5, 1),     # ntemb % 16 != 0, nxemb % 4 != 0: launch_gemm's scalar-A route with K = 10 and 24
    "T5": (128, 32, 32, 64, 15, 1),   # 8 k-groups of the in0 embedding on the generic kernel: not the fast one at w = 32
}
F_CASES = {
    "F1": (100, 128, 16, 8, 18, 0),   # sweep_fast_kernel<100, 128>, residual 0, ntemb / nxemb of no golden
}
W_CASES = {
    "W1": (64, 160, 32, 64, 4, 1),    # limb hyper at dout 160 and 320
    "W2": (128, 288, 16, 4, 2, 1),    # 2 w = 576 > 512: fp32 hyper; too wide for a team and for the row image
}
N_CASES = {
    "N1": (2, 16, 16, 4, 1, 0),       # row-resident minimum
    "N2": (6, 32, 32, 8, 17, 1),      # nz % 4 == 2: Philox quads straddle the row end
    "N3": (126, 64, 16, 64, 16, 1),   # the largest narrow nz
    "N4": None,                       # (10, the largest admitted w % 16 == 0, 16, 4, 3, 1): n4_width()
}
CASES = dict(T_CASES, **F_CASES, **W_CASES, **N_CASES)
WIDE_IDS = list(T_CASES) + list(F_CASES) + list(W_CASES)
N_IDS = list(N_CASES)

# damc_sweep_stages of each case, from validate()'s and the stages' rules by hand.  skinny needs ntemb % 16 == 0,
# nxemb % 4 == 0 and EVERY stage block's dout % 16 == 0, out2's dout = nz included unless nz % 4 != 0: of the T cases
# only T5; the limb hyper needs every stage block's dout % 32 == 0 and <= 512, so nz % 32 == 0 too unless narrow.
# The row image is kpad(2 nz) + 8 w + max(w + pad64(w), pad64(2 w)) + 4 floats x 16 rows within 156 KB: W1 1764 floats
# fits, W2 (>= 256 + 9 x 288) does not; N4: n4_stages().
STAGES = {
    "T1": ST_ROWS_FIT, "T2": ST_ROWS_FIT, "T3": ST_ROWS_FIT, "T4": ST_ROWS_FIT,
    "T5": ST_SKINNY | ST_ROWS_FIT | LIMB7,
    "F1": ST_ROWS_FIT,
    "W1": ST_SKINNY | ST_ROWS_FIT | LIMB7,
    "W2": ST_SKINNY,
    "N1": ST_SKINNY | ST_NARROW | ST_ROWS_FIT,
    "N2": ST_SKINNY | ST_NARROW | ST_ROWS_FIT | LIMB6,
    "N3": ST_SKINNY | ST_NARROW | ST_ROWS_FIT | LIMB6,
}
# the default form on a device whose CUs split into 8 groups (MI355X: 256 CUs, 32 slots per team); W1's is the device's
DEFAULT_FORM = {"T1": FORM_TEAM, "T2": FORM_TEAM, "T3": FORM_TEAM, "T4": FORM_TEAM, "T5": FORM_TEAM, "F1": FORM_FAST,
                "W1": None, "W2": FORM_CHAIN, "N1": FORM_ROWS, "N2": FORM_ROWS, "N3": FORM_ROWS, "N4": FORM_ROWS}

# (what, descriptor arguments, null field, code): refused by validate(), host only
REFUSALS = [
    ("nz3", dict(nz=3, w=32, ntemb=32, nxemb=64), None, ERR_ARG),
    ("nz132", dict(nz=132, w=32, ntemb=32, nxemb=64), None, ERR_UNSUPPORTED),
    ("nz130", dict(nz=130, w=32, ntemb=32, nxemb=64), None, ERR_UNSUPPORTED),
    ("nz6-ntemb24", dict(nz=6, w=32, ntemb=24, nxemb=8), None, ERR_UNSUPPORTED),
    ("nz6-nxemb6", dict(nz=6, w=32, ntemb=32, nxemb=6), None, ERR_UNSUPPORTED),
    ("nz6-w36", dict(nz=6, w=36, ntemb=32, nxemb=8), None, ERR_UNSUPPORTED),
    ("w34", dict(nz=8, w=34, ntemb=32, nxemb=64), None, ERR_UNSUPPORTED),
    ("null-wg", dict(nz=8, w=32, ntemb=32, nxemb=64), ("blocks", 3, "wg"), ERR_ARG),
    ("null-bmat", dict(nz=8, w=32, ntemb=32, nxemb=64), ("bmat",), ERR_ARG),
]


def block_dims(nz, w):
    """(din, dout) of in0 in1 in2 mid out0 out1 out2."""
    return list(zip((2 * nz, w, 2 * w, 2 * w, 4 * w, 4 * w, 2 * w), (w, 2 * w, 2 * w, 2 * w, 2 * w, w, nz)))


# ------------------------------------------------------------------------------------------- host-only descriptors
_DUMMY = 0x1000  # a non-null, 16-byte-aligned address no host query dereferences


def host_desc(nz, w, ntemb, nxemb, residual=1, null=None):
    """A damc_denoiser_t for the host-only queries (validate() tests pointers for NULL only)."""
    from damc import _lib

    d = _lib.Denoiser()
    d.nz, d.ntemb, d.nxemb, d.residual = nz, ntemb, nxemb, residual
    for k in ("bmat", "tw1", "tb1", "tw2", "tb2"):
        setattr(d, k, _DUMMY)
    for j, (din, dout) in enumerate(block_dims(nz, w)):
        b = d.blocks[j]
        b.din, b.dout = din, dout
        for k in ("wl", "bl", "ws", "bs", "wg", "bg", "wb"):
            setattr(b, k, _DUMMY)
        d.wctx[j] = _DUMMY
        d.bctx[j] = _DUMMY
    if null is not None:
        if len(null) == 1:
            setattr(d, null[0], None)
        else:
            setattr(d.blocks[null[1]], null[2], None)
    return d


def n4_admitted():
    """The widths w % 16 == 0 damc_sweep_workspace_bytes admits at nz = 10 (host only)."""
    from damc import _lib

    L = _lib.lib()
    return [w for w in range(16, 1025, 16)
            if L.damc_sweep_workspace_bytes(ctypes.byref(host_desc(10, w, 16, 4)), 3, N_STEPS) > 0]


@functools.lru_cache(maxsize=None)
def n4_width():
    ok = n4_admitted()
    assert ok and ok == list(range(16, ok[-1] + 16, 16)), "the admitted widths at nz = 10 are one run from 16"
    return ok[-1]


def n4_stages():
    w = n4_width()
    return ST_SKINNY | ST_NARROW | ST_ROWS_FIT | (LIMB6 if w % 32 == 0 and 2 * w <= 512 else 0)


def shape(cid):
    if cid == "N4":
        return (10, n4_width(), 16, 4, 3, 1)
    return CASES[cid]


def stages_of(cid):
    return n4_stages() if cid == "N4" else STAGES[cid]


def _seed(cid):
    return 7300 + 19 * sorted(CASES).index(cid)


# ------------------------------------------------------------------------------------------------ inputs
WEIGHT_KEYS = ("wl", "bl", "ws", "bs", "wg", "bg", "wb", "wctx", "bctx")


@functools.lru_cache(maxsize=None)
def weights(cid):
    """{bmat, tw1, tb1, tw2, tb2, blocks: [7 x {wl bl ws bs wg bg wb wctx bctx}]}: fp32 CPU tensors, PyTorch layouts."""
    import torch

    from damc import synth

    nz, w, nt, nx, _, _ = shape(cid)
    s, stream = _seed(cid), [0]

    def lin(out, fin, bias=True):
        b = 1.0 / math.sqrt(fin)
        stream[0] += 2
        wt = torch.from_numpy(synth.uniform_f32(s, stream[0], (out, fin), -b, b))
        bs = torch.from_numpy(synth.uniform_f32(s, stream[0] + 1, (out,), -b, b)) if bias else None
        return wt, bs

    W = dict(bmat=torch.from_numpy(synth.normal_f32(s, 1, (nz, nz // 2))))
    W["tw1"], W["tb1"] = lin(nt, nt)
    W["tw2"], W["tb2"] = lin(nt, nt)
    W["blocks"] = []
    for din, dout in block_dims(nz, w):
        b = {}
        b["wl"], b["bl"] = lin(dout, din)
        b["ws"], b["bs"] = lin(dout, din)
        b["wg"], b["bg"] = lin(dout, dout)
        b["wb"], _ = lin(dout, dout, bias=False)
        b["wctx"], b["bctx"] = lin(dout, nt + nx)
        W["blocks"].append(b)
    return W


@functools.lru_cache(maxsize=None)
def inputs(cid, n=N_STEPS):
    """zt0 (B, nz), xemb (B, nxemb), noise (n - 1, B, nz): fp32 CPU tensors."""
    import torch

    from damc import synth

    nz, w, nt, nx, B, _ = shape(cid)
    s = _seed(cid)
    return dict(zt0=torch.from_numpy(synth.normal_f32(s + 1, 0, (B, nz))),
                xemb=torch.from_numpy(synth.normal_f32(s + 2, 0, (B, nx))),
                noise=torch.from_numpy(synth.normal_f32(s + 3, n, (max(n - 1, 1), B, nz)))[:n - 1].contiguous())


@functools.lru_cache(maxsize=None)
def tables(n, ntemb):
    """(coef (n, 6), temb_in (n, ntemb)) of the default schedule: the host tables the library takes."""
    from damc import amortizer

    coef, temb = amortizer.step_tables(n, LOGSNR_MIN, LOGSNR_MAX, VAR_TYPE, ntemb)
    return coef.contiguous(), temb.contiguous()


def single_step_tables(ntemb):
    """A caller-built one-row table: the default 3-step schedule's first row with is_last set."""
    coef, temb = tables(N_STEPS, ntemb)
    c = coef[0:1].clone()
    c[0, 5] = 1.0
    return c.contiguous(), temb[0:1].contiguous()


# ------------------------------------------------------------------------------------------------ reference
def denoise(W, z, temb_row, xemb, residual):
    """Diffusion_UnetA.forward on the time embedding's input row temb_row (ntemb): eps (B, nz), in z's dtype."""
    import torch
    import torch.nn.functional as F

    dt = z.dtype
    c = lambda t: t.to(dt)  # noqa: E731
    temb = F.linear(F.silu(F.linear(c(temb_row)[None, :], c(W["tw1"]), c(W["tb1"]))), c(W["tw2"]), c(W["tb2"]))
    ctx = torch.cat([temb.expand(z.shape[0], -1), c(xemb)], dim=1)

    def block(b, x):
        cc = F.silu(F.linear(F.silu(ctx), c(b["wctx"]), c(b["bctx"])))
        return (F.linear(x, c(b["wl"]), c(b["bl"])) * torch.sigmoid(F.linear(cc, c(b["wg"]), c(b["bg"]))) +
                F.linear(cc, c(b["wb"])) + F.linear(x, c(b["ws"]), c(b["bs"])))

    act = lambda t: F.leaky_relu(t, negative_slope=0.01)  # noqa: E731
    proj = 2 * math.pi * (z @ c(W["bmat"]))
    out = torch.cat([torch.sin(proj), torch.cos(proj), z], dim=1)
    bl = W["blocks"]
    skips = []
    for b in bl[0:3]:
        out = block(b, out)
        skips.append(out)
        out = act(out)
    out = block(bl[3], out)
    for b in bl[4:7]:
        out = block(b, act(torch.cat([out, skips.pop()], dim=1)))
    return z + out if residual else out


def sweep(W, zt0, xemb, temb_in, coef, noise, residual, dt):
    """The reverse sweep (diffusion_net.py:595-622) on the host tables: (eps (n, B, nz), zt (B, nz)) in dtype dt.
    eps = p(zt); pred = c0 (zt - eps c1); zt <- last ? pred : c2 zt + c3 pred (+ c4 xi_k)."""
    import torch

    zt = zt0.to(dt)
    cf = coef.to(dt)
    eps_log = []
    with torch.no_grad():
        for k in range(coef.shape[0]):
            eps = denoise(W, zt, temb_in[k], xemb, residual)
            eps_log.append(eps)
            pred = cf[k, 0] * (zt - eps * cf[k, 1])
            if float(coef[k, 5]) != 0.0:
                zt = pred
            else:
                zt = cf[k, 2] * zt + cf[k, 3] * pred
                if noise is not None:
                    zt = zt + cf[k, 4] * noise[k].to(dt)
    return torch.stack(eps_log).numpy(), zt.numpy()


def _refs(cid, coef, temb, noise, rows=None):
    import torch

    W, I = weights(cid), inputs(cid)
    sl = slice(None) if rows is None else rows
    nz = noise[:, sl].contiguous() if noise is not None else None
    out = []
    for dt in (torch.float32, torch.float64):
        eps, zt = sweep(W, I["zt0"][sl], I["xemb"][sl], temb, coef, nz, shape(cid)[5], dt)
        out.append(dict(eps=eps, zt=zt))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def refs(cid, n=N_STEPS):
    """(fp32, fp64) dicts {eps (n, B, nz), zt (B, nz)} of the default schedule at n steps with the injected noise."""
    coef, temb = tables(n, shape(cid)[2])
    return _refs(cid, coef, temb, inputs(cid, n)["noise"])


@functools.lru_cache(maxsize=None)
def single_step_refs(cid):
    coef, temb = single_step_tables(shape(cid)[2])
    return _refs(cid, coef, temb, None)


def unet_module(cid):
    """The case as the drop-in module's Diffusion_UnetA (w = 32 nf only), loaded with weights(cid)."""
    import torch

    from src import diffusion_net as dn

    nz, w, nt, nx, _, res = shape(cid)
    assert w % 32 == 0
    m = dn.Diffusion_UnetA(nz=nz, nxemb=nx, ntemb=nt, residual=bool(res), nf=w // 32)
    W = weights(cid)
    with torch.no_grad():
        m.B.copy_(W["bmat"])
        for lin, (wk, bk) in ((m.time_mlp[1], ("tw1", "tb1")), (m.time_mlp[3], ("tw2", "tb2"))):
            lin.weight.copy_(W[wk])
            lin.bias.copy_(W[bk])
        blocks = list(m.in_layers) + list(m.mid_layers) + list(m.out_layers)
        for blk, b in zip(blocks, W["blocks"]):
            for mod, wk, bk in ((blk._layer[0], "wl", "bl"), (blk._skip, "ws", "bs"), (blk._hyper_gate, "wg", "bg"),
                                (blk._hyper_bias, "wb", None), (blk._layer_ctx[1], "wctx", "bctx")):
                mod.weight.copy_(b[wk])
                if bk:
                    mod.bias.copy_(b[bk])
    return m.eval()


def step_logsnr(n, k):
    """logsnr_t of sweep step k (i = n - 1 - k) as step_tables evaluates it."""
    import torch

    from damc import amortizer

    it = torch.ones(1, dtype=torch.float32) * float(n - 1 - k)
    return amortizer._schedule(it / (n - 1.0), LOGSNR_MIN, LOGSNR_MAX)


SLICES = (("lastrow", (Ellipsis, -1, slice(None))), ("lastcol", (Ellipsis, -1)))   # eps[k] and zt: (B, nz)
