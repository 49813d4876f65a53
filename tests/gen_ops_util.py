"""Shared by tests/test_gen_ops_cases_cpu.py and tests/test_gpu_gen_ops.py: the case table of the G update's two
calls of include/damc.h (damc_generator_train_forward / damc_generator_train_backward), their fp32 / fp64 CPU
references (oracle.damc_oracle's explicit backward), the route arithmetic of csrc/generator.hip and csrc/wgrad.hip
restated in Python, and the launch counts each case must show.

Rule (the project's per-op rule, encoder_ops_util): per tensor |hip - fp64| <= 3 |fp32 CPU - fp64| + 1e-6 in rel-L2.  A
gradient's denominator is its fp64 norm floored at 1e-3 x the largest gradient norm of the call (train_ops_util.rule_rows);
x_hat is measured against its own norm.

A case is a stack [ConvT(nz, hidden[0], k0, 1, 0), LReLU(.2)] + [ConvT(a, b, 4, 2, 1), LReLU(.2)]* + ConvT(., nc, k, s, p),
Tanh in a holder module's `.gen`, or (G8) damc.toy.ToyG's `.net`.  Weights synth.load_into(seed); z = normal_f32(seed + 1,
0), x = uniform_f32(seed + 2, 0); grad_xhat = 2 (x_hat32 - x) / B with x_hat32 the fp32 CPU reference's, fed identically to
the library and, cast, to both references.  The seeds are the ones at which no fp64 pre-activation of an activated
layer lies within KINK_REL x its layer's RMS of zero (test_gen_ops_cases_cpu pins it).

  case  nz   k0  hidden         out (k, s, p)  nc  B     what it reaches (both engines unless said)
  G1    4    2   (8, 8)         (3, 1, 1)      1   1     nothing limb-capable; first layer on launch_small_gemm; Bp = 32
                                                         with 31 zero samples; up2_wgrad_reduce_any_kernel (Cout 8); R = 1
  G2    32   4   (64, 32, 32)   (3, 1, 1)      3   33    every layer limb-capable both ways; sign bits for every hidden
                                                         activation; the limbs-only gradient into h3 and the transposes
                                                         reading src3; Bp = 64 with 31 padded samples
  G3    100  4   (32, 16, 8)    (4, 2, 1)      3   20    nz % 32 != 0; 32 -> 16 forward on limbs, dgrad on fp32 MFMA;
                                                         16 -> 8 on neither; the k4 s2 output layer (SW(3, 4))
  G4    32   4   (256, 64)      (3, 1, 1)      3   4     256 -> 64 on a 4 x 4 grid, K = 1024 both ways: x3_ksplit splits
                                                         (4 sign blocks of 256); also under DAMC_X3_KSPLIT=0
  G5    100  7   (64, 32, 8)    (3, 1, 1)      1   5     7 x 7 grid (x3_tapshare_ok false); K0 = 3136: 11 of 12 slices run,
                                                         the zeroed tail of dz_slabs; hidden layer 1 without bias
  G6a   8    28  (8)            (3, 1, 1)      1   512   no activation after the first layer; smallc_rows = 8 with row
                                                         blocks 8, 8, 8, 4; the bias gradient over 401 408 rows at C = 1 on
                                                         the two-pass scalar column sum; K0 = 6272: 22 of 24 slices run
  G6b   8    32  (8)            (3, 1, 1)      3   256   no activation; smallc_rows = 4; C = 3 two-pass
  G6c   8    4   (8, 8)         (4, 2, 1)      4   3     SW(4, 4) and the Cout = 4 output-layer forward and dgrad
  G6d   8    4   (8, 8)         (3, 1, 1)      2   3     SW(2, 3)
  G7    8    4   (32, 16, 4)    (4, 2, 1)      3   4     last hidden Cout = 4: refused on the host (N % 8 of launch_wgrad_x3)
  G8    damc.toy.ToyG (2 -> 128 -> 128 -> 128 -> 2, ReLU)  37  linear_wgrad, linear_dgrad, linear_out with ACT_NONE

G6a / G6b carry no hidden activation: with 3.2 M pre-activations some always lie within KINK_REL of the kink, and a flip
moves the first layer's gradients by far more than the bound; the plan and the library take a ConvT without one.
"""
import functools

import numpy as np

from encoder_ops_util import (GUARD_WORD, KINK_REL, assert_guards_intact, check, distances, guarded,  # noqa: F401
                              is_pattern, report, reset_guards)
from train_ops_util import check_rows, rule_rows  # noqa: F401

ENGINE_LIMB, ENGINE_FP32 = 0, 1
ENGINES = (("limb", ENGINE_LIMB), ("fp32", ENGINE_FP32))
PROJ, UP2, SMALLC, LINEAR = 1, 2, 3, 4       # include/damc.h DAMC_LAYER_*
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2

# ------------------------------------------------------------------------------------------------ case table
CASES = {
    "G1": dict(nz=4, k0=2, hidden=(8, 8), out=(3, 1, 1), nc=1, B=1, seed=101),
    "G2": dict(nz=32, k0=4, hidden=(64, 32, 32), out=(3, 1, 1), nc=3, B=33, seed=102),
    "G3": dict(nz=100, k0=4, hidden=(32, 16, 8), out=(4, 2, 1), nc=3, B=20, seed=103),
    "G4": dict(nz=32, k0=4, hidden=(256, 64), out=(3, 1, 1), nc=3, B=4, seed=104),
    "G5": dict(nz=100, k0=7, hidden=(64, 32, 8), out=(3, 1, 1), nc=1, B=5, seed=105, nobias=(1,)),
    "G6a": dict(nz=8, k0=28, hidden=(8,), out=(3, 1, 1), nc=1, B=512, seed=106, act0=False),
    "G6b": dict(nz=8, k0=32, hidden=(8,), out=(3, 1, 1), nc=3, B=256, seed=107, act0=False),
    "G6c": dict(nz=8, k0=4, hidden=(8, 8), out=(4, 2, 1), nc=4, B=3, seed=108),
    "G6d": dict(nz=8, k0=4, hidden=(8, 8), out=(3, 1, 1), nc=2, B=3, seed=109),
    "G7": dict(nz=8, k0=4, hidden=(32, 16, 4), out=(4, 2, 1), nc=3, B=4, seed=110),
    "G8": dict(linear=True, nz=2, B=37, seed=111),
}
RUN_IDS = [c for c in CASES if c != "G7"]   # G7 is the contract case: refused by the library
CONTRACT_ID = "G7"
SLOPE = 0.2

# what the table above claims, pinned by test_gen_ops_cases_cpu from the mirrored arithmetic below
BP = {"G1": 32, "G2": 64, "G3": 32, "G4": 32, "G5": 32, "G6a": 512, "G6b": 256, "G6c": 32, "G6d": 32,
      "G7": 32, "G8": 64}
SMALLC_ROWS = {"G1": 1, "G2": 1, "G3": 1, "G4": 1, "G5": 1, "G6a": 8, "G6b": 4, "G6c": 1, "G6d": 1}
DZ_SLICES = {"G5": (12, 288, 11), "G6a": (24, 288, 22), "G6b": (32, 256, 32), "G2": (4, 256, 4)}  # (carved, k_per, run)
# per UP2 layer (forward limb-capable, input gradient limb-capable)
X3_CAPS = {"G2": [(True, True), (True, True)], "G3": [(True, False), (False, False)],
           "G1": [(False, False)], "G5": [(True, True), (True, False)], "G4": [(True, True)]}
X3_PROJ = {"G1": False, "G2": True, "G3": False, "G4": True, "G5": False, "G6a": False}
HBITS = {"G2": [True, True, True], "G3": [False, False, False], "G5": [False, False, True], "G1": [False, False]}
# output-layer bias gradient: (rows, C, passes)
OUT_COLSUM = {"G1": (16, 1, 1), "G2": (33 * 256, 3, 2), "G3": (20 * 1024, 3, 2), "G5": (5 * 784, 1, 1),
              "G6a": (401408, 1, 2), "G6b": (262144, 3, 2), "G6c": (768, 4, 1), "G6d": (192, 2, 1), "G8": (37, 2, 1)}


# ------------------------------------------------------------------------------------------------ building a case
def build_module(cid):
    """The case's holder module (CPU, fp32, synth weights): `.gen` an nn.Sequential, or ToyG with its `.net`."""
    import torch
    import torch.nn as nn

    from damc import synth, toy

    c = CASES[cid]
    if c.get("linear"):
        return synth.load_into(toy.ToyG(nz=c["nz"]), c["seed"])
    nobias = c.get("nobias", ())
    hidden = c["hidden"]
    mods = [nn.ConvTranspose2d(c["nz"], hidden[0], c["k0"], 1, 0, bias=0 not in nobias)]
    if c.get("act0", True):
        mods.append(nn.LeakyReLU(SLOPE))
    for i, (a, b) in enumerate(zip(hidden[:-1], hidden[1:])):
        mods += [nn.ConvTranspose2d(a, b, 4, 2, 1, bias=(i + 1) not in nobias), nn.LeakyReLU(SLOPE)]
    k, s, p = c["out"]
    mods += [nn.ConvTranspose2d(hidden[-1], c["nc"], k, s, p), nn.Tanh()]

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            self.gen = nn.Sequential(*mods)

    return synth.load_into(Holder(), c["seed"])


@functools.lru_cache(maxsize=None)
def case(cid):
    """dict(G, z, x, grad_xhat, names, ref32, ref64, pre64): CPU tensors and the two references as dicts of numpy arrays
    (x_hat, w<i>, b<i> for every layer with a bias, grad_z), computed once and shared."""
    import torch

    from damc import synth
    from oracle import damc_oracle as orc

    c = CASES[cid]
    G = build_module(cid)
    B = c["B"]
    z = torch.from_numpy(synth.normal_f32(c["seed"] + 1, 0, (B, c["nz"])))
    L32 = orc.generator_layers(G, torch.float32)
    L64 = orc.generator_layers(G, torch.float64)
    with torch.no_grad():
        xh32 = orc.generator_sample(L32, z)
        x = torch.from_numpy(synth.uniform_f32(c["seed"] + 2, 0, tuple(xh32.shape)))
        gx = (2.0 * (xh32 - x) / B).contiguous()
        refs = []
        for L, dt in ((L32, torch.float32), (L64, torch.float64)):
            grads, gz, xh = orc.generator_train_grads(L, z.to(dt), gx.to(dt))
            d = dict(x_hat=xh.numpy(), grad_z=gz.numpy())
            for i, (gw, gb) in enumerate(grads):
                d["w%d" % i] = gw.numpy()
                if gb is not None:
                    d["b%d" % i] = gb.numpy()
            refs.append(d)
        pre64 = _pre_activations(L64, z.double())
    names = ["x_hat"]
    for i, L in enumerate(L32):
        names.append("w%d" % i)
        if L["b"] is not None:
            names.append("b%d" % i)
    names.append("grad_z")
    return dict(G=G, z=z, x=x, grad_xhat=gx, names=names, ref32=refs[0], ref64=refs[1], pre64=pre64)


def _pre_activations(layers, z):
    """The pre-activations of every LeakyReLU / ReLU layer (oracle.generator_forward's loop, keeping them)."""
    import torch.nn.functional as F

    from oracle import damc_oracle as orc

    h, pre = z, []
    for i, L in enumerate(layers):
        if L["kind"] == "convT":
            if i == 0:
                h = h.reshape(len(h), -1, 1, 1)
            a = F.conv_transpose2d(h, L["W"], L["b"], stride=L["stride"], padding=L["pad"])
        else:
            a = F.linear(h, L["W"], L["b"])
        if L["act"][0] == "lrelu":
            pre.append(a.numpy())
        h = orc._apply_act(a, L["act"])
    return pre


def kink_margin(cid):
    """min |pre-activation| / rms of its layer over the activated hidden layers, fp64 (inf: no such layer)."""
    pre = case(cid)["pre64"]
    return min([float(np.abs(a).min() / np.sqrt(np.mean(a * a))) for a in pre] or [float("inf")])


FWD = ("x_hat",)


def slices_of(name, arr):
    """The slices a tail bug would hit (encoder_ops_util.CONV_SLICES' idea): the last channel and the last pixel row
    of x_hat (NCHW), the last output and input channel of a ConvT weight gradient (Cin, Cout, k, k), the last row and
    column of a matrix."""
    if arr.ndim == 4 and name == "x_hat":
        return (("lastchan", (slice(None), -1)), ("lastpixrow", (-1, slice(None), -1)))
    if arr.ndim == 4:
        return (("lastcout", (slice(None), -1)), ("lastcin", (-1,)))
    if arr.ndim == 2:
        return (("lastrow", (-1,)), ("lastcol", (Ellipsis, -1)))
    return ()


# ------------------------------------------------------------------------------------------------ layer specs
@functools.lru_cache(maxsize=None)
def layer_specs(cid):
    """damc.plans.GeneratorPlan's layer dicts (kind, cin, cout, k, stride, pad, hin, hout, act, slope) plus `bias`."""
    from damc import plans

    G = build_module(cid) if cid == CONTRACT_ID else case(cid)["G"]
    plan = plans.GeneratorPlan(G)
    out = []
    for spec, m in zip(plan.layers, plan.modules):
        d = dict(spec)
        d["bias"] = m.bias is not None
        out.append(d)
    return out


def host_descriptor(cid, engine=ENGINE_LIMB, fake=1 << 20):
    """A damc_generator_t of the case with made-up addresses: for calls that return before any launch."""
    from damc import _lib

    specs = layer_specs(cid)
    g = _lib.Generator()
    g.n_layers, g.nz = len(specs), specs[0]["cin"]
    g.nc, g.h, g.w = specs[-1]["cout"], specs[-1]["hout"], specs[-1]["hout"]
    for i, s in enumerate(specs):
        d = g.layers[i]
        d.kind, d.cin, d.cout, d.k, d.stride, d.pad = s["kind"], s["cin"], s["cout"], s["k"], s["stride"], s["pad"]
        d.hin = d.win = s["hin"]
        d.hout = d.wout = s["hout"]
        d.act, d.slope, d.engine = s["act"], s["slope"], engine
        d.w_fwd, d.w_bwd = fake + 65536 * (2 * i), fake + 65536 * (2 * i + 1)
        d.bias = fake + 65536 * 64 + 4096 * i if s["bias"] else None
    return g


# ------------------------------------------------------------------------------------------------ route arithmetic
def bp_of(B):
    """csrc/generator.hip bp_of: the batch padded to whole 32-sample K tiles."""
    return (B + 31) // 32 * 32


def smallc_rows(L, B):
    """csrc/wgrad.hip smallc_rows: input rows per block of the output layer's weight gradient."""
    R = 8
    Wd = L["stride"] * (L["hin"] - 1) + L["k"]
    while R > 1 and ((L["stride"] * (R - 1) + L["k"]) * Wd * L["cout"] * 4 > 40960 or
                     B * ((L["hin"] + R - 1) // R) < 2048):
        R //= 2
    return R


def smallc_row_blocks(L, B):
    """The rows each block of launch_smallc_wgrad's grid.x covers (smallc_wgrad_kernel's `rows`)."""
    R = smallc_rows(L, B)
    return [min(R, L["hin"] - r0) for r0 in range(0, L["hin"], R)]


def up2_wgrad_split(L, Bp):
    """csrc/generator.hip up2_wgrad_split: (slices, slice length) of a k4 s2 p1 weight gradient."""
    M, N, K = 4 * L["cin"], L["cout"], L["hin"] * L["hin"] * Bp
    base = ((M + 255) // 256) * ((N + 127) // 128) * 4
    nkt = K // 32
    sl = max(1, min(min((512 + base - 1) // base, 16), nkt))
    kp = (nkt + sl - 1) // sl * 32
    return (K + kp - 1) // kp, kp


def proj_slices(K):
    """csrc/generator.hip proj_slices: split-K slices carved for the first layer's input gradient."""
    return max(1, min(512, K // 256))


def proj_k_per(K, S):
    """csrc/generator.hip proj_k_per: slice length, a multiple of 32."""
    return ((K + S - 1) // S + 31) // 32 * 32


def dz_split(specs):
    """(slices carved, slice length, slices dz_slabs runs): fewer run than carved = the zeroed slab tail."""
    L0 = specs[0]
    K = L0["hout"] * L0["hout"] * L0["cout"]
    S = 1 if len(specs) == 1 else proj_slices(K)
    kp = proj_k_per(K, S)
    return S, kp, (K + kp - 1) // kp


def colsum_lanes(C):
    """csrc/wgrad.hip colsum_lanes."""
    cl = 1
    while cl < C and cl < 64:
        cl <<= 1
    return cl


def colsum_blocks(R, C):
    """csrc/wgrad.hip colsum_blocks: row blocks of the scalar column sum's first pass (1: a single pass)."""
    per = 16 * (256 // colsum_lanes(C))
    return 1 if R <= 8 * per else min(1024, (R + per - 1) // per)


def colsum4_lanes(C4):
    """csrc/wgrad.hip colsum4_lanes."""
    cl = 1
    while cl < C4 and cl < 16:
        cl <<= 1
    return cl


def colsum4_blocks(R, C):
    """csrc/wgrad.hip colsum4_blocks: the float4 form's row blocks."""
    rl = 256 // colsum4_lanes(C // 4)
    return 1 if R <= 32 * rl else min(256, (R + 32 * rl - 1) // (32 * rl))


def colsum_passes(R, C):
    """launch_colsum's passes for 16-B aligned operands with ld = C: the float4 kernel when C % 4 == 0."""
    return 1 if (colsum4_blocks(R, C) if C % 4 == 0 else colsum_blocks(R, C)) == 1 else 2


def x3_fwd_cap(L):
    """csrc/generator.hip x3_fwd_cap."""
    return L["kind"] == UP2 and L["cin"] % 32 == 0 and L["cout"] % 8 == 0


def x3_bwd_cap(L):
    """csrc/generator.hip x3_bwd_cap."""
    return L["kind"] == UP2 and L["cout"] % 32 == 0 and L["cin"] % 8 == 0


def x3_proj_cap(L):
    """csrc/generator.hip x3_proj_cap."""
    return L["kind"] == PROJ and L["cin"] % 32 == 0 and L["cout"] % 8 == 0


def _known_taps(L):
    """csrc/smallc.hip known_taps."""
    return L["cout"] in (1, 3) and ((L["k"] == 3 and L["stride"] == 1) or (L["k"] == 4 and L["stride"] == 2))


def _smallc_reg_ok(L):
    """csrc/smallc.hip smallc_reg_ok."""
    if not _known_taps(L):
        return False
    ch = 4 if L["k"] == 3 else 2
    if L["cin"] % ch:
        return False
    g = L["cin"] // ch
    return g <= 64 and 64 % g == 0


def _smallc_x3_ok(L):
    """csrc/smallc.hip smallc_x3_ok."""
    return _smallc_reg_ok(L) and L["cin"] % 8 == 0


def smallc_dgrad_reads_bits(L):
    """csrc/smallc.hip smallc_dgrad_reads_bits = smallc_k3 || smallc_s2_mfma."""
    if L["kind"] != SMALLC:
        return False
    k3 = L["k"] == 3 and L["pad"] == 1 and L["hout"] == L["hin"] and _smallc_x3_ok(L)
    s2 = (_known_taps(L) and L["k"] == 4 and L["pad"] == 1 and L["hout"] == 2 * L["hin"] and
          L["cin"] in (64, 128, 256))
    return k3 or s2


def hbits_cap(specs, j):
    """csrc/generator.hip hbits_cap: activation j travels as sign bits on the limb engine."""
    if j + 1 >= len(specs):
        return False
    L, N = specs[j], specs[j + 1]
    prod = x3_proj_cap(L) if j == 0 else x3_fwd_cap(L)
    return prod and L["act"] == ACT_LRELU and (x3_bwd_cap(N) or smallc_dgrad_reads_bits(N))


def x3_conv_negk(m_per_sample, N, K, zdim):
    """csrc/gemm.h x3_conv_negk (no DAMC_X3_NEGK_RULE): k per sign block of a limb-engine conv weight."""
    w16 = ((16 * m_per_sample + 255) // 256) * ((N + 127) // 128) * zdim * K
    nk = 1024 if w16 >= 1 << 18 else 512 if w16 >= 1 << 16 else 256
    while nk > 256 and K % nk:
        nk >>= 1
    return nk


def x3_ksplit(M, N, K, zdim, negk, bm=256, bn=128):
    """csrc/gemm_x3.hip x3_ksplit with its defaults: the sign blocks an under-filled limb-engine conv splits into."""
    wgs = ((M + bm - 1) // bm) * ((N + bn - 1) // bn) * zdim
    if K % negk or K // negk < 2:
        return 1
    ks = K // negk
    return ks if (wgs < 128 or (wgs < 256 and ks <= 16)) else 1


def up2_ksplits(L, B):
    """(forward, input gradient) x3_ksplit of a k4 s2 p1 layer at batch B (generator.hip up2_negk_fwd / _bwd)."""
    P = L["hin"] * L["hin"]
    nf = x3_conv_negk(P, L["cout"], 4 * L["cin"], 4)
    nb = x3_conv_negk(P, L["cin"], 16 * L["cout"], 1)
    return (x3_ksplit(B * P, L["cout"], 4 * L["cin"], 4, nf), x3_ksplit(B * P, L["cin"], 16 * L["cout"], 1, nb))


def x3_tapshare_ok(hq, wq):
    """csrc/gemm.h x3_tapshare_ok."""
    hw = hq * wq
    if hq <= 0 or wq <= 0 or 256 % hw:
        return False
    return 64 % hw == 0 or (hw % 64 == 0 and 64 % wq == 0)


def train_supported(specs, B):
    """csrc/generator.hip train_supported: what the G update refuses on the host (sizes beyond 2^31 B left out: no
    case comes near)."""
    for L in specs:
        if L["kind"] == UP2 and L["cout"] % 8:
            return False
        if L["kind"] == PROJ and (L["cout"] * L["hout"] * L["hout"]) % 8:
            return False
        if L["kind"] == SMALLC and not (1 <= L["cout"] <= 4 and L["k"] in (3, 4)):
            return False
    return True


# ------------------------------------------------------------------------------------------------ launch counts
PROF_NAMES = ("proj_fwd", "small_gemm", "upconv_fwd", "split_x3", "smallc_fwd", "linear_out", "out_delta",
              "smallc_wgrad", "wgrad_transpose", "wgrad_up2", "wgrad_proj", "wgrad_reduce", "bias_grad", "upconv_dgrad",
              "smallc_dgrad", "proj_dgrad", "slab_sum", "linear_wgrad", "linear_dgrad")


def expected_counts(cid, engine, want_gz=True, skip_w=(), skip_b=()):
    """Profiler scopes one forward + backward of the case opens, by name, from the predicates above: forward_hidden,
    forward_final, train_backward and dgrad_layer of csrc/generator.hip walked without launching.  A launch_colsum call
    is ONE bias_grad scope whether it takes one pass or two; launch_smallc_wgrad opens one for its own reduction."""
    specs = layer_specs(cid)
    n = len(specs)
    limb = engine == ENGINE_LIMB
    fcap = [limb and x3_fwd_cap(L) for L in specs]
    bcap = [limb and x3_bwd_cap(L) for L in specs]
    pcap = limb and x3_proj_cap(specs[0])
    c = dict.fromkeys(PROF_NAMES, 0)
    for i in range(n - 1):
        L = specs[i]
        wrote = False
        if i == 0 and pcap:
            c["split_x3"] += 1
            c["proj_fwd"] += 1
            wrote = fcap[1]
        elif L["kind"] == PROJ and L["cin"] % 32 == 0:
            c["proj_fwd"] += 1
        elif L["kind"] == PROJ:
            c["proj_fwd"] += 1
            if L["cin"] % 4 == 0:
                c["small_gemm"] += 1
            else:
                c["proj_fwd"] += 1
        elif L["kind"] == LINEAR:
            c["proj_fwd"] += 1
        else:
            c["upconv_fwd"] += 1
            wrote = fcap[i] and fcap[i + 1]
        if fcap[i + 1] and not wrote:
            c["split_x3"] += 1
    c["smallc_fwd" if specs[-1]["kind"] == SMALLC else "linear_out"] += 1
    c["out_delta"] += 1
    for i in range(n - 1, -1, -1):
        L = specs[i]
        dw, db = i not in skip_w, L["bias"] and i not in skip_b
        if L["kind"] == SMALLC:
            if dw:
                c["smallc_wgrad"] += 1
                c["bias_grad"] += 1
        elif L["kind"] == LINEAR:
            if dw:
                c["linear_wgrad"] += 1
        else:
            c["wgrad_transpose"] += 2 if dw else 1
            if dw:
                c["wgrad_up2" if L["kind"] == UP2 else "wgrad_proj"] += 1
                c["wgrad_reduce"] += 1 if L["kind"] == UP2 else 0
        if db:
            c["bias_grad"] += 1
        if i >= 1:
            x3_out = False
            if L["kind"] == SMALLC:
                c["smallc_dgrad"] += 1
                x3_out = bcap[i - 1] and _smallc_x3_ok(L)   # smallc_grad_form: limbs where the dgrad below reads them
            elif L["kind"] == UP2:
                c["upconv_dgrad"] += 1
                x3_out = bcap[i] and bcap[i - 1]
            else:
                c["linear_dgrad"] += 1
            if bcap[i - 1] and not x3_out:
                c["split_x3"] += 1
        elif want_gz:
            c["proj_dgrad"] += 1
            c["slab_sum"] += 1
    return c
