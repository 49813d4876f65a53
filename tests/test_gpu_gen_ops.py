"""GPU: the G update's two calls, damc_generator_train_forward / damc_generator_train_backward, called directly through
ctypes at the smallest shapes that reach each route of csrc/generator.hip train_backward, csrc/wgrad.hip and the output
layer's weight and input gradients (tests/gen_ops_util.py holds the table and says what each case reaches), on both
engines.

Rule: per tensor |hip - fp64| <= 3 |fp32 CPU - fp64| + 1e-6 in rel-L2, gradients floored at 1e-3 x the call's largest
gradient norm (train_ops_util.rule_rows), and the same for the last-channel / last-row slices (encoder_ops_util.report's
slice floor); no tensor and no case is left out.  x_hat, every dW and db and grad_z sit in guarded buffers that start out
as one NaN bit pattern (encoder_ops_util.guarded): the calls WRITE them, a skipped one keeps the pattern, and as the
workspace starts out as that pattern too, a read of a region nothing wrote shows as a non-finite output.  The guards are
compared after every library call.  Run with -s for the per-tensor distances (profiles/r20/gen_ops_parity.txt is one
such run).
"""
import ctypes
import functools

import pytest
import torch

import gen_ops_util as U
from gen_ops_util import assert_guards_intact, guarded, is_pattern

pytestmark = pytest.mark.gpu

ENGINE_IDS = [n for n, _ in U.ENGINES]
ENGINE_OF = dict(U.ENGINES)


@pytest.fixture(autouse=True)
def _fresh_guards():
    U.reset_guards()
    yield
    U.reset_guards()
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:  # a device fault is sticky: nothing more is started on this device
            pytest.exit("device error after a test of this file: %s" % e, returncode=3)


def _api(dev):
    from damc import _lib

    return _lib, _lib.lib(), _lib.stream_ptr(dev)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _module(cid, dev):
    """The case's net on the device (its weights are read-only for every test)."""
    import copy

    G = U.build_module(cid) if cid == U.CONTRACT_ID else U.case(cid)["G"]
    return copy.deepcopy(G).to(dev)


def _prepare(dev, cid, engine, want_gz=True, skip_w=(), skip_b=()):
    """The case's buffers and its two calls: (out, forward(stream) -> rc, backward(stream) -> rc).  Every output is
    allocated and guarded whether requested or not; the workspace starts out as the NaN pattern.  The weights are packed
    here, before anything is recorded or timed."""
    from damc import plans

    _lib, L, _ = _api(dev)
    ptr = _lib.ptr
    c = U.case(cid)
    G = _module(cid, dev)
    plan = plans.generator_plan(G)
    desc = plan.refresh(dev, engine=engine)
    torch.cuda.synchronize()
    B = U.CASES[cid]["B"]
    z, gx = c["z"].to(dev).contiguous(), c["grad_xhat"].to(dev).contiguous()
    nb = int(L.damc_generator_train_workspace_bytes(ctypes.byref(desc), B))
    assert nb > 0
    ws = guarded(nb, dev)
    out = dict(x_hat=guarded(tuple(c["ref64"]["x_hat"].shape), dev), grad_z=guarded(tuple(z.shape), dev))
    grads = _lib.GeneratorGrads()
    for i, m in enumerate(plan.modules):
        out["w%d" % i] = guarded(tuple(m.weight.shape), dev)
        if i not in skip_w:
            grads.w[i] = out["w%d" % i].data_ptr()
        if m.bias is not None:
            out["b%d" % i] = guarded(tuple(m.bias.shape), dev)
            if i not in skip_b:
                grads.b[i] = out["b%d" % i].data_ptr()
    assert set(out) == set(c["names"])
    keep = (desc, z, gx, ws, grads, plan)

    def forward(stream):
        return L.damc_generator_train_forward(ctypes.byref(desc), ptr(z), B, ptr(out["x_hat"]), ptr(ws), nb, stream)

    def backward(stream, d=desc, batch=B):
        return L.damc_generator_train_backward(ctypes.byref(d), ptr(z), ptr(out["x_hat"]), ptr(gx), batch,
                                               ctypes.byref(grads), ptr(out["grad_z"]) if want_gz else None, ptr(ws),
                                               nb, stream)

    forward.keep = keep
    return out, forward, backward


def _run(dev, cid, engine, **kw):
    """One forward and one backward of the case, the guards compared after each; returns copies of every output."""
    _, _, stream = _api(dev)
    out, forward, backward = _prepare(dev, cid, engine, **kw)
    rc = forward(stream)
    assert rc == 0, rc
    assert_guards_intact()
    rc = backward(stream)
    assert rc == 0, rc
    assert_guards_intact()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}


def _check(label, cid, res):
    """The rule for every tensor of the call, then for the slices a tail bug would hit; prints every pair of distances
    and the share of the bound used."""
    c = U.case(cid)
    got = {n: res[n].cpu().numpy() for n in c["names"]}
    rows = U.rule_rows(c["names"], got, c["ref32"], c["ref64"], U.FWD)
    worst = 0.0
    for n, e, e32 in rows:
        share = e / (3.0 * e32 + 1e-6)
        worst = max(worst, share)
        print("PARITY %-14s %-7s all        hip-fp64 %.3e  fp32-fp64 %.3e  share %.3f" % (label, n, e, e32, share))
    bad = [r for r in rows if not r[1] <= 3.0 * r[2] + 1e-6]
    for n in c["names"]:
        for sl, e, e32 in U.distances(got[n], c["ref32"][n], c["ref64"][n], U.slices_of(n, got[n]))[1:]:
            share = e / (3.0 * e32 + 1e-6)
            worst = max(worst, share)
            print("PARITY %-14s %-7s %-10s hip-fp64 %.3e  fp32-fp64 %.3e  share %.3f" % (label, n, sl, e, e32, share))
            if not e <= 3.0 * e32 + 1e-6:
                bad.append((n, sl, e, e32))
    print("PARITY %-14s largest share of the bound %.3f" % (label, worst))
    assert not bad, (label, bad)


# ------------------------------------------------------------------------------------------------ parity
_RUNS = ([(cid, eng, "default") for cid in U.RUN_IDS for eng in ENGINE_IDS] +
         [("G4", eng, "ksplit0") for eng in ENGINE_IDS])
_ENVS = {"default": {}, "ksplit0": {"DAMC_X3_KSPLIT": "0"}}


@pytest.mark.parametrize("cid,eng,env", _RUNS, ids=["%s-%s-%s" % r for r in _RUNS])
def test_generator_train_matches_fp64(gpu_device, monkeypatch, cid, eng, env):
    for k, v in _ENVS[env].items():
        monkeypatch.setenv(k, v)
    res = _run(gpu_device, cid, ENGINE_OF[eng])
    for n, t in res.items():
        assert torch.isfinite(t).all(), (cid, eng, n, "non-finite: a pattern word left, or unwritten workspace read")
    _check("%s %s%s" % (cid, eng, "" if env == "default" else " " + env), cid, res)


# ------------------------------------------------------------------------------------------------ routes
def _prof_counts(dev, fn):
    """Launch counts per profiler scope (damc_prof_query) during fn(): test_gpu_train_ops._prof_counts for PROF_NAMES."""
    _, L, _ = _api(dev)
    L.damc_prof_select(None)
    L.damc_prof_reset()
    L.damc_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for name in U.PROF_NAMES:
            ms, n, fl = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
            rc = L.damc_prof_query(name.encode(), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
            out[name] = int(n.value) if rc == 0 else 0
    finally:
        L.damc_prof_enable(0)
        L.damc_prof_reset()
    return out


@pytest.mark.parametrize("eng", ENGINE_IDS)
@pytest.mark.parametrize("cid", U.RUN_IDS)
def test_cases_take_the_routes_the_table_names(gpu_device, cid, eng):
    """Every profiler scope of one forward + backward, against the count the mirrored predicates give
    (gen_ops_util.expected_counts): split_x3 absent where an epilogue or a limbs-only dgrad wrote the limbs, small_gemm
    for a first layer off both GEMM engines, the linear_* scopes for the MLP, one bias_grad per column sum."""
    engine = ENGINE_OF[eng]
    out, forward, backward = _prepare(gpu_device, cid, engine)
    _, _, stream = _api(gpu_device)
    got = _prof_counts(gpu_device, lambda: (forward(stream), backward(stream)))
    want = U.expected_counts(cid, engine)
    print("ROUTES %s %s %s" % (cid, eng, {k: v for k, v in got.items() if v}))
    assert got == want, (cid, eng, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
    assert_guards_intact()


def test_g4_without_ksplit_is_the_same_route_by_name(gpu_device, monkeypatch):
    """DAMC_X3_KSPLIT=0 changes how the 256 -> 64 layer's two GEMMs run, not which scopes open."""
    monkeypatch.setenv("DAMC_X3_KSPLIT", "0")
    out, forward, backward = _prepare(gpu_device, "G4", U.ENGINE_LIMB)
    _, _, stream = _api(gpu_device)
    got = _prof_counts(gpu_device, lambda: (forward(stream), backward(stream)))
    assert got == U.expected_counts("G4", U.ENGINE_LIMB)


# ------------------------------------------------------------------------------------------------ NULL entries
@pytest.mark.parametrize("eng", ENGINE_IDS)
def test_null_entries_are_skipped(gpu_device, eng):
    """G2 with grads->w[1] = b[1] = NULL (a hidden k4 s2 p1 layer), and with grad_z = NULL: what is not requested keeps
    the guard pattern, everything else is bitwise the full call's."""
    engine = ENGINE_OF[eng]
    full = _run(gpu_device, "G2", engine)
    for label, kw, skipped in (("w1 b1 NULL", dict(skip_w=(1,), skip_b=(1,)), {"w1", "b1"}),
                               ("grad_z NULL", dict(want_gz=False), {"grad_z"}),
                               ("w3 NULL", dict(skip_w=(3,)), {"w3"})):
        res = _run(gpu_device, "G2", engine, **kw)
        for n in res:
            if n in skipped:
                assert is_pattern(res[n]), (label, n, "was written")
            else:
                assert _same_bits(res[n], full[n]), (label, n)


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("eng", ENGINE_IDS)
@pytest.mark.parametrize("cid", ["G2", "G5", "G6a"])
def test_generator_train_is_repeatable(gpu_device, cid, eng):
    """No atomics anywhere: two runs agree bit for bit in every output."""
    a, b = _run(gpu_device, cid, ENGINE_OF[eng]), _run(gpu_device, cid, ENGINE_OF[eng])
    for n in a:
        assert _same_bits(a[n], b[n]), (cid, eng, n)


# ------------------------------------------------------------------------------------------------ graph replay
@pytest.mark.parametrize("eng", ENGINE_IDS)
@pytest.mark.parametrize("cid", ["G5", "G6a"])
def test_generator_train_replays_from_a_captured_graph(gpu_device, cid, eng):
    """Forward and backward recorded into one graph on a workspace that holds the NaN pattern, replayed twice from
    re-patterned outputs: every output is bitwise the eager call's.  Both cases run fewer first-layer input-gradient
    slices than the workspace carves (11 of 12, 22 of 24), so slab_sum adds a tail that only dz_slabs' zero fill wrote:
    leftover pattern words there would show as NaN in grad_z.  That fill used to be a hipMemsetAsync over all the slabs,
    the one kind of node DESIGN.md section 2 records a replay as not ordering before the kernels behind it: inside a
    whole-suite run G5's second replay then gave a finite grad_z that was not the eager one (on both engines), as a
    memset landing after the GEMM's stores would.  zero_floats_kernel writes the tail now.  Like its denoiser
    counterpart, this test passes with the memset form too whenever the memset happens to run first."""
    _lib, _, _ = _api(gpu_device)
    engine = ENGINE_OF[eng]
    S, _, run = U.dz_split(U.layer_specs(cid))
    assert run < S
    eager = _run(gpu_device, cid, engine)
    out, forward, backward = _prepare(gpu_device, cid, engine)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = _lib.stream_ptr(gpu_device)
        rcs = (forward(stream), backward(stream))
    assert rcs == (0, 0), rcs
    assert all(is_pattern(t) for t in out.values())  # recorded, not run
    for rep in range(2):
        for t in out.values():
            t.view(torch.int32).fill_(U.GUARD_WORD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_guards_intact()
        for n in out:
            assert torch.isfinite(out[n]).all(), (cid, eng, rep, n, "non-finite after a replay")
            assert _same_bits(out[n], eager[n]), (cid, eng, rep, n)


# ------------------------------------------------------------------------------------------------ the train record
def test_backward_must_match_its_forward(gpu_device):
    """include/damc.h: train_forward records (workspace, batch, engine); a backward whose engine or batch disagrees,
    and a second backward of one forward, return DAMC_ERR_ARG before any launch (every gradient keeps the pattern)."""
    _lib, _, stream = _api(gpu_device)
    from damc import plans

    cid = "G6d"
    out, forward, backward = _prepare(gpu_device, cid, U.ENGINE_LIMB)
    other = plans.generator_plan(_module(cid, gpu_device)).refresh(gpu_device, engine=U.ENGINE_FP32)
    grads = [n for n in out if n != "x_hat"]
    assert forward(stream) == 0
    assert backward(stream, d=other) == _lib.DAMC_ERR_ARG     # the other engine
    assert backward(stream, batch=U.CASES[cid]["B"] - 1) == _lib.DAMC_ERR_ARG   # another batch
    torch.cuda.synchronize()
    assert all(is_pattern(out[n]) for n in grads)
    assert backward(stream) == 0                              # the refusals left the record in place
    assert backward(stream) == _lib.DAMC_ERR_ARG             # consumed
    assert_guards_intact()
    res = {k: v.detach().clone() for k, v in out.items()}
    _check("%s limb record" % cid, cid, res)


# ------------------------------------------------------------------------------------------------ contracts
def _dropin(cid, dev):
    """The case's stack behind the drop-in generator's own forward (src.diffusion_net._GeneratorBase.forward)."""
    import copy

    from src import diffusion_net as dn

    gen = copy.deepcopy(U.build_module(cid).gen)

    class Stack(dn._GeneratorBase):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.nz = U.CASES[cid]["nz"]
            self._spc = False
            self.gen = gen

    return Stack().to(dev).train()


@pytest.mark.parametrize("eng", ENGINE_IDS)
def test_contract_case_is_refused_before_any_launch(gpu_device, eng):
    """G7 (last hidden Cout = 4): the workspace query is 0 and train_forward returns DAMC_ERR_UNSUPPORTED with x_hat
    untouched; the plain forward still runs and meets the rule."""
    from damc import plans

    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    cid = U.CONTRACT_ID
    B, nz = U.CASES[cid]["B"], U.CASES[cid]["nz"]
    G = _module(cid, gpu_device)
    desc = plans.generator_plan(G).refresh(gpu_device, engine=ENGINE_OF[eng])
    assert L.damc_generator_train_workspace_bytes(ctypes.byref(desc), B) == 0
    from damc import synth

    z = torch.from_numpy(synth.normal_f32(U.CASES[cid]["seed"] + 1, 0, (B, nz))).to(gpu_device)
    xh = guarded((B, 3, 32, 32), gpu_device)
    ws = guarded(1 << 24, gpu_device)
    assert L.damc_generator_train_forward(ctypes.byref(desc), ptr(z), B, ptr(xh), ptr(ws), 1 << 24,
                                          stream) == _lib.DAMC_ERR_UNSUPPORTED
    assert_guards_intact()
    assert is_pattern(xh) and is_pattern(ws.view(torch.float32))
    nb = int(L.damc_posterior_workspace_bytes(ctypes.byref(desc), B))
    assert 0 < nb <= 1 << 24
    assert L.damc_generator_forward(ctypes.byref(desc), ptr(z), B, ptr(xh), ptr(ws), nb, stream) == 0
    assert_guards_intact()
    from oracle import damc_oracle as orc

    x32 = orc.generator_sample(orc.generator_layers(G, torch.float32), z.cpu())
    x64 = orc.generator_sample(orc.generator_layers(G, torch.float64), z.cpu().double())
    U.check("G7 %s plain forward" % eng, xh.detach().cpu().numpy(), x32.numpy(), x64.numpy())


def test_contract_case_trains_on_the_stock_layers(gpu_device):
    """damc.training.generator_apply returns None for G7 under autograd, so the drop-in's forward runs the stock layers:
    G(z).backward() gives every gradient within the rule of the fp64 reference (it used to raise DamcError from the
    backward).  Without grad it stays on the library."""
    from damc import synth, training
    from oracle import damc_oracle as orc

    cid = U.CONTRACT_ID
    c = U.CASES[cid]
    G = _dropin(cid, gpu_device)
    z = torch.from_numpy(synth.normal_f32(c["seed"] + 1, 0, (c["B"], c["nz"])))
    zd = z.to(gpu_device).requires_grad_(True)
    assert training.generator_apply(G, zd) is None
    with torch.no_grad():
        assert training.generator_apply(G, zd) is not None
    L32, L64 = orc.generator_layers(G, torch.float32), orc.generator_layers(G, torch.float64)
    with torch.no_grad():
        xh32 = orc.generator_sample(L32, z)
    x = torch.from_numpy(synth.uniform_f32(c["seed"] + 2, 0, tuple(xh32.shape)))
    gx = 2.0 * (xh32 - x) / c["B"]
    xh = G(zd)
    xh.backward(gx.to(gpu_device))
    torch.cuda.synchronize()
    refs = []
    for Ls, dt in ((L32, torch.float32), (L64, torch.float64)):
        grads, gz, xr = orc.generator_train_grads(Ls, z.to(dt), gx.to(dt))
        d = dict(x_hat=xr.numpy(), grad_z=gz.numpy())
        for i, (gw, gb) in enumerate(grads):
            d["w%d" % i], d["b%d" % i] = gw.numpy(), gb.numpy()
        refs.append(d)
    convs = [m for m in G.gen if isinstance(m, torch.nn.ConvTranspose2d)]
    got = dict(x_hat=xh.detach().cpu().numpy(), grad_z=zd.grad.cpu().numpy())
    for i, m in enumerate(convs):
        got["w%d" % i], got["b%d" % i] = m.weight.grad.cpu().numpy(), m.bias.grad.cpu().numpy()
    names = ["x_hat"] + [k for i in range(len(convs)) for k in ("w%d" % i, "b%d" % i)] + ["grad_z"]
    U.check_rows("G7 stock layers", U.rule_rows(names, got, refs[0], refs[1], U.FWD))
