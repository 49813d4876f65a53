"""GPU: the per-op training calls of the Q and E updates called directly through ctypes, at the smallest shapes that
reach each GEMM route (tests/train_ops_util.py holds the tables and says what each case reaches):
damc_denoiser_train_forward / _backward, damc_ebm_train_*, damc_prior_emb_train_*, damc_q_loss_* and damc_q_noise_glue.

Rule: per tensor |hip - fp64| <= 3 |torch fp32 (CPU) - fp64| + 1e-6 in rel-L2, gradients floored at 1e-3 x the call's
largest gradient norm (train_ops_util.rule_rows); no tensor and no case is left out or masked.  Every output and every
workspace sits in a guarded buffer (encoder_ops_util.guarded: one NaN bit pattern in the payload, in front and behind);
the guards are compared after every library call, and as a workspace starts out as that pattern, a read of a region
nothing wrote shows as a non-finite output.  Run with -s for the per-tensor distances
(profiles/r18/train_ops_parity.txt is one such run).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_ops_util as T
from train_ops_util import assert_guards_intact, guarded, is_pattern

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_guards():
    T.reset_guards()
    yield
    T.reset_guards()


def _api(dev):
    from damc import _lib

    return _lib, _lib.lib(), _lib.stream_ptr(dev)


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _dev_copy(t, dev, offset=False):
    """t on the device; offset: one float past a 256-B aligned address, inside a guarded buffer."""
    if not offset:
        return t.to(dev).contiguous()
    d = guarded(tuple(t.shape), dev, lead=260)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4
    return d


# ------------------------------------------------------------------------------------------------ denoiser
@functools.lru_cache(maxsize=None)
def _dn_module(cid, dev):
    """The case's net on the device (its weights are read-only for every test)."""
    import copy

    return copy.deepcopy(T.dn_case(cid)["p"]).to(dev)


def _dn_prepare(dev, cid, want=None, want_zt=True, want_xemb=True, offset=False):
    """The case's buffers and its two calls: (out, forward(stream) -> rc, backward(stream) -> rc).  want: the names of
    the parameter gradients requested (None: all 68).  Every output is allocated and guarded whether requested or not;
    the workspace starts out as the NaN pattern."""
    from damc import training

    _lib, L, _ = _api(dev)
    ptr = _lib.ptr
    nz, nxemb, ntemb, nf, B, residual = T.DN_CASES[cid]
    c = T.dn_case(cid)
    p = _dn_module(cid, dev)
    d = T.dn_desc(p, lambda n, t: t.data_ptr())
    zt, xe, se, ge = (_dev_copy(c[k], dev, offset) for k in ("zt", "xemb", "se", "grad_eps"))
    nb = int(L.damc_denoiser_train_workspace_bytes(ctypes.byref(d), B))
    assert nb > 0
    ws = guarded(nb, dev)  # the NaN pattern throughout, before the forward
    out = dict(eps_pred=guarded((B, nz), dev), grad_zt=guarded((B, nz), dev), grad_xemb=guarded((B, nxemb), dev))
    for n, (_, _, q) in zip(T.dn_param_names(p), training._denoiser_params(p)):
        out[n] = guarded(tuple(q.shape), dev)
    assert out["wl[0]"].data_ptr() % 16 == 0
    g = T.dn_grads_struct(p, lambda n: out[n].data_ptr() if want is None or n in want else None)

    def forward(stream):
        return L.damc_denoiser_train_forward(ctypes.byref(d), ptr(zt), ptr(se), ptr(xe), B, ptr(out["eps_pred"]),
                                             ptr(ws), nb, stream)

    def backward(stream):
        return L.damc_denoiser_train_backward(ctypes.byref(d), ptr(ge), B, ctypes.byref(g),
                                              ptr(out["grad_zt"]) if want_zt else None,
                                              ptr(out["grad_xemb"]) if want_xemb else None, ptr(ws), nb, stream)

    return out, forward, backward


def _dn_run(dev, cid, **kw):
    """One forward and one backward of the case, the guards compared after each; returns copies of every output."""
    _lib, _, stream = _api(dev)
    out, forward, backward = _dn_prepare(dev, cid, **kw)
    rc = forward(stream)
    assert rc == 0, rc
    assert_guards_intact()
    rc = backward(stream)
    assert rc == 0, rc
    assert_guards_intact()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}


def _dn_check(label, cid, res):
    r32, r64 = T.dn_refs(cid)
    names = T.dn_tensor_names(cid)
    assert len(names) == 71
    got = {n: res[n].cpu().numpy() for n in names}
    T.check_rows(label, T.rule_rows(names, got, r32, r64, T.DN_FWD))
    return got


_DN_RUNS = [(cid, "default") for cid in T.DN_IDS] + [("D4", "group0"), ("D4", "smallgemm0")]


@pytest.mark.parametrize("cid,env", _DN_RUNS, ids=["%s-%s" % r for r in _DN_RUNS])
def test_denoiser_train_matches_fp64(gpu_device, monkeypatch, cid, env):
    for k, v in T.DN_ENVS[env].items():
        monkeypatch.setenv(k, v)
    res = _dn_run(gpu_device, cid)
    got = _dn_check("denoiser %s %s" % (cid, env), cid, res)
    if cid in T.DN_TAIL_CASES and env == "default":  # the rows and columns a tail bug would hit, slice-floored
        r32, r64 = T.dn_refs(cid)
        rows = []
        for n in ("eps_pred", "grad_zt", "grad_xemb"):
            rows += [(n,) + r for r in T.report("denoiser %s %s" % (cid, n), got[n], r32[n], r64[n],
                                                (("lastrow", (-1,)),))[1:]]
        for n in T.DN_TAIL_PARAMS:
            rows += [(n,) + r for r in T.report("denoiser %s %s" % (cid, n), got[n], r32[n], r64[n],
                                                (("lastrow", (-1,)), ("lastcol", (Ellipsis, -1))))[1:]]
        bad = [r for r in rows if not r[2] <= 3.0 * r[3] + 1e-6]
        assert not bad, bad


@pytest.mark.parametrize("cid", ["D1", "D4"])
def test_denoiser_train_is_repeatable(gpu_device, cid):
    """No atomics anywhere: two runs agree bit for bit in every output."""
    a, b = _dn_run(gpu_device, cid), _dn_run(gpu_device, cid)
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n


def test_denoiser_forward_rows_are_batch_independent(gpu_device):
    """D8 is D7's net on D7's first 16 rows: a forward row depends on its own inputs only."""
    a = _dn_run(gpu_device, "D7")["eps_pred"][:16].double()
    b = _dn_run(gpu_device, "D8")["eps_pred"].double()
    e = float((a - b).norm() / b.norm())
    print("D7[:16] vs D8 eps_pred: rel-L2 %.3e, bitwise %s" % (e, bool(torch.equal(a, b))))
    assert e <= 1e-6


@pytest.mark.parametrize("cid", ["D9", "D6"])
def test_denoiser_train_replays_from_a_captured_graph(gpu_device, cid):
    """The forward and backward recorded into a graph on a workspace that holds the NaN pattern, then replayed: every
    output is bitwise the eager call's.  Whatever the calls need zeroed must be written by something a replay orders
    before its readers.  The nz = 2 layout's zero padding used to be a memset node, the one kind of node DESIGN.md §1
    records a replay as not ordering before the kernels behind it; a captured toy Q update
    (test_gpu_dp.test_seeded_q_update_replays_from_a_captured_graph) once replayed with a bitwise loss and NaN in every
    gradient, which is what leftover NaN bits in the pad rows times the zero pad gradients give.  The padding is now
    written by the pack kernel.  This test passes with the memset form too whenever the memset happens to run first."""
    _lib, _, _ = _api(gpu_device)
    eager = _dn_run(gpu_device, cid)
    out, forward, backward = _dn_prepare(gpu_device, cid)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream = _lib.stream_ptr(gpu_device)
        rcs = (forward(stream), backward(stream))
    assert rcs == (0, 0), rcs
    assert all(is_pattern(t) for t in out.values())  # recorded, not run
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert_guards_intact()
        for n in out:
            assert torch.isfinite(out[n]).all(), (cid, n, "non-finite after a replay")
            assert _same_bits(out[n], eager[n]), (cid, n)


def _prof_counts(dev, fn):
    """Launch counts of the denoiser's three GEMM classes (and its column sums) during fn()."""
    _lib, L, _ = _api(dev)
    L.damc_prof_select(None)
    L.damc_prof_reset()
    L.damc_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for name in ("dn_gemm", "small_gemm", "small_gemm_group", "bias_grad"):
            ms, n, fl = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
            assert L.damc_prof_query(name.encode(), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)) == 0
            out[name] = int(n.value)
    finally:
        L.damc_prof_enable(0)
        L.damc_prof_reset()
    return out


def test_denoiser_cases_take_the_routes_the_table_names(gpu_device, monkeypatch):
    run = lambda cid: _prof_counts(gpu_device, lambda: _dn_run(gpu_device, cid))  # noqa: E731
    d1 = run("D1")
    print("D1 launches", d1)
    assert d1["dn_gemm"] > 0 and d1["small_gemm"] > 0 and d1["bias_grad"] > 0
    d5 = run("D5")
    print("D5 launches", d5)
    assert d5["dn_gemm"] > 0 and d5["small_gemm"] > 0 and d5["bias_grad"] > 0
    d4 = run("D4")
    print("D4 launches", d4)
    assert d4["small_gemm_group"] > 0 and d4["dn_gemm"] == 0 and d4["small_gemm"] == 0 and d4["bias_grad"] == 0
    for cid in ("D7", "D8"):  # every K = B member (each shares its group with a column sum) stayed on the grouped kernel,
        r = run(cid)          # idle waves and all; only the K = nz / 2 = 6 product and its group-mate leave it
        print(cid, "launches", r)
        assert r["small_gemm_group"] > 0 and r["bias_grad"] == 0 and r["dn_gemm"] == 1 and r["small_gemm"] == 1
    monkeypatch.setenv("DAMC_DN_GROUP", "0")
    g0 = run("D4")
    print("D4 DAMC_DN_GROUP=0 launches", g0)
    assert g0["small_gemm_group"] == 0 and g0["small_gemm"] > 0 and g0["bias_grad"] > 0
    monkeypatch.delenv("DAMC_DN_GROUP")
    monkeypatch.setenv("DAMC_DN_SMALL_GEMM", "0")
    s0 = run("D4")
    print("D4 DAMC_DN_SMALL_GEMM=0 launches", s0)
    assert s0["small_gemm_group"] == 0 and s0["small_gemm"] == 0 and s0["dn_gemm"] > 0 and s0["bias_grad"] > 0


@pytest.mark.parametrize("cid", ["D6", "D1"])
def test_denoiser_null_outputs_are_skipped(gpu_device, cid):
    """grad_zt NULL, grad_xemb NULL, and a grads struct with three entries: what is requested is bitwise the full
    call's, what is not still holds the guard pattern."""
    full = _dn_run(gpu_device, cid)
    params = T.dn_param_names(T.dn_case(cid)["p"])
    few = {"wl[3]", "bctx[0]", "tw1"}
    for label, kw in (("grad_zt NULL", dict(want_zt=False)), ("grad_xemb NULL", dict(want_xemb=False)),
                      ("three grads", dict(want=few))):
        res = _dn_run(gpu_device, cid, **kw)
        skipped = set()
        if not kw.get("want_zt", True):
            skipped.add("grad_zt")
        if not kw.get("want_xemb", True):
            skipped.add("grad_xemb")
        if "want" in kw:
            skipped |= set(params) - few
        for n in res:
            if n in skipped:
                assert is_pattern(res[n]), (cid, label, n, "was written")
            else:
                assert torch.equal(res[n].view(torch.int32), full[n].view(torch.int32)), (cid, label, n)


@pytest.mark.parametrize("cid", ["D6", "D3"])
def test_denoiser_caller_tensors_offset_by_one_float(gpu_device, cid):
    """zt, xemb, temb_in and grad_eps one float off a 16-B boundary (include/damc.h: only the workspace needs 16 B).
    The kernels that touch them read one float at a time (input_emb*, emb_finish_kernel, csq_combine_kernel's residual,
    csq_bwd_kernel, dz_kernel, the memcpy of temb_in); zt as the A operand of the z B product leaves the float4
    kernels for the engine's scalar gather."""
    res = _dn_run(gpu_device, cid, offset=True)
    _dn_check("denoiser %s inputs+4B" % cid, cid, res)


# ------------------------------------------------------------------------------------------------ E update
def _ebm_desc(_lib, w):
    d = _lib.Ebm()
    d.nz, d.nh, d.slope = w["w1"].shape[1], w["w1"].shape[0], T.E_SLOPE
    for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
        setattr(d, k, w[k].data_ptr())
    return d


E_PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")


def _e_run(dev, case, want=E_PARAMS, want_z=True, g=None, stride=1):
    """damc_ebm_train_forward + _backward; g: the upstream gradient buffer (element stride `stride`)."""
    _lib, L, stream = _api(dev)
    ptr = _lib.ptr
    B, nz, nh = case
    seq, z, gv = T.e_case(case)
    w = dict(zip(E_PARAMS, [q.detach().to(dev).contiguous() for q in seq.parameters()]))
    d = _ebm_desc(_lib, w)
    zd = z.to(dev)
    out = dict(h1=guarded((B, nh), dev), h2=guarded((B, nh), dev), energy=guarded((B,), dev),
               grad_z=guarded((B, nz), dev))
    for k in E_PARAMS:
        out[k] = guarded(tuple(w[k].shape), dev)
    rc = L.damc_ebm_train_forward(ctypes.byref(d), ptr(zd), B, ptr(out["h1"]), ptr(out["h2"]), ptr(out["energy"]), stream)
    assert rc == 0, rc
    assert_guards_intact()
    nb = int(L.damc_ebm_train_workspace_bytes(ctypes.byref(d), B))
    assert nb > 0
    ws = guarded(nb, dev)
    gr = _lib.EbmGrads()
    for k in want:
        setattr(gr, k, out[k].data_ptr())
    gd = gv.to(dev) if g is None else g
    rc = L.damc_ebm_train_backward(ctypes.byref(d), ptr(zd), ptr(out["h1"]), ptr(out["h2"]), ptr(gd), stride, B,
                                   ctypes.byref(gr), ptr(out["grad_z"]) if want_z else None, ptr(ws), nb, stream)
    assert rc == 0, rc
    assert_guards_intact()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", T.E_CASES, ids=T.case_id)
def test_ebm_train_matches_fp64(gpu_device, case):
    res = _e_run(gpu_device, case)
    r32, r64 = T.e_refs(case)
    got = {n: res[n].cpu().numpy() for n in T.E_NAMES}
    T.check_rows("ebm %s" % T.case_id(case), T.rule_rows(T.E_NAMES, got, r32, r64, T.E_FWD))


@pytest.mark.parametrize("case", T.E_CASES, ids=T.case_id)
def test_ebm_train_grad_stride(gpu_device, case):
    """The same upstream value as one scalar (stride 0), a dense vector (1) and a strided view (3, NaN between)."""
    B = case[0]
    c = 1.0 / B
    g0 = torch.full((1,), c, device=gpu_device)
    g1 = torch.full((B,), c, device=gpu_device)
    g3 = torch.full((3 * B,), float("nan"), device=gpu_device)
    g3[::3] = c
    a = _e_run(gpu_device, case, g=g0, stride=0)
    for g, s in ((g1, 1), (g3, 3)):
        b = _e_run(gpu_device, case, g=g, stride=s)
        for n in a:
            assert _same_bits(a[n], b[n]), (case, s, n)
    assert torch.isfinite(a["w1"]).all() and torch.isfinite(a["grad_z"]).all()


@pytest.mark.parametrize("case", T.E_CASES, ids=T.case_id)
def test_ebm_train_null_outputs_are_skipped(gpu_device, case):
    full = _e_run(gpu_device, case)
    for label, want, want_z in (("grad_z only", (), True), ("w3 b3 only", ("w3", "b3"), False),
                                ("nothing", (), False), ("all but grad_z", E_PARAMS, False)):
        res = _e_run(gpu_device, case, want=want, want_z=want_z)
        for n in E_PARAMS + ("grad_z",):
            if n in want or (n == "grad_z" and want_z):
                assert _same_bits(res[n], full[n]), (case, label, n)
            else:
                assert is_pattern(res[n]), (case, label, n, "was written")


def test_ebm_train_refuses_misaligned_before_writing(gpu_device):
    """A weight (or z) one float off a 16-B boundary: DAMC_ERR_UNSUPPORTED from the host, h1 / h2 / energy untouched (the
    check used to sit in the launcher: a misaligned w2 was refused after h1 had been written); the drop-in then keeps the
    stock modules."""
    from damc import training
    from src import diffusion_net as dn

    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    case = T.E_CASES[1]
    B, nz, nh = case
    seq, z, _ = T.e_case(case)
    zd = z.to(gpu_device)
    for which in ("w1", "w2", "w3", "z"):
        w = {k: _dev_copy(q.detach(), gpu_device, offset=(k == which)) for k, q in zip(E_PARAMS, seq.parameters())}
        d = _ebm_desc(_lib, w)
        zz = _dev_copy(z, gpu_device, offset=(which == "z"))
        h1, h2, e = guarded((B, nh), gpu_device), guarded((B, nh), gpu_device), guarded((B,), gpu_device)
        rc = L.damc_ebm_train_forward(ctypes.byref(d), ptr(zz), B, ptr(h1), ptr(h2), ptr(e), stream)
        assert rc == _lib.DAMC_ERR_UNSUPPORTED, (which, rc)
        assert_guards_intact()
        assert is_pattern(h1) and is_pattern(h2) and is_pattern(e), which
        assert (int(L.damc_ebm_train_workspace_bytes(ctypes.byref(d), B)) == 0) == (which != "z")
    # the drop-in: a misaligned first weight keeps the stock modules, and E(z) still evaluates
    E = dn._netE(nz=nz).to(gpu_device).train()
    zt = zd[:, :E.ebm[0].in_features].contiguous()
    assert training.ebm_apply(E, zt) is not None
    lin = E.ebm[0]
    buf = torch.zeros(lin.weight.numel() + 1, device=gpu_device)
    buf[1:] = lin.weight.detach().flatten()
    lin.weight = torch.nn.Parameter(buf[1:].view_as(lin.weight))
    assert lin.weight.data_ptr() % 16 == 4
    assert training.ebm_apply(E, zt) is None
    en = E(zt)
    en.sum().backward()
    assert torch.isfinite(en).all() and lin.weight.grad is not None and torch.isfinite(lin.weight.grad).all()


# ------------------------------------------------------------------------------------------------ prior embedding
PE_PARAMS = ("w1", "b1", "w2", "b2")


def _pe_run(dev, case, slope, want=PE_PARAMS):
    _lib, L, stream = _api(dev)
    ptr = _lib.ptr
    B, nz, nh, nout = case
    seq, x, g = T.pe_case(case, slope)
    w = dict(zip(PE_PARAMS, [q.detach().to(dev).contiguous() for q in seq.parameters()]))
    d = _lib.PriorEmb()
    d.nz, d.nh, d.nout, d.slope = nz, nh, nout, slope
    for k in PE_PARAMS:
        setattr(d, k, w[k].data_ptr())
    xd, gd = x.to(dev), g.to(dev)
    out = dict(h=guarded((B, nh), dev), out=guarded((B, nout), dev))
    for k in PE_PARAMS:
        out[k] = guarded(tuple(w[k].shape), dev)
    rc = L.damc_prior_emb_train_forward(ctypes.byref(d), ptr(xd), B, ptr(out["h"]), ptr(out["out"]), stream)
    assert rc == 0, rc
    assert_guards_intact()
    nb = int(L.damc_prior_emb_train_workspace_bytes(ctypes.byref(d), B))
    assert nb > 0
    ws = guarded(nb, dev)
    gr = _lib.PriorEmbGrads()
    for k in want:
        setattr(gr, k, out[k].data_ptr())
    rc = L.damc_prior_emb_train_backward(ctypes.byref(d), ptr(xd), ptr(out["h"]), ptr(gd), B, ctypes.byref(gr), ptr(ws),
                                         nb, stream)
    assert rc == 0, rc
    assert_guards_intact()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}


_PE_IDS = [T.case_id(c + (s,)) for c, s in T.PE_CASES]


@pytest.mark.parametrize("case,slope", T.PE_CASES, ids=_PE_IDS)
def test_prior_emb_train_matches_fp64(gpu_device, case, slope):
    res = _pe_run(gpu_device, case, slope)
    r32, r64 = T.pe_refs(case, slope)
    got = {n: res[n].cpu().numpy() for n in T.PE_NAMES}
    T.check_rows("prior_emb %s" % T.case_id(case + (slope,)), T.rule_rows(T.PE_NAMES, got, r32, r64, T.PE_FWD))


@pytest.mark.parametrize("case,slope", T.PE_CASES, ids=_PE_IDS)
def test_prior_emb_train_null_outputs_are_skipped(gpu_device, case, slope):
    full = _pe_run(gpu_device, case, slope)
    for label, want in (("w2 NULL", ("w1", "b1", "b2")), ("w1 b1 NULL", ("w2", "b2")), ("nothing", ())):
        res = _pe_run(gpu_device, case, slope, want=want)
        for n in PE_PARAMS:
            if n in want:
                assert _same_bits(res[n], full[n]), (case, label, n)
            else:
                assert is_pattern(res[n]), (case, label, n, "was written")


def test_prior_emb_train_refuses_misaligned_before_writing(gpu_device):
    from damc import training

    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    case, slope = T.PE_CASES[1]
    B, nz, nh, nout = case
    seq, x, _ = T.pe_case(case, slope)
    for which in ("w1", "w2"):
        w = {k: _dev_copy(q.detach(), gpu_device, offset=(k == which)) for k, q in zip(PE_PARAMS, seq.parameters())}
        d = _lib.PriorEmb()
        d.nz, d.nh, d.nout, d.slope = nz, nh, nout, slope
        for k in PE_PARAMS:
            setattr(d, k, w[k].data_ptr())
        h, o = guarded((B, nh), gpu_device), guarded((B, nout), gpu_device)
        rc = L.damc_prior_emb_train_forward(ctypes.byref(d), ptr(x.to(gpu_device)), B, ptr(h), ptr(o), stream)
        assert rc == _lib.DAMC_ERR_UNSUPPORTED, (which, rc)
        assert_guards_intact()
        assert is_pattern(h) and is_pattern(o), which
        assert int(L.damc_prior_emb_train_workspace_bytes(ctypes.byref(d), B)) == 0
    import copy

    mod = copy.deepcopy(seq).to(gpu_device)
    xd = x.to(gpu_device)
    assert training.prior_emb_apply(mod, xd) is not None
    lin = mod[2]
    buf = torch.zeros(lin.weight.numel() + 1, device=gpu_device)
    buf[1:] = lin.weight.detach().flatten()
    lin.weight = torch.nn.Parameter(buf[1:].view_as(lin.weight))
    assert training.prior_emb_apply(mod, xd) is None


# ------------------------------------------------------------------------------------------------ q_loss
@pytest.mark.parametrize("case", T.QLOSS_CASES, ids=T.case_id)
def test_q_loss_forward_and_bitwise_backward(gpu_device, case):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, nz = case
    eps, pred = (t.to(gpu_device) for t in T.qloss_inputs(case))
    loss = guarded((B,), gpu_device)
    assert L.damc_q_loss_forward(ptr(eps), ptr(pred), B, nz, ptr(loss), stream) == 0
    assert_guards_intact()
    l32, _ = T.qloss_ref(case, torch.float32)
    l64, _ = T.qloss_ref(case, torch.float64)
    T.check_rows("q_loss %s" % T.case_id(case), T.rule_rows(("loss",), {"loss": _np(loss)}, {"loss": l32},
                                                            {"loss": l64}, ("loss",)))
    from damc import synth

    gvec = torch.from_numpy(synth.normal_f32(76, nz, (B,)))
    for stride in (0, 1, 2):
        if stride == 0:
            gref = torch.full((B,), 1.0 / 3.0)  # one scalar for every row, not a power of two
            gd = gref[:1].to(gpu_device)
        elif stride == 1:
            gref, gd = gvec, gvec.to(gpu_device)
        else:
            gref = gvec
            gd = torch.full((2 * B,), float("nan"), device=gpu_device)
            gd[::2] = gvec.to(gpu_device)
        gp = guarded((B, nz), gpu_device)
        assert L.damc_q_loss_backward(ptr(eps), ptr(pred), ptr(gd), stride, B, nz, ptr(gp), stream) == 0
        assert_guards_intact()
        _, ref = T.qloss_ref(case, torch.float32, gref)
        got = _np(gp)
        same = np.array_equal(got.view(np.int32), ref.view(np.int32))
        print("q_loss backward %s stride %d: bitwise %s, max abs diff %.3e"
              % (T.case_id(case), stride, same, float(np.abs(got.astype(np.float64) - ref).max())))
        assert same, (case, stride)


# ------------------------------------------------------------------------------------------------ q_noise_glue
@pytest.mark.parametrize("case", T.GLUE_CASES, ids=T.case_id)
def test_q_noise_glue_small_shapes(gpu_device, case):
    """test_gpu_training.test_q_noise_glue_matches_torch_ops' comparison and bounds (5e-7, 5e-7, 2.5e-4) at shapes where
    nz < ntemb, nz > ntemb and B = 1, with guarded outputs, and with logsnr NULL."""
    from damc import synth, training
    from src import diffusion_helper_func as dh
    from src import diffusion_net as dn

    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, nz, ntemb = case
    lmin, lmax = T.GLUE_LOGSNR
    u = torch.from_numpy(synth.uniform_f32(73, nz, (B,), 0.0, 1.0)).to(gpu_device)
    z = torch.from_numpy(synth.normal_f32(74, nz, (B, nz))).to(gpu_device)
    eps = torch.from_numpy(synth.normal_f32(75, nz, (B, nz))).to(gpu_device)
    freqs = training._freqs(ntemb // 2, gpu_device)
    outs = []
    for with_l in (True, False):
        lg, zt, se = guarded((B,), gpu_device), guarded((B, nz), gpu_device), guarded((B, ntemb), gpu_device)
        rc = L.damc_q_noise_glue(ptr(u), ptr(z), ptr(eps), B, nz, T.c_float(lmin), T.c_float(lmax), ptr(freqs), ntemb,
                                 ptr(lg) if with_l else None, ptr(zt), ptr(se), stream)
        assert rc == 0, rc
        assert_guards_intact()
        torch.cuda.synchronize()
        outs.append((lg.clone(), zt.clone(), se.clone()))
    (lg, zt, se), (lg_n, zt_n, se_n) = outs
    assert is_pattern(lg_n) and _same_bits(zt, zt_n) and _same_bits(se, se_n)
    l = dh.logsnr_schedule_fn(u, logsnr_max=lmax, logsnr_min=lmin)
    fwd = dh.diffusion_forward(z, logsnr=l.reshape(B, 1))
    zt_ref = fwd["mean"] + fwd["std"] * eps
    t_in = torch.arctan(torch.exp(-0.5 * torch.clamp(l, min=-20.0, max=20.0))) / (0.5 * np.pi)
    se_ref = dn.SinusoidalPosEmb(ntemb, max_time=1.0)(t_in)
    dl = float(((lg - l).abs() / l.abs().clamp_min(1e-30)).max())
    dz = float(((zt - zt_ref).abs() / (fwd["mean"].abs() + (fwd["std"] * eps).abs())).max())
    ds = float((se - se_ref).abs().max())
    print("q_noise_glue %s: logsnr max rel %.2e, zt max rel %.2e, temb max abs %.2e" % (T.case_id(case), dl, dz, ds))
    assert torch.isfinite(zt).all() and torch.isfinite(se).all() and torch.isfinite(lg).all()
    assert dl < 5e-7 and dz < 5e-7 and ds < 2.5e-4
