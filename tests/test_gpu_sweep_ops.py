"""GPU: the reverse sweep (damc_reverse_sweep, damc_denoise_step) through ctypes on hand-built descriptors, every form
(row-resident, team on the generic and on the shape-specialised kernel, launch chain cached-graph and eager) at the edge
shapes of tests/sweep_ops_util.py, against the fp64 evaluation of the same sweep on the same host tables.

Rule: |hip - fp64| <= 3 |torch fp32 - fp64| + 1e-6 in rel-L2 (encoder_ops_util.check) for the eps of every step and the
end point: whole, last row, last column.  Every weight, input, table, output and the workspace (exactly
damc_sweep_workspace_bytes) sit in guarded buffers checked after every call; xemb and the weights must come back
unchanged.  The form a run is meant to take is asserted through damc_sweep_form before the call.

Forced fix (csrc/denoiser_rows.hip rows_layout): at 32 < w % 64 < 64 the row image ended before out2's padded K range,
so launch_sweep_rows returned DAMC_ERR_UNSUPPORTED for shapes damc_sweep_workspace_bytes admits: T3-rows, T4-rows and
every narrow denoiser of w = 48, 112, 176, 240 (N4 was w = 240 then, with no other form to fall to).  Read from
launch_rows' own bound check.  With the fix reverted (the library rebuilt with the old row stride, one run):
test_sweep_matches_fp64[T3-rows], [T4-rows] and [N4-rows] (w = 240) fail with damc_reverse_sweep returning 1003 where
damc_sweep_form says 1; [T1-rows] (w = 32) passes.
"""
import ctypes

import numpy as np
import pytest
import torch

import sweep_ops_util as su

pytestmark = pytest.mark.gpu

SWITCHES = ("DAMC_SWEEP_TEAM", "DAMC_SWEEP_FAST", "DAMC_SWEEP_ROWS", "DAMC_SWEEP_GRAPH")
FORM_ENV = {"default": {}, "generic": {"DAMC_SWEEP_FAST": "0"}, "chain": {"DAMC_SWEEP_TEAM": "0"},
            "eager": {"DAMC_SWEEP_TEAM": "0", "DAMC_SWEEP_GRAPH": "0"}, "rows": {"DAMC_SWEEP_ROWS": "1"}}
FORM_NAME = {0: "none", 1: "rows", 2: "team", 3: "team-fast", 4: "chain"}


def set_form(monkeypatch, form):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORM_ENV[form].items():
        monkeypatch.setenv(k, v)


def expected_form(cid, form):
    if form in ("chain", "eager"):
        return su.FORM_CHAIN
    if form == "rows":
        return su.FORM_ROWS
    if form == "generic":
        return su.FORM_TEAM
    return su.DEFAULT_FORM[cid]


def to_guarded(t, dev):
    g = su.guarded(tuple(t.shape), dev)
    g.copy_(t)
    return g


class Case:
    """A case's weights on the device (guarded) and its damc_denoiser_t."""

    def __init__(self, cid, dev):
        from damc import _lib

        su.reset_guards()
        self.cid, self.dev = cid, dev
        self.nz, self.w, self.nt, self.nx, self.B, self.res = su.shape(cid)
        self.L = _lib.lib()
        W = su.weights(cid)
        self.host, self.devt = [], []
        d = _lib.Denoiser()
        d.nz, d.ntemb, d.nxemb, d.residual = self.nz, self.nt, self.nx, self.res

        def up(t):
            g = to_guarded(t, dev)
            self.host.append(t)
            self.devt.append(g)
            return g.data_ptr()

        for k in ("bmat", "tw1", "tb1", "tw2", "tb2"):
            setattr(d, k, up(W[k]))
        for j, ((din, dout), b) in enumerate(zip(su.block_dims(self.nz, self.w), W["blocks"])):
            d.blocks[j].din, d.blocks[j].dout = din, dout
            for k in ("wl", "bl", "ws", "bs", "wg", "bg", "wb"):
                setattr(d.blocks[j], k, up(b[k]))
            d.wctx[j] = up(b["wctx"])
            d.bctx[j] = up(b["bctx"])
        self.d = d

    def form(self, B, n):
        return self.L.damc_sweep_form(ctypes.byref(self.d), B, n)

    def run(self, coef, temb, noise=None, rows=None, seed=0, chain_base=0, eps_steps=None, want_rc=0, ws_bytes=None,
            step=None):
        """One damc_reverse_sweep (step = (k, zt): one damc_denoise_step on row k of the tables from zt) on rows
        `rows` of the case's inputs.  noise: None (seeded Philox), a (n - 1, B', nz) tensor, or False (with_noise 0).
        Returns (eps (n, B', nz), zt (B', nz)) as CPU tensors, or the workspace when a refusal is expected."""
        from damc import _lib
        from damc._lib import ptr

        I = su.inputs(self.cid)
        sl = slice(None) if rows is None else rows
        xemb_h = I["xemb"][sl].contiguous()
        zt0 = (I["zt0"][sl] if step is None else step[1]).contiguous()
        B, n = zt0.shape[0], (coef.shape[0] if step is None else 1)
        dev = self.dev
        xemb, zt = to_guarded(xemb_h, dev), to_guarded(zt0, dev)
        tin = to_guarded(temb if step is None else temb[step[0]:step[0] + 1], dev)
        coef_h = np.ascontiguousarray((coef if step is None else coef[step[0]:step[0] + 1]).numpy())
        nse = to_guarded(noise, dev) if torch.is_tensor(noise) and noise.numel() else None
        eps_steps = n if eps_steps is None else eps_steps
        eps = su.guarded((max(eps_steps, 1), B, self.nz), dev)
        nb = int(self.L.damc_sweep_workspace_bytes(ctypes.byref(self.d), B, n)) if ws_bytes is None else ws_bytes
        assert nb > 0
        ws = su.guarded(nb, dev)
        dref, cp, stream = ctypes.byref(self.d), coef_h.ctypes.data_as(ctypes.c_void_p), _lib.stream_ptr(dev)
        with_noise = 0 if noise is False else 1
        if step is None:
            rc = self.L.damc_reverse_sweep(dref, ptr(xemb), ptr(zt), B, n, ptr(tin), cp, with_noise, ptr(nse), seed,
                                           chain_base, ptr(eps), eps_steps, ptr(ws), nb, stream)
        else:
            rc = self.L.damc_denoise_step(dref, ptr(xemb), ptr(zt), B, ptr(tin), cp, with_noise, ptr(nse), seed, step[0],
                                          chain_base, ptr(eps), ptr(ws), nb, stream)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:  # a device fault is sticky: nothing after it in this process can run
            pytest.exit("device error after %s: %s" % (self.cid, e), returncode=3)
        su.assert_guards_intact()
        assert rc == want_rc, (self.cid, rc, want_rc)
        assert torch.equal(xemb.cpu(), xemb_h), "xemb changed"
        for h, g in zip(self.host, self.devt):
            assert torch.equal(g.cpu(), h), "a weight changed"
        if want_rc:
            assert torch.equal(zt.cpu(), zt0), "zt touched by a refused call"
            return ws
        return eps[:eps_steps].cpu(), zt.cpu()


def check_sweep(name, got, r32, r64, steps=None):
    eps, zt = got
    for k in range(eps.shape[0] if steps is None else steps):
        su.check("%s eps[%d]" % (name, k), eps[k].numpy(), r32["eps"][k], r64["eps"][k], su.SLICES)
    su.check("%s zt" % name, zt.numpy(), r32["zt"], r64["zt"], su.SLICES)


def default_run(c, form_env, monkeypatch, **kw):
    set_form(monkeypatch, form_env)
    coef, temb = su.tables(su.N_STEPS, c.nt)
    return c.run(coef, temb, **kw)


# ------------------------------------------------------------------------------------------------ 1. parity
PARITY = [(c, f) for c in su.WIDE_IDS for f in ("default", "chain", "rows")] + [(c, "rows") for c in su.N_IDS]


@pytest.mark.parametrize("cid,form", PARITY, ids=["%s-%s" % p for p in PARITY])
def test_sweep_matches_fp64(gpu_device, monkeypatch, cid, form):
    c = Case(cid, gpu_device)
    coef, temb = su.tables(su.N_STEPS, c.nt)
    noise = su.inputs(cid)["noise"]
    r32, r64 = su.refs(cid)
    dev_index = gpu_device.index or 0
    set_form(monkeypatch, "default")
    nb_default = int(c.L.damc_sweep_workspace_bytes(ctypes.byref(c.d), c.B, su.N_STEPS))
    set_form(monkeypatch, form)
    got_form = c.form(c.B, su.N_STEPS)
    print("%s %s: form %d (%s)" % (cid, form, got_form, FORM_NAME[got_form]))
    if form == "rows" and not (su.stages_of(cid) & su.ST_ROWS_FIT):
        assert got_form == su.FORM_NONE
        assert c.L.damc_sweep_workspace_bytes(ctypes.byref(c.d), c.B, su.N_STEPS) == 0
        ws = c.run(coef, temb, noise, want_rc=su.ERR_UNSUPPORTED, ws_bytes=nb_default)
        assert su.is_pattern(ws.view(torch.float32)), "workspace written by a refused call"
        return
    want = expected_form(cid, form)
    if want is None:
        assert got_form in (su.FORM_TEAM, su.FORM_CHAIN), got_form
    else:
        assert got_form == want, (cid, form, got_form, want)
    fails = c.L.damc_sweep_team_failures(dev_index)
    got = c.run(coef, temb, noise)
    check_sweep("%s %s" % (cid, FORM_NAME[got_form]), got, r32, r64)
    if got_form in (su.FORM_TEAM, su.FORM_FAST):
        assert c.L.damc_sweep_team_failures(dev_index) == fails, "a team launch needed the rescue"


# ------------------------------------------------------------------------------------------------ 2. forms
def test_default_forms(gpu_device, monkeypatch):
    from damc import _lib

    set_form(monkeypatch, "default")
    for cid in su.CASES:
        nz, w, nt, nx, B, res = su.shape(cid)
        f = _lib.lib().damc_sweep_form(ctypes.byref(su.host_desc(nz, w, nt, nx, res)), B, su.N_STEPS)
        print("%s %s: default form %d (%s)" % (cid, su.shape(cid), f, FORM_NAME[f]))
        if su.DEFAULT_FORM[cid] is None:
            assert f in (su.FORM_TEAM, su.FORM_CHAIN), (cid, f)
        else:
            assert f == su.DEFAULT_FORM[cid], (cid, f)
    # F1: the shape-specialised kernel and the generic one are bitwise equal
    c = Case("F1", gpu_device)
    noise = su.inputs("F1")["noise"]
    assert c.form(c.B, su.N_STEPS) == su.FORM_FAST
    fast = default_run(c, "default", monkeypatch, noise=noise)
    set_form(monkeypatch, "generic")
    assert c.form(c.B, su.N_STEPS) == su.FORM_TEAM
    gen = default_run(c, "generic", monkeypatch, noise=noise)
    assert torch.isfinite(fast[1]).all()
    assert torch.equal(fast[0], gen[0]) and torch.equal(fast[1], gen[1])


# ------------------------------------------------------------------------------------------------ 3. n = 1, the hook
@pytest.mark.parametrize("cid", ["T3", "N2"])
def test_single_step_and_hook(gpu_device, monkeypatch, cid):
    c = Case(cid, gpu_device)
    set_form(monkeypatch, "default")
    assert c.form(c.B, 1) == su.DEFAULT_FORM[cid] and c.form(c.B, su.N_STEPS) == su.DEFAULT_FORM[cid]
    coef1, temb1 = su.single_step_tables(c.nt)
    s32, s64 = su.single_step_refs(cid)
    check_sweep("%s n=1" % cid, c.run(coef1, temb1, noise=False), s32, s64)
    # three damc_denoise_step calls are the n = 3 sweep
    coef, temb = su.tables(su.N_STEPS, c.nt)
    noise = su.inputs(cid)["noise"]
    eps, zt = c.run(coef, temb, noise)
    z = su.inputs(cid)["zt0"]
    for k in range(su.N_STEPS):
        last = k == su.N_STEPS - 1
        e, z = c.run(coef, temb, noise=False if last else noise[k:k + 1], step=(k, z))
        assert torch.equal(e[0], eps[k]), (cid, k)
    assert torch.isfinite(zt).all() and torch.equal(z, zt)


# ------------------------------------------------------------------------------------------------ 4. n > 256
def test_long_table(gpu_device, monkeypatch):
    """257 steps: past TS_TAB_STEPS the team kernel reads its step rows from memory, not from LDS."""
    c = Case("T1", gpu_device)
    set_form(monkeypatch, "default")
    n = su.LONG_STEPS
    assert c.form(c.B, n) == su.FORM_TEAM
    coef, temb = su.tables(n, c.nt)
    r32, r64 = su.refs("T1", n)
    got = c.run(coef, temb, su.inputs("T1", n)["noise"], eps_steps=2)
    check_sweep("T1 team n=%d" % n, got, r32, r64, steps=2)


# ------------------------------------------------------------------------------------------------ 5. Philox
SEEDED = [("T3", "default", 5), ("T4", "chain", 2), ("N2", "rows", 9)]


@pytest.mark.parametrize("cid,form,cut", SEEDED, ids=["%s-%s" % p[:2] for p in SEEDED])
def test_seeded_equals_injected_stream(gpu_device, monkeypatch, cid, form, cut):
    from damc.langevin import philox_normal

    c = Case(cid, gpu_device)
    set_form(monkeypatch, form)
    assert c.form(c.B, su.N_STEPS) == expected_form(cid, form)
    coef, temb = su.tables(su.N_STEPS, c.nt)
    seed, base = 1234, 40
    seeded = c.run(coef, temb, None, seed=seed, chain_base=base)
    pn = philox_normal(su.N_STEPS - 1, c.B, c.nz, seed, gpu_device, step_offset=0, chain_base=base,
                       stream_id=su.STREAM_SWEEP).cpu()
    injected = c.run(coef, temb, pn)
    assert torch.isfinite(seeded[1]).all() and not torch.equal(seeded[1], su.inputs(cid)["zt0"])
    assert torch.equal(seeded[0], injected[0]) and torch.equal(seeded[1], injected[1])
    unseeded = c.run(coef, temb, False)
    assert not torch.equal(unseeded[1], seeded[1])
    parts = [c.run(coef, temb, None, rows=slice(a, b), seed=seed, chain_base=base + a)
             for a, b in ((0, cut), (cut, c.B))]
    assert torch.equal(torch.cat([p[0] for p in parts], 1), seeded[0])
    assert torch.equal(torch.cat([p[1] for p in parts], 0), seeded[1])


# ------------------------------------------------------------------------------------------------ 6. rows alone
ALONE = [("T2", "default"), ("T3", "chain"), ("N2", "rows")]


@pytest.mark.parametrize("cid,form", ALONE, ids=["%s-%s" % p for p in ALONE])
def test_rows_do_not_depend_on_the_batch(gpu_device, monkeypatch, cid, form):
    c = Case(cid, gpu_device)
    set_form(monkeypatch, form)
    assert c.form(c.B, su.N_STEPS) == expected_form(cid, form) == c.form(1, su.N_STEPS)
    coef, temb = su.tables(su.N_STEPS, c.nt)
    noise = su.inputs(cid)["noise"]
    whole = c.run(coef, temb, noise)
    alone = c.run(coef, temb, noise[:, -1:].contiguous(), rows=slice(c.B - 1, c.B))
    assert torch.isfinite(whole[1]).all()
    assert torch.equal(alone[0], whole[0][:, -1:]) and torch.equal(alone[1], whole[1][-1:])


# ------------------------------------------------------------------------------------------------ 7. graph
@pytest.mark.parametrize("cid", ["T3", "W2"])
def test_chain_graph_equals_eager(gpu_device, monkeypatch, cid):
    c = Case(cid, gpu_device)
    noise = su.inputs(cid)["noise"]
    set_form(monkeypatch, "chain")
    assert c.form(c.B, su.N_STEPS) == su.FORM_CHAIN
    graph = default_run(c, "chain", monkeypatch, noise=noise)
    eager = default_run(c, "eager", monkeypatch, noise=noise)
    assert c.form(c.B, su.N_STEPS) == su.FORM_CHAIN
    assert torch.isfinite(graph[1]).all()
    assert torch.equal(graph[0], eager[0]) and torch.equal(graph[1], eager[1])


# ------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("what,args,null,code", su.REFUSALS, ids=[r[0] for r in su.REFUSALS])
def test_refusals(gpu_device, monkeypatch, what, args, null, code):
    """validate()'s refusals from damc_reverse_sweep itself: the code, with zt and the workspace untouched."""
    from damc import _lib
    from damc._lib import ptr

    set_form(monkeypatch, "default")
    su.reset_guards()
    L = _lib.lib()
    d = su.host_desc(null=null, **args)
    B, n, nz = 4, su.N_STEPS, args["nz"]
    coef, temb = su.tables(n, args["ntemb"])
    zt, xemb = su.guarded((B, nz), gpu_device), to_guarded(torch.zeros(B, args["nxemb"]), gpu_device)
    tin, ws = to_guarded(temb, gpu_device), su.guarded(1 << 16, gpu_device)
    coef_h = np.ascontiguousarray(coef.numpy())
    assert L.damc_sweep_form(ctypes.byref(d), B, n) == su.FORM_NONE
    rc = L.damc_reverse_sweep(ctypes.byref(d), ptr(xemb), ptr(zt), B, n, ptr(tin),
                              coef_h.ctypes.data_as(ctypes.c_void_p), 1, None, 1, 0, None, 0, ptr(ws), 1 << 16,
                              _lib.stream_ptr(gpu_device))
    torch.cuda.synchronize()
    su.assert_guards_intact()
    assert rc == code, (what, rc, code)
    assert su.is_pattern(zt) and su.is_pattern(ws.view(torch.float32))
