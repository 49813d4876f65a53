"""No GPU: the case table of tests/sweep_ops_util.py against the library's host queries (damc_sweep_stages,
damc_sweep_workspace_bytes), and the table's reference against the drop-in module's stock CPU path."""
import ctypes

import numpy as np
import pytest
import torch

import sweep_ops_util as su

ALL_IDS = list(su.CASES)


def _lib():
    from damc import _lib

    return _lib.lib()


def _desc(cid):
    nz, w, nt, nx, _, res = su.shape(cid)
    return su.host_desc(nz, w, nt, nx, res)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_stages_mask_is_the_tables(cid):
    got = _lib().damc_sweep_stages(ctypes.byref(_desc(cid)))
    assert got == su.stages_of(cid), (cid, hex(got), hex(su.stages_of(cid)))
    nz, w = su.shape(cid)[:2]
    assert bool(got & su.ST_NARROW) == (nz % 4 != 0)
    limb = got >> 8
    assert limb in (0, 0x3F if nz % 4 else 0x7F), "the hyper stage's blocks go to the limb product together or not at all"
    if limb:
        assert all(dout % 32 == 0 and dout <= 512 for _, dout in su.block_dims(nz, w)[:6 if nz % 4 else 7])


@pytest.mark.parametrize("cid", ALL_IDS)
def test_cases_have_a_workspace(cid):
    B = su.shape(cid)[4]
    L = _lib()
    assert L.damc_sweep_workspace_bytes(ctypes.byref(_desc(cid)), B, su.N_STEPS) > 0
    assert L.damc_sweep_workspace_bytes(ctypes.byref(_desc(cid)), B, 0) == 0
    assert L.damc_sweep_workspace_bytes(ctypes.byref(_desc(cid)), 0, su.N_STEPS) == 0


@pytest.mark.parametrize("what,args,null,code", su.REFUSALS, ids=[r[0] for r in su.REFUSALS])
def test_refusals_host(what, args, null, code):
    L = _lib()
    d = su.host_desc(null=null, **args)
    assert L.damc_sweep_workspace_bytes(ctypes.byref(d), 4, su.N_STEPS) == 0
    assert L.damc_sweep_stages(ctypes.byref(d)) == -code
    assert L.damc_sweep_form(ctypes.byref(d), 4, su.N_STEPS) == su.FORM_NONE


def test_null_descriptor():
    L = _lib()
    assert L.damc_sweep_stages(None) == -su.ERR_ARG
    assert L.damc_sweep_form(None, 4, su.N_STEPS) == su.FORM_NONE
    assert L.damc_sweep_workspace_bytes(None, 4, su.N_STEPS) == 0


def test_n4_width_search():
    """The widths admitted at nz = 10 are one contiguous run of multiples of 16; the next one is refused by validate()
    (the row image no longer fits), and a narrow case reports the row-resident form without a device."""
    L = _lib()
    ok = su.n4_admitted()
    w = su.n4_width()
    assert ok == list(range(16, w + 16, 16))
    # 16 rows x (kpad(20) + 8 w + max(w + pad64(w), pad64(2 w)) + 4) floats within 156 KB
    ld = lambda v: 64 + 8 * v + max(v + (v + 63) // 64 * 64, (2 * v + 63) // 64 * 64) + 4  # noqa: E731
    assert 64 * ld(w) <= 156 * 1024 < 64 * ld(w + 16), (w, ld(w), ld(w + 16))
    assert L.damc_sweep_stages(ctypes.byref(su.host_desc(10, w + 16, 16, 4))) == -su.ERR_UNSUPPORTED
    assert L.damc_sweep_form(ctypes.byref(su.host_desc(10, w, 16, 4)), 3, su.N_STEPS) == su.FORM_ROWS


def test_forced_rows_query(monkeypatch):
    """DAMC_SWEEP_ROWS=1 is read per call by both queries: a shape whose row image does not fit (W2) has no form and
    no workspace then; one that fits reports the row-resident form."""
    L = _lib()
    monkeypatch.setenv("DAMC_SWEEP_ROWS", "1")
    assert L.damc_sweep_form(ctypes.byref(_desc("W2")), 2, su.N_STEPS) == su.FORM_NONE
    assert L.damc_sweep_workspace_bytes(ctypes.byref(_desc("W2")), 2, su.N_STEPS) == 0
    for cid in ("T1", "T3", "T4", "W1"):
        assert L.damc_sweep_form(ctypes.byref(_desc(cid)), su.shape(cid)[4], su.N_STEPS) == su.FORM_ROWS


@pytest.mark.parametrize("cid", ["T1", "T5"])
def test_reference_is_the_stock_module(cid):
    """The fp32 reference against Diffusion_UnetA's stock CPU forward at each step's logsnr: the same ops on the same
    weights.  The module evaluates the sinusoidal embedding itself, step_tables on the host for the library; both are
    fp32 CPU ops, so 1e-6 rel-L2 (a few fp32 roundings of the output) bounds what may differ."""
    nz, w, nt, nx, B, res = su.shape(cid)
    m = su.unet_module(cid)
    W, I = su.weights(cid), su.inputs(cid)
    coef, temb = su.tables(su.N_STEPS, nt)
    for k in range(su.N_STEPS):
        with torch.no_grad():
            want = m(I["zt0"], su.step_logsnr(su.N_STEPS, k).expand(B).clone(), I["xemb"]).numpy()
            got = su.denoise(W, I["zt0"], temb[k], I["xemb"], res).numpy()
        d = float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))
        print("%s step %d: reference vs Diffusion_UnetA rel-L2 %.3e" % (cid, k, d))
        assert np.isfinite(got).all() and d <= 1e-6, (cid, k, d)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_references_are_finite_and_apart(cid):
    """Finite, and |fp32 - fp64| > 0 for every quantity and slice the rule is applied to: the bound is never
    0 <= 0 + 1e-6 by accident.  The end point moved away from zt0."""
    r32, r64 = su.refs(cid)
    n, B, nz = r32["eps"].shape
    assert (n, B, nz) == (su.N_STEPS, su.shape(cid)[4], su.shape(cid)[0])
    assert np.isfinite(r32["eps"]).all() and np.isfinite(r32["zt"]).all() and np.isfinite(r64["zt"]).all()
    for k in range(n):
        for label, e, e32 in su.distances(r32["eps"][k], r32["eps"][k], r64["eps"][k], su.SLICES):
            assert e32 > 0, (cid, k, label)
    for label, e, e32 in su.distances(r32["zt"], r32["zt"], r64["zt"], su.SLICES):
        assert e32 > 0, (cid, label)
    assert not np.array_equal(r32["zt"], su.inputs(cid)["zt0"].numpy())


def test_long_and_single_step_references():
    r32, r64 = su.refs("T1", su.LONG_STEPS)
    assert r32["eps"].shape[0] == su.LONG_STEPS and np.isfinite(r32["zt"]).all()
    assert su.distances(r32["zt"], r32["zt"], r64["zt"])[0][2] > 0
    for cid in ("T3", "N2"):
        s32, s64 = su.single_step_refs(cid)
        assert s32["eps"].shape[0] == 1 and np.isfinite(s32["zt"]).all()
        assert su.distances(s32["zt"], s32["zt"], s64["zt"])[0][2] > 0
