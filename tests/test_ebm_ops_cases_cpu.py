"""CPU: the case tables of tests/ebm_ops_util.py hold what tests/test_gpu_ebm_ops.py relies on.

  * through damc_ebm_kernel (host only: the function the entry points dispatch through), every case reaches the kernel
    its row names, and each boundary pair falls on its side;
  * no fp64 pre-activation of any case, at either layer, at any step of its chain and at any of its slopes, comes within
    KINK_REL of the LeakyReLU kink, so the GPU comparison needs no exclusion logic;
  * the fp32 reference is finite and within 1e-4 of fp64 on its own, so the bound's yardstick is sound;
  * the host-side refusals of damc_posterior_update (every one returns before a launch; no address is dereferenced).
"""
import ctypes

import numpy as np
import pytest

import ebm_ops_util as E


def _L():
    from damc import _lib

    return _lib, _lib.lib()


ALL_RUNS = E.runs(list(E.CASES))


# ------------------------------------------------------------------------------------------------ reachability
@pytest.mark.parametrize("cid", list(E.CASES))
def test_case_reaches_the_kernel_its_row_names(cid):
    _, L = _L()
    nz, nh, B = E.shape(cid)
    hook, eng1, eng2 = E.KERNELS[cid]
    assert L.damc_ebm_kernel(nz, nh, -1, B) == hook
    assert L.damc_ebm_kernel(nz, nh, 1, B) == eng1
    assert L.damc_ebm_kernel(nz, nh, 2, B) == eng2
    # engine 0 below the MFMA threshold is engine 1; from it up, engine 2 where that engine takes the shape
    nmin = L.damc_ebm_mfma_min_chains()
    assert B < nmin
    assert L.damc_ebm_kernel(nz, nh, 0, B) == eng1
    assert L.damc_ebm_kernel(nz, nh, 0, nmin) == (eng2 or eng1)
    if cid[0] == "R":
        assert hook == eng1 == E.KERNEL_REG
    if cid[0] == "S":
        assert hook == eng1 == E.KERNEL_STREAM
    if cid[0] == "M":
        assert eng2 == (E.KERNEL_MFMA if nh % 4 == 0 else E.KERNEL_NONE)


def test_table_is_the_issue_s():
    assert E.R_CASES == dict(R1=(1, 1, 1), R2=(3, 13, 2), R3=(63, 14, 3), R4=(64, 64, 5), R5=(65, 207, 2),
                             R6=(128, 208, 3), R7=(100, 200, 4))
    assert [E.shape(c) for c in ("S1", "S2", "S3", "S4", "S5")] == [(128, 209, 3), (129, 208, 3), (132, 212, 5),
                                                                    (130, 256, 2), (2, 760, 3)]
    assert [E.shape(c) for c in ("M1", "M2", "M3", "M4", "M5", "M6")] == [(16, 1, 1), (16, 17, 15), (48, 200, 17),
                                                                          (128, 201, 33), (144, 202, 3), (256, 256, 16)]
    assert E.SLOPE_CASES == ("R4", "S3", "M3") and E.EXTRA_SLOPES == (0.0, -0.1) and E.SLOPE == 0.2
    assert max(B for _, _, B in map(E.shape, E.CASES)) <= 33 and E.N_STEPS == 3


def test_boundary_pairs():
    _, L = _L()
    k = L.damc_ebm_kernel
    for eng in (-1, 1):
        assert k(128, 208, eng, 3) == E.KERNEL_REG and k(128, 209, eng, 3) == E.KERNEL_STREAM
        assert k(129, 208, eng, 3) == E.KERNEL_STREAM
    # the LDS limit of the streaming kernels at nz = 2: R = 2 rows of 2 nz + 4 nh floats, 32 and the k-group partials
    nh = E.s6_nh()
    assert E.shape("S6") == (2, nh, 1)
    floats = lambda n: 2 * 2 * 2 + 2 * n * 4 + 32 + 2 * (4 * 1024 + 4 * 256)  # noqa: E731
    assert 4 * floats(nh) <= 65536 < 4 * floats(nh + 1)
    for eng in (-1, 0, 1):
        assert k(2, nh, eng, 1) == E.KERNEL_STREAM and k(2, nh + 1, eng, 1) == E.KERNEL_NONE
    # engine 2: nz % 16, nh % 4, both <= 256
    assert k(32, 200, 2, 2) == E.KERNEL_MFMA and k(33, 200, 2, 2) == E.KERNEL_NONE
    assert k(128, 200, 2, 2) == E.KERNEL_MFMA and k(128, 201, 2, 2) == E.KERNEL_NONE
    assert k(256, 256, 2, 2) == E.KERNEL_MFMA and k(272, 256, 2, 2) == k(256, 260, 2, 2) == E.KERNEL_NONE
    # engine 0 falls to the VALU kernels where the MFMA tile does not take the shape, at any batch
    nmin = L.damc_ebm_mfma_min_chains()
    assert k(128, 200, 0, nmin - 1) == E.KERNEL_REG and k(128, 200, 0, nmin) == E.KERNEL_MFMA
    assert k(128, 201, 0, nmin) == E.KERNEL_REG and k(144, 202, 0, nmin) == E.KERNEL_STREAM
    # the update without an EBM streams at every nz; nothing else takes nh = 0, and no engine past 2 exists
    assert k(100, 0, -1, 4) == k(1024, 0, -1, 4) == E.KERNEL_STREAM and k(1025, 0, -1, 4) == E.KERNEL_NONE
    assert k(100, 0, 1, 4) == k(16, 0, 2, 4) == k(0, 8, 1, 4) == k(16, 8, 3, 4) == k(16, 8, -2, 4) == E.KERNEL_NONE


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("cid,slope", ALL_RUNS, ids=[E.run_id(r) for r in ALL_RUNS])
def test_reference_stays_clear_of_the_kink(cid, slope):
    """Every step of the noisy chain and of the noise-free one (the posterior update and the energy / gradient call
    evaluate E at the chain's first z)."""
    for with_noise in (True, False):
        m = E.kink_margin(E.chain_refs(cid, slope, with_noise)[1]["pre"])
        print("%s slope %g noise %d kink margin %.3e" % (cid, slope, with_noise, m))
        assert m >= E.KINK_REL, (cid, slope, m)
    assert E.kink_margin(E.eg_refs(cid, slope)[1]["pre"]) >= E.KINK_REL


@pytest.mark.parametrize("cid,slope", ALL_RUNS, ids=[E.run_id(r) for r in ALL_RUNS])
def test_fp32_reference_is_a_sound_yardstick(cid, slope):
    refs = [("eg", E.eg_refs(cid, slope), ("energy", "grad")), ("chain", E.chain_refs(cid, slope), ("z", "diag")),
            ("post", E.post_refs(cid, slope), ("z", "diag")),
            ("post no ebm", E.post_refs(cid, slope, use_ebm=False), ("z", "diag"))]
    for tag, (r32, r64), names in refs:
        for n in names:
            assert np.isfinite(r32[n]).all() and np.isfinite(r64[n]).all()
            slices = E.MAT_SLICES if r64[n].ndim == 2 and n != "diag" else ()
            for label, e, e32 in E.report("%s %s %g %s" % (cid, tag, slope, n), r32[n], r32[n], r64[n], slices):
                assert e32 < 1e-4, (cid, tag, n, label, e32)


def test_slopes_change_the_reference():
    """The three slopes are three different functions at the slope cases (a test at 0.0 or -0.1 is not the 0.2 one)."""
    for cid in E.SLOPE_CASES:
        g = [E.eg_refs(cid, s)[1]["grad"] for s in E.slopes_of(cid)]
        assert not np.allclose(g[0], g[1]) and not np.allclose(g[1], g[2]) and not np.allclose(g[0], g[2])


def test_limbs_of_is_the_octet_layout():
    import torch

    z = torch.tensor([[1.0 + 2.0 ** -9 + 2.0 ** -18] * 8 + [-3.0] * 8])
    w = E.limbs_of(z)
    assert tuple(w.shape) == (1, 2, 3, 8)
    f = w.view(torch.bfloat16).float()
    assert torch.equal(f[0, 0, 0], torch.full((8,), 1.0)) and torch.equal(f[0, 0, 1], torch.full((8,), 2.0 ** -9))
    assert torch.equal(f[0, 0, 2], torch.full((8,), 2.0 ** -18))
    assert torch.equal(f[0, 1, 0], torch.full((8,), -3.0)) and not f[0, 1, 1:].any()


# ------------------------------------------------------------------------------------------------ host refusals
def _desc(nz, nh, fake=0x1000):
    _lib, _ = _L()
    d = _lib.Ebm()
    d.nz, d.nh, d.slope = nz, nh, 0.2
    for k in ("w1", "b1", "w2", "b2", "w3", "b3", "w1t", "w2t"):
        setattr(d, k, fake)
    return d


def test_posterior_update_refuses_on_the_host():
    """Fake addresses throughout: each of these calls has to return before it launches or reads anything."""
    _lib, L = _L()
    P = ctypes.c_void_p
    z, g = P(0x1000), P(0x2000)
    wrote = ctypes.c_int(7)

    def call(ebm=None, z=z, g=g, nslab=1, stride=400, B=4, nz=100, wrote=wrote):
        return L.damc_posterior_update(ctypes.byref(ebm) if ebm is not None else None, z, g, nslab, stride, B, nz, 0.1,
                                       0, None, 0, 0, 0, None, None, ctypes.byref(wrote) if wrote is not None else None,
                                       None)

    assert call(z=None) == E.ERR_ARG and wrote.value == 0
    wrote.value = 7
    assert call(g=None) == E.ERR_ARG and wrote.value == 0
    assert call(wrote=None) == E.ERR_ARG
    assert call(B=0) == E.ERR_ARG and call(nz=0) == E.ERR_ARG and call(nslab=0) == E.ERR_ARG
    assert call(nslab=2, stride=399) == E.ERR_ARG
    assert call(ebm=_desc(64, 200)) == E.ERR_ARG            # the EBM's nz is not the update's
    assert call(ebm=_desc(100, 0)) == E.ERR_ARG
    d = _desc(100, 200)
    d.w2t = None
    assert call(ebm=d) == E.ERR_ARG
    assert call(nz=1025, stride=4100) == E.ERR_UNSUPPORTED   # no kernel without an EBM
    nh = E.s6_nh()
    assert call(ebm=_desc(2, nh + 1), nz=2, stride=8) == E.ERR_UNSUPPORTED


def test_prior_and_energy_grad_refuse_on_the_host():
    _lib, L = _L()
    P = ctypes.c_void_p
    nh = E.s6_nh()
    d = _desc(2, nh + 1)
    assert L.damc_ebm_energy_grad(ctypes.byref(d), P(0x1000), 1, None, P(0x2000), None) == E.ERR_UNSUPPORTED
    assert L.damc_prior_langevin_engine(ctypes.byref(d), P(0x1000), 1, 3, 0.4, 0, None, 0, 0, 0, None, 1,
                                        None) == E.ERR_UNSUPPORTED
    for nz_, nh_ in ((33, 200), (128, 201), (144, 202), (16, 1)):
        d = _desc(nz_, nh_)
        assert L.damc_prior_langevin_engine(ctypes.byref(d), P(0x1000), 1, 3, 0.4, 0, None, 0, 0, 0, None, 2,
                                            None) == E.ERR_UNSUPPORTED, (nz_, nh_)
    d = _desc(16, 0)
    assert L.damc_ebm_energy_grad(ctypes.byref(d), P(0x1000), 1, None, P(0x2000), None) == E.ERR_ARG
