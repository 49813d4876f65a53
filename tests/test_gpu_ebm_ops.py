"""GPU: the Langevin-side EBM calls of include/damc.h called directly through ctypes with a hand-built damc_ebm_t, at
the smallest shapes that reach each of csrc/ebm.hip's three engines and each of their tails (tests/ebm_ops_util.py holds
the tables and says what each case reaches; tests/test_ebm_ops_cases_cpu.py pins them through damc_ebm_kernel):
damc_ebm_energy_grad, damc_prior_langevin_engine, damc_posterior_update, the Philox streams of the seeded chains, the
rows' independence of the batch, the refusals, and one whole posterior step against likelihood gradient + update hook.

Rule: |hip - fp64| <= 3 |torch fp32 (CPU) - fp64| + 1e-6 in rel-L2 for the whole output, its last row and its last
column; diagnostics by absolute error (ebm_ops_util.check_scalar).  Every input, weight, packed transpose and output sits
in a guarded buffer (encoder_ops_util.guarded: one quiet-NaN bit pattern in the payload, 256 bytes of it in front and
behind): a read past a weight lands in the pattern and shows as a non-finite result, a write past an output shows in
assert_guards_intact(), and neither leaves the allocation.  Run with -s for the distances
(profiles/r21/ebm_ops_parity.txt is one such run).

Measured with the two fixes these tests forced reverted (the same tests on such a library): M1, M2, M4 and M5 ran on
engine 2 instead of being refused and every z value came back NaN (M4: 4224 of 4224; the float4 run at the end of a
weight row reads the next row and, for the last row, the guard); S3 at slope -0.1 on the streaming kernels: grad_z
hip-fp64 1.1e+00 against torch32-fp64 3.1e-07, the 3-step chain 2.0e-03 against 5.9e-08, the update 5.1e-05 against
3.7e-08.
"""
import ctypes

import numpy as np
import pytest
import torch

import ebm_ops_util as E
from ebm_ops_util import assert_guards_intact, guarded, is_pattern

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_guards():
    E.reset_guards()
    yield
    E.reset_guards()


def _api(dev):
    from damc import _lib

    return _lib, _lib.lib(), _lib.stream_ptr(dev)


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _g(t, dev):
    """t in a guarded device buffer."""
    d = guarded(tuple(t.shape), dev)
    d.copy_(t)
    return d


def _bytes_are_pattern(t):
    """True when the uint8 payload t still holds the guard pattern (its length need not be a multiple of 4)."""
    want = torch.tensor(list(int(E.GUARD_WORD).to_bytes(4, "little")), dtype=torch.uint8).repeat((t.numel() + 3) // 4)
    return torch.equal(t.cpu(), want[:t.numel()])


def _ebm(dev, cid, slope):
    """The case's damc_ebm_t over guarded weights and guarded packed transposes; (descriptor, the buffers)."""
    _lib, L, stream = _api(dev)
    nz, nh, _ = E.shape(cid)
    w = {k: _g(v, dev) for k, v in E.weights(cid, slope).items()}
    w["w1t"], w["w2t"] = guarded((nz, nh), dev), guarded((nh, nh), dev)
    d = _lib.Ebm()
    d.nz, d.nh, d.slope = nz, nh, slope
    for k, v in w.items():
        setattr(d, k, v.data_ptr())
    assert L.damc_pack_ebm(ctypes.byref(d), _lib.ptr(w["w1t"]), _lib.ptr(w["w2t"]), stream) == 0
    assert_guards_intact()
    assert torch.equal(w["w1t"], w["w1"].t()) and torch.equal(w["w2t"], w["w2"].t())
    return d, w


# ------------------------------------------------------------------------------------------------ energy / gradient
def _energy_grad(dev, cid, slope, want_energy=True):
    _lib, L, stream = _api(dev)
    nz, nh, B = E.shape(cid)
    d, w = _ebm(dev, cid, slope)
    z0 = E.inputs(cid)["z"]
    z, en, gr = _g(z0, dev), guarded((B,), dev), guarded((B, nz), dev)
    rc = L.damc_ebm_energy_grad(ctypes.byref(d), _lib.ptr(z), B, _lib.ptr(en) if want_energy else None, _lib.ptr(gr),
                                stream)
    assert rc == 0, rc
    assert_guards_intact()
    assert torch.equal(z.cpu(), z0)
    return en, gr


EG_RUNS = E.runs(E.RS_IDS)


@pytest.mark.parametrize("cid,slope", EG_RUNS, ids=[E.run_id(r) for r in EG_RUNS])
def test_energy_grad_matches_fp64(gpu_device, cid, slope):
    en, gr = _energy_grad(gpu_device, cid, slope)
    r32, r64 = E.eg_refs(cid, slope)
    tag = "energy_grad %s slope %g" % (cid, slope)
    E.check(tag + " energy", _np(en), r32["energy"], r64["energy"], E.ROW_SLICES)
    E.check(tag + " grad_z", _np(gr), r32["grad"], r64["grad"], E.MAT_SLICES)


@pytest.mark.parametrize("cid", ["R7", "S3"])
def test_energy_grad_without_energy(gpu_device, cid):
    en, gr = _energy_grad(gpu_device, cid, E.SLOPE, want_energy=False)
    assert is_pattern(en)
    _, gr2 = _energy_grad(gpu_device, cid, E.SLOPE)
    assert torch.equal(gr, gr2)


# ------------------------------------------------------------------------------------------------ prior chains
def _prior(dev, cid, slope, engine, z0=None, noise="inject", seed=0, step_offset=0, chain_base=0, diag=True,
           expect=0):
    """N_STEPS prior steps of the case on `engine`; returns (z, diag) device tensors, or None after the expected
    refusal (z untouched).  noise: "inject" (the case's), a tensor to inject, "seed" (in-kernel Philox) or None."""
    _lib, L, stream = _api(dev)
    nz, nh, B = E.shape(cid)
    d, w = _ebm(dev, cid, slope)
    z0 = E.inputs(cid)["z"] if z0 is None else z0
    B = z0.shape[0]
    z = _g(z0, dev)
    nbuf = None
    if isinstance(noise, str) and noise == "inject":
        nbuf = _g(E.inputs(cid)["noise"], dev)
    elif torch.is_tensor(noise):
        nbuf = _g(noise, dev)
    dg = guarded((E.N_STEPS, 2), dev) if diag else None
    rc = L.damc_prior_langevin_engine(ctypes.byref(d), _lib.ptr(z), B, E.N_STEPS, E.PRIOR_STEP, int(noise is not None),
                                      _lib.ptr(nbuf), seed, step_offset, chain_base, _lib.ptr(dg), engine, stream)
    assert rc == expect, rc
    assert_guards_intact()
    if expect:
        assert torch.equal(z.cpu(), z0) and (dg is None or is_pattern(dg))
        return None
    return z, dg


def _check_chain(tag, cid, slope, z, dg):
    r32, r64 = E.chain_refs(cid, slope)
    E.check(tag + " z", _np(z), r32["z"], r64["z"], E.MAT_SLICES)
    E.check_scalar(tag + " diag", _np(dg), r32["diag"], r64["diag"], r64["dterms"])


ENGINE1_RUNS = E.runs(E.RS_IDS + E.M_IDS)


@pytest.mark.parametrize("cid,slope", ENGINE1_RUNS, ids=[E.run_id(r) for r in ENGINE1_RUNS])
def test_prior_chain_engine1_matches_fp64(gpu_device, cid, slope):
    z, dg = _prior(gpu_device, cid, slope, 1)
    _check_chain("prior engine 1 (kernel %d) %s slope %g" % (E.KERNELS[cid][1], cid, slope), cid, slope, z, dg)


ENGINE2_RUNS = E.runs(E.M_IDS)


@pytest.mark.parametrize("cid,slope", ENGINE2_RUNS, ids=[E.run_id(r) for r in ENGINE2_RUNS])
def test_prior_chain_engine2_matches_fp64_or_is_refused(gpu_device, cid, slope):
    """The table, not the library, says which M cases engine 2 refuses (nh % 4 != 0: M1, M2, M4, M5)."""
    if E.KERNELS[cid][2] == E.KERNEL_NONE:
        assert E.shape(cid)[1] % 4 != 0
        assert _prior(gpu_device, cid, slope, 2, expect=E.ERR_UNSUPPORTED) is None
        return
    z, dg = _prior(gpu_device, cid, slope, 2)
    _check_chain("prior engine 2 %s slope %g" % (cid, slope), cid, slope, z, dg)
    z1, _ = _prior(gpu_device, cid, slope, 1)
    r32, r64 = E.chain_refs(cid, slope)
    E.check_pair("prior engine 2 - engine 1 %s slope %g" % (cid, slope), _np(z), _np(z1), r32["z"], r64["z"])


def test_engine0_takes_the_batch_s_engine(gpu_device):
    """Engine 0 below the MFMA threshold is engine 1, bit for bit."""
    z0, _ = _prior(gpu_device, "M3", E.SLOPE, 0)
    z1, _ = _prior(gpu_device, "M3", E.SLOPE, 1)
    assert torch.equal(z0, z1)


# ------------------------------------------------------------------------------------------------ Philox streams
# nz in {3, 65, 130, 144}: quads picked at nz % 4 != 0, on each engine 1 kernel; M9 and M3 on the MFMA engine
PHILOX_RUNS = [("R2", 1), ("R5", 1), ("S4", 1), ("M5", 1), ("M9", 2), ("M3", 2)]


@pytest.mark.parametrize("cid,engine", PHILOX_RUNS, ids=["%s-engine%d" % r for r in PHILOX_RUNS])
def test_seeded_chain_is_the_injected_philox_chain(gpu_device, cid, engine):
    _lib, L, stream = _api(gpu_device)
    nz, nh, B = E.shape(cid)
    assert (cid, nz) in (("R2", 3), ("R5", 65), ("S4", 130), ("M5", 144), ("M9", 144), ("M3", 48))
    seed, off, base = 0x1234567, 7, 100
    xi = guarded((E.N_STEPS, B, nz), gpu_device)
    assert L.damc_philox_normal(_lib.ptr(xi), E.N_STEPS, B, nz, seed, off, base, E.STREAM_PRIOR, stream) == 0
    assert_guards_intact()
    xi = xi.cpu()
    assert bool(torch.isfinite(xi).all())
    zs, _ = _prior(gpu_device, cid, E.SLOPE, engine, noise="seed", seed=seed, step_offset=off, chain_base=base)
    zi, _ = _prior(gpu_device, cid, E.SLOPE, engine, noise=xi)
    assert torch.equal(zs, zi)
    zn, _ = _prior(gpu_device, cid, E.SLOPE, engine, noise=None)
    assert not torch.equal(zs, zn)


# ------------------------------------------------------------------------------------------------ posterior update
def _post(dev, cid, slope, nslab=1, noise="inject", use_ebm=True, z0=None, seed=0, step_index=0, chain_base=0,
          slabs=None, expect=0):
    """One damc_posterior_update of the case; returns (z, diag, limbs, limbs_written)."""
    _lib, L, stream = _api(dev)
    nz, nh, B = E.shape(cid)
    d = None
    if use_ebm:
        d, w = _ebm(dev, cid, slope)
    z0 = E.inputs(cid)["z"] if z0 is None else z0
    B = z0.shape[0]
    n = B * nz
    sl = E.inputs(cid, nslab)["slabs"] if slabs is None else slabs
    stride = n + 5 if nslab > 1 else n  # the gaps between slabs keep the NaN pattern: nothing may read them
    sbuf = guarded((nslab, stride), dev)
    sbuf[:, :n] = sl.reshape(nslab, n).to(dev)
    z = _g(z0, dev)
    nbuf = _g(E.inputs(cid)["noise"][0], dev) if isinstance(noise, str) and noise == "inject" else None
    dg = guarded((4,), dev)
    limbs = guarded(B * nz * 6, dev)
    wrote = ctypes.c_int(-1)
    rc = L.damc_posterior_update(ctypes.byref(d) if d is not None else None, _lib.ptr(z), _lib.ptr(sbuf), nslab, stride,
                                 B, nz, E.POST_STEP, int(noise is not None), _lib.ptr(nbuf), seed, step_index,
                                 chain_base, _lib.ptr(dg), _lib.ptr(limbs), ctypes.byref(wrote), stream)
    assert rc == expect, rc
    assert_guards_intact()
    if expect:
        assert torch.equal(z.cpu(), z0) and is_pattern(dg) and wrote.value == 0
        return None
    return z, dg, limbs, wrote.value


def _check_post(tag, cid, slope, res, nslab=1, with_noise=True, use_ebm=True):
    z, dg, limbs, wrote = res
    nz, nh, B = E.shape(cid)
    r32, r64 = E.post_refs(cid, slope, nslab, with_noise, use_ebm)
    E.check(tag + " z", _np(z), r32["z"], r64["z"], E.MAT_SLICES)
    E.check_scalar(tag + " diag", _np(dg), r32["diag"], r64["diag"], r64["dterms"])
    assert _np(dg)[1] == 0.0
    # the limbs: written by the register-resident kernel at nz % 8 == 0 alone, and then bit-exact limbs of the new z
    kernel = E.KERNELS[cid][0] if use_ebm else E.KERNEL_STREAM
    assert wrote == int(kernel == E.KERNEL_REG and nz % 8 == 0), (wrote, kernel, nz)
    if wrote:
        got = limbs.view(torch.int16).reshape(B, nz // 8, 3, 8).cpu()
        assert torch.equal(got, E.limbs_of(z.cpu()))
    else:
        assert _bytes_are_pattern(limbs)


POST_RUNS = E.runs(E.RS_IDS)


@pytest.mark.parametrize("cid,slope", POST_RUNS, ids=[E.run_id(r) for r in POST_RUNS])
def test_posterior_update_matches_fp64(gpu_device, cid, slope):
    res = _post(gpu_device, cid, slope)
    _check_post("posterior_update (kernel %d) %s slope %g" % (E.KERNELS[cid][0], cid, slope), cid, slope, res)


def test_posterior_update_writes_limbs_where_the_table_says():
    assert [c for c in E.RS_IDS if E.KERNELS[c][0] == E.KERNEL_REG and E.shape(c)[0] % 8 == 0] == ["R4", "R6"]


@pytest.mark.parametrize("cid", ["R7", "S3", "S2"])
def test_posterior_update_without_ebm_streams(gpu_device, cid):
    for noise in ("inject", None):
        res = _post(gpu_device, cid, E.SLOPE, noise=noise, use_ebm=False)
        _check_post("posterior_update no ebm %s noise %d" % (cid, noise is not None), cid, E.SLOPE, res,
                    with_noise=noise is not None, use_ebm=False)


SLAB_RUNS = [(c, n) for c in ("R7", "S3") for n in (1, 2, 15, 16, 17, 33)]


@pytest.mark.parametrize("cid,nslab", SLAB_RUNS, ids=["%s-%d" % r for r in SLAB_RUNS])
def test_posterior_update_sums_the_slabs(gpu_device, cid, nslab):
    """Without noise (the one-slab runs above inject it); 15 / 16 / 17 and 33 straddle the register kernel's 16 slab
    groups (a group of one, of two, of three slabs)."""
    res = _post(gpu_device, cid, E.SLOPE, nslab=nslab, noise=None)
    _check_post("posterior_update %s nslab %d" % (cid, nslab), cid, E.SLOPE, res, nslab=nslab, with_noise=False)


@pytest.mark.parametrize("cid", ["R4", "S3"])
def test_posterior_update_seeded_noise_is_the_posterior_stream(gpu_device, cid):
    _lib, L, stream = _api(gpu_device)
    nz, nh, B = E.shape(cid)
    seed, idx, base = 0x7654321, 7, 100
    xi = guarded((1, B, nz), gpu_device)
    assert L.damc_philox_normal(_lib.ptr(xi), 1, B, nz, seed, idx, base, E.STREAM_POSTERIOR, stream) == 0
    seeded = _post(gpu_device, cid, E.SLOPE, noise="seed", seed=seed, step_index=idx, chain_base=base)
    r32, r64 = E.post_refs(cid, E.SLOPE, 1, False)
    c, x0 = np.float32(E.POST_STEP), xi[0].cpu().numpy()
    want32, want64 = r32["z"] + c * x0, r64["z"] + float(c) * x0.astype(np.float64)
    E.check("posterior_update seeded %s z" % cid, _np(seeded[0]), want32, want64, E.MAT_SLICES)
    # bitwise the injected call fed the drawn values
    zi = _post_with_noise(gpu_device, cid, xi[0].cpu())
    assert torch.equal(seeded[0], zi)


def _post_with_noise(dev, cid, xi):
    """_post with `xi` (B, nz) injected instead of the case's noise."""
    _lib, L, stream = _api(dev)
    nz, nh, B = E.shape(cid)
    d, w = _ebm(dev, cid, E.SLOPE)
    z, sbuf, nbuf = _g(E.inputs(cid)["z"], dev), _g(E.inputs(cid)["slabs"][0], dev), _g(xi, dev)
    wrote = ctypes.c_int(-1)
    rc = L.damc_posterior_update(ctypes.byref(d), _lib.ptr(z), _lib.ptr(sbuf), 1, B * nz, B, nz, E.POST_STEP, 1,
                                 _lib.ptr(nbuf), 0, 0, 0, None, None, ctypes.byref(wrote), stream)
    assert rc == 0 and wrote.value == 0
    assert_guards_intact()
    return z


# ------------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("cid,engine", [("R7", 1), ("S3", 1), ("M3", 2)], ids=["reg", "streaming", "mfma"])
def test_prior_rows_do_not_depend_on_the_batch(gpu_device, cid, engine):
    """B = 5 cut as [0:3] + [3:5] with chain_base set: bit for bit the unsharded z (seeded noise).  The odd cut makes the
    streaming kernel pair the rows differently and the MFMA tile hold them at other tile rows."""
    from damc import synth

    nz = E.shape(cid)[0]
    z0 = torch.from_numpy(synth.normal_f32(4242, nz, (5, nz)))
    kw = dict(noise="seed", seed=99, step_offset=3, diag=False)
    full, _ = _prior(gpu_device, cid, E.SLOPE, engine, z0=z0, chain_base=100, **kw)
    a, _ = _prior(gpu_device, cid, E.SLOPE, engine, z0=z0[0:3].contiguous(), chain_base=100, **kw)
    b, _ = _prior(gpu_device, cid, E.SLOPE, engine, z0=z0[3:5].contiguous(), chain_base=103, **kw)
    assert torch.equal(full, torch.cat([a, b]))
    assert not torch.equal(full[3:5], _prior(gpu_device, cid, E.SLOPE, engine, z0=z0[3:5].contiguous(),
                                             chain_base=100, **kw)[0])


@pytest.mark.parametrize("cid", ["R7", "S3"], ids=["reg", "streaming"])
def test_posterior_update_rows_do_not_depend_on_the_batch(gpu_device, cid):
    from damc import synth

    nz = E.shape(cid)[0]
    z0 = torch.from_numpy(synth.normal_f32(4243, nz, (5, nz)))
    gl = torch.from_numpy(synth.normal_f32(4244, nz, (1, 5, nz)))
    kw = dict(noise="seed", seed=98, step_index=3)
    full = _post(gpu_device, cid, E.SLOPE, z0=z0, slabs=gl, chain_base=100, **kw)[0]
    a = _post(gpu_device, cid, E.SLOPE, z0=z0[0:3].contiguous(), slabs=gl[:, 0:3].contiguous(), chain_base=100, **kw)[0]
    b = _post(gpu_device, cid, E.SLOPE, z0=z0[3:5].contiguous(), slabs=gl[:, 3:5].contiguous(), chain_base=103, **kw)[0]
    assert torch.equal(full, torch.cat([a, b]))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_z_untouched(gpu_device):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    # a shape with no kernel: one nh past S6 (the weights are real, so a missed refusal stays inside its buffers)
    nz, nh, B = E.shape("S6")
    nh += 1
    assert L.damc_ebm_kernel(nz, nh, -1, B) == L.damc_ebm_kernel(nz, nh, 1, B) == E.KERNEL_NONE
    w = dict(w1=guarded((nh, nz), gpu_device), b1=guarded((nh,), gpu_device), w2=guarded((nh, nh), gpu_device),
             b2=guarded((nh,), gpu_device), w3=guarded((nh,), gpu_device), b3=guarded((1,), gpu_device),
             w1t=guarded((nz, nh), gpu_device), w2t=guarded((nh, nh), gpu_device))
    d = _lib.Ebm()
    d.nz, d.nh, d.slope = nz, nh, E.SLOPE
    for k, v in w.items():
        v.zero_()
        setattr(d, k, v.data_ptr())
    z0 = E.inputs("S6")["z"]
    z, g, en, gr = _g(z0, gpu_device), _g(z0, gpu_device), guarded((B,), gpu_device), guarded((B, nz), gpu_device)
    dg = guarded((6,), gpu_device)
    wrote = ctypes.c_int(5)
    U, A = E.ERR_UNSUPPORTED, E.ERR_ARG
    assert L.damc_ebm_energy_grad(ctypes.byref(d), ptr(z), B, ptr(en), ptr(gr), stream) == U
    assert L.damc_prior_langevin_engine(ctypes.byref(d), ptr(z), B, 3, 0.4, 0, None, 0, 0, 0, None, 1, stream) == U
    assert L.damc_prior_langevin_engine(ctypes.byref(d), ptr(z), B, 3, 0.4, 0, None, 0, 0, 0, None, 0, stream) == U
    assert L.damc_posterior_update(ctypes.byref(d), ptr(z), ptr(g), 1, B * nz, B, nz, 0.1, 0, None, 0, 0, 0, ptr(dg),
                                   None, ctypes.byref(wrote), stream) == U
    assert wrote.value == 0
    # NULL arguments
    assert L.damc_ebm_energy_grad(None, ptr(z), B, ptr(en), ptr(gr), stream) == A
    assert L.damc_ebm_energy_grad(ctypes.byref(d), None, B, ptr(en), ptr(gr), stream) == A
    assert L.damc_ebm_energy_grad(ctypes.byref(d), ptr(z), B, ptr(en), None, stream) == A
    assert L.damc_prior_langevin_engine(None, ptr(z), B, 3, 0.4, 0, None, 0, 0, 0, None, 1, stream) == A
    assert L.damc_prior_langevin_engine(ctypes.byref(d), None, B, 3, 0.4, 0, None, 0, 0, 0, None, 1, stream) == A
    assert L.damc_prior_langevin_engine(ctypes.byref(d), ptr(z), B, 3, 0.4, 0, None, 0, 0, 0, None, 3, stream) == A
    assert L.damc_posterior_update(None, None, ptr(g), 1, B * nz, B, nz, 0.1, 0, None, 0, 0, 0, ptr(dg), None,
                                   ctypes.byref(wrote), stream) == A
    assert L.damc_posterior_update(None, ptr(z), None, 1, B * nz, B, nz, 0.1, 0, None, 0, 0, 0, ptr(dg), None,
                                   ctypes.byref(wrote), stream) == A
    assert L.damc_posterior_update(None, ptr(z), ptr(g), 1, B * nz, B, nz, 0.1, 0, None, 0, 0, 0, ptr(dg), None, None,
                                   stream) == A
    assert L.damc_posterior_update(None, ptr(z), ptr(g), 2, B * nz - 1, B, nz, 0.1, 0, None, 0, 0, 0, ptr(dg), None,
                                   ctypes.byref(wrote), stream) == A
    assert_guards_intact()
    assert torch.equal(z.cpu(), z0) and is_pattern(en) and is_pattern(gr) and is_pattern(dg)


def test_engine2_refuses_nz_33(gpu_device):
    """nz = 33 on engine 2 (and nh = 201 at nz = 128, through the M4 run above): refused, z untouched."""
    _lib, L, stream = _api(gpu_device)
    d, w = _ebm(gpu_device, "R4", E.SLOPE)   # real 64 x 64 weights; the descriptor then claims nz = 33
    d.nz = 33
    z0 = torch.from_numpy(np.arange(2 * 33, dtype=np.float32).reshape(2, 33))
    z = _g(z0, gpu_device)
    assert L.damc_ebm_kernel(33, 64, 2, 2) == E.KERNEL_NONE and L.damc_ebm_kernel(32, 64, 2, 2) == E.KERNEL_MFMA
    rc = L.damc_prior_langevin_engine(ctypes.byref(d), _lib.ptr(z), 2, 3, 0.4, 0, None, 0, 0, 0, None, 2, stream)
    assert rc == E.ERR_UNSUPPORTED
    assert_guards_intact()
    assert torch.equal(z.cpu(), z0)


# ------------------------------------------------------------------------------------------------ the whole step
@pytest.mark.parametrize("ndf", [13, 209])
def test_posterior_step_is_likelihood_grad_then_update_hook(gpu_device, ndf):
    """One damc_posterior_langevin step (n_steps = 1, seeded noise) equals damc_likelihood_grad followed by
    damc_posterior_update: z bit for bit, and the diagnostics' EBM, |z|^2 and gradient terms up to the order of their
    atomic adds: the hook launches what the step launches.  ndf = 13: the register-resident update (fused slab sum
    inside the step); 209: the streaming one."""
    from damc import synth
    from damc.plans import ebm_plan, generator_plan
    from src import diffusion_net as dn

    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, nz, sigma, step = 3, 16, 0.3, 0.1
    G = synth.load_into(dn._netG_mnist(nz=nz, ngf=2, nc=1), 0).to(gpu_device).eval()
    Enet = synth.load_into(dn._netE(nz, ndf), 10).to(gpu_device).eval()
    assert L.damc_ebm_kernel(nz, ndf, -1, B) == (E.KERNEL_REG if ndf == 13 else E.KERNEL_STREAM)
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 1, 28, 28))).to(gpu_device)
    z0 = torch.from_numpy(synth.normal_f32(2, 0, (B, nz)))
    gp, ep = generator_plan(G), ebm_plan(Enet)
    gd, ed = gp.refresh(gpu_device), ep.refresh(gpu_device)
    ws, nbytes = gp.workspace(B)
    seed, off, base = 31337, 5, 9
    za, da = _g(z0, gpu_device), guarded((4,), gpu_device)
    rc = L.damc_posterior_langevin(ctypes.byref(gd), ctypes.byref(ed), ptr(za), ptr(x), B, 1, sigma, step, 1, None, seed,
                                   off, base, ptr(da), ptr(ws), nbytes, stream)
    assert rc == 0, rc
    zb, gl, db = _g(z0, gpu_device), guarded((B, nz), gpu_device), guarded((4,), gpu_device)
    rc = L.damc_likelihood_grad(ctypes.byref(gd), ptr(zb), ptr(x), B, sigma, ptr(gl), ptr(ws), nbytes, stream)
    assert rc == 0, rc
    wrote = ctypes.c_int(-1)
    rc = L.damc_posterior_update(ctypes.byref(ed), ptr(zb), ptr(gl), 1, B * nz, B, nz, step, 1, None, seed, off, base,
                                 ptr(db), None, ctypes.byref(wrote), stream)
    assert rc == 0 and wrote.value == 0
    assert_guards_intact()
    assert torch.equal(za, zb)
    assert not torch.equal(za.cpu(), z0)
    # the diagnostics are atomic adds of the workgroups' sums in arrival order: equal up to that reordering
    da, db = _np(da), _np(db)
    assert np.allclose(da[[0, 2, 3]], db[[0, 2, 3]], rtol=1e-6, atol=1e-6) and db[1] == 0.0 and da[1] > 0.0


# ------------------------------------------------------------------------------------------------ damc.langevin
def test_injected_noise_may_be_longer_on_every_path(gpu_device):
    """damc.langevin takes the first n_steps * B * nz values of a longer injected buffer on the per-step (train-mode
    spectral norm) paths as on the one-call paths: a buffer one row too long gives the exact buffer's z."""
    import copy

    from damc import langevin as lv
    from damc import synth
    from src import diffusion_net as dn

    B, nz, n = 3, 16, 2
    z0 = torch.from_numpy(synth.normal_f32(2, 0, (B, nz))).to(gpu_device)
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 1, 28, 28))).to(gpu_device)
    exact = torch.from_numpy(synth.normal_f32(3, 0, (n * B, nz))).to(gpu_device)
    longer = torch.cat([exact, torch.full((1, nz), float("nan"), device=gpu_device)]).contiguous()
    G = synth.load_into(dn._netG_mnist(nz=nz, ngf=2, nc=1), 0).to(gpu_device).eval()
    for sn in (False, True):
        E0 = synth.load_into(dn._netE(nz, 13, e_sn=sn), 10).to(gpu_device)
        E0 = E0.train() if sn else E0.eval()
        out = {}
        for tag, buf in (("exact", exact), ("longer", longer)):
            Ea, Eb = copy.deepcopy(E0), copy.deepcopy(E0)
            zp, zq = z0.clone(), z0.clone()
            lv.prior_langevin(zp, Ea, n, 0.4, True, noise=buf)
            lv.posterior_langevin(zq, x, G, Eb, n, 0.3, 0.1, True, noise=buf)
            out[tag] = (zp, zq)
        assert torch.equal(out["exact"][0], out["longer"][0]) and torch.equal(out["exact"][1], out["longer"][1])
        assert bool(torch.isfinite(out["longer"][0]).all()) and bool(torch.isfinite(out["longer"][1]).all())
