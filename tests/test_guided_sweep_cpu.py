"""CPU: the guided sweep's entry points (include/damc.h), their host-side shape and argument logic (no device work),
and the toy's refusal of cond_w > 0."""
import ctypes

import pytest

from test_toyq_cpu import _toy_desc
from toyq_util import build_toy_case


def _cifar_desc():
    """The CIFAR amortizer's denoiser: nz 128, nf 4 (w = 128), nxemb 1024, ntemb 128, placeholder pointers."""
    return _toy_desc(128, w=128, ntemb=128, nxemb=1024)


def test_symbols_are_exported_and_bound():
    from damc import _lib

    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("damc_guided_sweep_workspace_bytes", "damc_guided_sweep"):
        assert hasattr(so, name), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib.lib().damc_abi_version() == 3  # additive


def test_workspace_bytes_host_only(monkeypatch):
    from damc import _lib

    L = _lib.lib()
    monkeypatch.delenv("DAMC_SWEEP_ROWS", raising=False)
    gws = lambda d, B=128, n=100: int(L.damc_guided_sweep_workspace_bytes(ctypes.byref(d), B, n))  # noqa: E731
    ws = lambda d, B=128, n=100: int(L.damc_sweep_workspace_bytes(ctypes.byref(d), B, n))  # noqa: E731
    d = _cifar_desc()
    assert gws(d) > 0
    assert gws(d) > ws(d)
    # the unconditional planes: 4 S floats per (step, row), S = 128 + 4 * 256 + 128 + 128
    assert gws(d) - ws(d) >= 4 * 1408 * 4 * 128 * 100
    assert gws(d, 21, 5) > ws(d, 21, 5)
    assert gws(_toy_desc(6)) == 0           # nz % 4 != 0
    assert gws(_toy_desc(2)) == 0           # the toy
    assert gws(_toy_desc(128, w=256)) == 0  # the 16-row LDS image must fit the CU
    assert gws(d, 0, 100) == 0
    assert gws(d, 128, 0) == 0


def test_argument_errors_host_only():
    from damc import _lib

    L = _lib.lib()
    d = _cifar_desc()
    fake = ctypes.c_void_p(256)
    base = dict(xemb=fake, xemb_unc=fake, w=0.5, zt=fake, B=8, n=5, temb=fake, coef=fake)

    def call(desc=d, **kw):
        a = dict(base, **kw)
        return L.damc_guided_sweep(ctypes.byref(desc), a["xemb"], a["xemb_unc"], a["w"], a["zt"], a["B"], a["n"],
                                   a["temb"], a["coef"], 1, None, 0, 0, None, 0, fake, 1 << 40, None)

    for k in ("xemb", "xemb_unc", "zt", "temb", "coef"):
        assert call(**{k: None}) == _lib.DAMC_ERR_ARG, k
    assert call(B=0) == _lib.DAMC_ERR_ARG
    assert call(B=-3) == _lib.DAMC_ERR_ARG
    assert call(n=0) == _lib.DAMC_ERR_ARG
    assert call(w=0.0) == _lib.DAMC_ERR_ARG
    assert call(w=-0.5) == _lib.DAMC_ERR_ARG
    assert call(w=float("nan")) == _lib.DAMC_ERR_ARG
    # where the workspace size is 0 the sweep is unsupported
    assert call(desc=_toy_desc(6)) == _lib.DAMC_ERR_UNSUPPORTED
    assert call(desc=_toy_desc(2)) == _lib.DAMC_ERR_UNSUPPORTED
    assert call(desc=_toy_desc(128, w=256)) == _lib.DAMC_ERR_UNSUPPORTED


def test_toy_guidance_is_still_refused():
    """cond_w > 0 on a toy Q (nz = 2): NotImplementedError before any device work, with or without a seed."""
    c = build_toy_case("q_toy")
    with pytest.raises(NotImplementedError) as e:
        c["Q"](c["x"], cond_w=0.5)
    assert "training kernels" not in str(e.value)
    from damc import amortizer

    with pytest.raises(NotImplementedError):
        amortizer.q_forward(c["Q"], x=c["x"], cond_w=0.5, seed=3)
