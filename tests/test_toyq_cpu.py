"""CPU: the toy amortizer's drop-in class, its goldens against the fp64 oracle, and the host-side shape logic of the
row-resident sweep and the fused MLP (no device work)."""
import ctypes

import pytest

from conftest import load_golden, rel_l2
from toyq_util import TOY_NAMES, build_toy_case, toy_fp64


def test_dropin_state_dict_matches_reference():
    """state_dict keys, order and shapes of _netQ_U_toy at the defaults equal the reference's recorded list
    (workspace/toy_example/src/diffusion_net.py:141-186): xemb, encoder.{0,2,4,6}.*, p.*, prior_emb.{0,2}.*."""
    from src import diffusion_net as dn

    _, meta = load_golden("q_toy")
    Q = dn._netQ_U_toy()
    got = [[k, list(v.shape)] for k, v in Q.state_dict().items()]
    assert got == meta["q_keys"]
    assert len(got) == 81
    assert dn.Diffusion_Unet is dn.Diffusion_UnetA
    # the shared loss body: one function for both amortizers
    assert dn._netQ_U_toy.calculate_loss is dn._netQ_U.calculate_loss


@pytest.mark.parametrize("name", TOY_NAMES)
def test_fp64_oracle_reproduces_golden(name):
    """The reference's fp32 result sits 1.5e-7 .. 2.7e-6 from an fp64 evaluation of the same sweep on four schedules
    (torch-default weights), finite even at logsnr +-20: the toy sweep is well conditioned, so the oracle on the
    drop-in must reproduce the golden end-points (and xemb / pe / step-1 eps) within 1e-5 rel-L2."""
    rec, _ = load_golden(name)
    ref = toy_fp64(name)
    d = dict(xemb=rel_l2(rec["xemb"], ref["xemb"]), pe=rel_l2(rec["pe"], ref["pe"]),
             post_eps1=rel_l2(rec["q_post_eps3"][0], ref["post_eps"][0]),
             prior_eps1=rel_l2(rec["q_prior_eps3"][0], ref["prior_eps"][0]),
             post=rel_l2(rec["q_post"], ref["post"]), prior=rel_l2(rec["q_prior"], ref["prior"]))
    print(name, " ".join("%s %.2e" % kv for kv in d.items()))
    for k, v in d.items():
        assert v < 1e-5, (k, v)


def _toy_desc(nz, w=128, ntemb=128, nxemb=128):
    """A host-side damc_denoiser_t of Diffusion_Unet's shapes with placeholder (never dereferenced) pointers."""
    from damc import _lib

    d = _lib.Denoiser()
    d.nz, d.ntemb, d.nxemb, d.residual = nz, ntemb, nxemb, 1
    fake = 256
    for k in ("bmat", "tw1", "tb1", "tw2", "tb2"):
        setattr(d, k, fake)
    din = [2 * nz, w, 2 * w, 2 * w, 4 * w, 4 * w, 2 * w]
    dout = [w, 2 * w, 2 * w, 2 * w, 2 * w, w, nz]
    for j in range(7):
        b = d.blocks[j]
        b.din, b.dout = din[j], dout[j]
        for k in ("wl", "bl", "ws", "bs", "wg", "bg", "wb"):
            setattr(b, k, fake)
        d.wctx[j] = fake
        d.bctx[j] = fake
    return d


def test_sweep_workspace_shapes_host_only(monkeypatch):
    """damc_sweep_workspace_bytes: nz = 2 and nz = 6 (nz % 4 != 0: the row-resident form) are taken, an odd nz is not;
    the shapes accepted before keep their size, also under DAMC_SWEEP_ROWS=1."""
    from damc import _lib

    L = _lib.lib()
    monkeypatch.delenv("DAMC_SWEEP_ROWS", raising=False)
    ws = lambda d, B=21, n=20: int(L.damc_sweep_workspace_bytes(ctypes.byref(d), B, n))  # noqa: E731
    assert ws(_toy_desc(2)) > 0
    assert ws(_toy_desc(6)) > 0
    assert ws(_toy_desc(3)) == 0
    assert ws(_toy_desc(130)) == 0          # nz <= 128
    assert ws(_toy_desc(2, ntemb=24)) == 0  # the narrow route needs ntemb % 16 == 0
    assert ws(_toy_desc(2, w=256)) == 0     # the 16-row LDS image must fit the CU
    n128 = ws(_toy_desc(128))
    assert n128 > 0
    # a shape only the row form takes needs no team rings: at the driver's B = 500, 100 steps, smaller than nz = 4
    assert ws(_toy_desc(2), 500, 100) < ws(_toy_desc(4), 500, 100)
    monkeypatch.setenv("DAMC_SWEEP_ROWS", "1")
    assert ws(_toy_desc(128)) == n128
    assert ws(_toy_desc(100)) > 0


def test_mlp_forward_rejects_bad_descriptors_host_only():
    from damc import _lib

    L = _lib.lib()
    fake = ctypes.c_void_p(256)

    def desc(widths, act=_lib.ACT_RELU):
        d = _lib.Mlp()
        d.n_layers = len(widths) - 1
        for i in range(min(d.n_layers, _lib.MLP_MAX_LAYERS)):
            e = d.layers[i]
            e.din, e.dout, e.act, e.w, e.bias = widths[i], widths[i + 1], act, 256, 256
        return d

    call = lambda d, x=fake, B=4, out=fake: L.damc_mlp_forward(ctypes.byref(d), x, B, out, None)  # noqa: E731
    assert call(desc([2])) == _lib.DAMC_ERR_ARG                        # no layer
    assert call(desc([2] + [8] * 9)) == _lib.DAMC_ERR_ARG              # more than 8 layers
    assert call(desc([2, 128, 64], act=_lib.ACT_TANH)) == _lib.DAMC_ERR_ARG
    d = desc([2, 128, 64])
    d.layers[1].din = 96                                                # does not chain
    assert call(d) == _lib.DAMC_ERR_ARG
    d = desc([2, 128, 64])
    d.layers[0].w = None
    assert call(d) == _lib.DAMC_ERR_ARG
    assert call(desc([2, 0, 64])) == _lib.DAMC_ERR_ARG
    assert call(desc([2, 512, 64])) == _lib.DAMC_ERR_UNSUPPORTED       # widths <= 256
    good = desc([2, 128, 64])
    assert call(good, x=None) == _lib.DAMC_ERR_ARG
    assert call(good, out=None) == _lib.DAMC_ERR_ARG
    assert call(good, B=0) == _lib.DAMC_ERR_ARG


def test_toy_guidance_is_refused():
    """cond_w > 0 on the toy is out of scope: a clear NotImplementedError, before any device work."""
    import torch

    c = build_toy_case("q_toy")
    with pytest.raises(NotImplementedError):
        c["Q"](c["x"], cond_w=0.5)
    assert isinstance(c["Q"].encoder, torch.nn.Sequential)
