"""GPU: the tap-shared A staging of the limb GEMM (gemm_x3.hip X3_TAPSHARE) -- one fp32 input image per group of four K
tiles (a ConvT phase's four taps, or the four taps of a parity class of its input gradient) instead of one per tap.

* the per-op hooks damc_convT_fwd / damc_convT_dgrad against fp64 conv_transpose2d / conv2d at the project's ConvT
  tolerance (rel-L2 < 1e-6, tests/test_gpu_ops.py), on 4^2, 8^2 and 16^2 grids, with a ragged last tile and an image
  boundary inside a tile (B=5) and a single partial tile (B=1); damc_x3_layer_tapshare and the launch counter show
  that the shared staging ran;
* noisy posterior steps at full width, shared staging against per-tap staging (DAMC_X3_TAPSHARE=0), bit for bit, unsplit
  and split-K;
* a 32^2 grid (CelebA-HQ) reports "not shared", launches nothing shared and still matches fp64.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _hooks_against_fp64(gpu_device, ctor, ngf, nz, layer, batches, shared):
    from damc import _lib, plans, synth
    from damc._lib import ptr
    from src import diffusion_net as dn

    G = synth.load_into(getattr(dn, ctor)(nz=nz, ngf=ngf, nc=3), 0).to(gpu_device).eval()
    Ld = plans.generator_plan(G).refresh(gpu_device).layers[layer]
    conv = G.gen[2 * layer]
    assert isinstance(conv, torch.nn.ConvTranspose2d) and Ld.kind == _lib.LAYER_UP2
    L = _lib.lib()
    want = 1 if shared else 0
    assert L.damc_x3_layer_walk(ctypes.byref(Ld), 0) == 1 and L.damc_x3_layer_walk(ctypes.byref(Ld), 1) == 1
    assert L.damc_x3_layer_tapshare(ctypes.byref(Ld), 0) == want
    assert L.damc_x3_layer_tapshare(ctypes.byref(Ld), 1) == want
    Bmax = max(batches)
    g = torch.Generator().manual_seed(41 + layer)
    h = torch.randn(Bmax, Ld.cin, Ld.hin, Ld.win, generator=g, dtype=torch.float64).float()
    gout = torch.randn(Bmax, Ld.cout, Ld.hout, Ld.wout, generator=g, dtype=torch.float64).float()
    w = conv.weight.detach().cpu().double()
    b = conv.bias.detach().cpu().double()
    # the references once, for the largest batch (samples are independent: a smaller batch is its first rows)
    ref = _nhwc(F.leaky_relu(F.conv_transpose2d(h.double(), w, b, stride=2, padding=1), 0.2)).numpy()
    gfull = F.conv2d(gout.double(), w, stride=2, padding=1)
    gref = _nhwc(gfull).numpy()
    gref_m = _nhwc(gfull * torch.where(h.double() > 0, 1.0, 0.2)).numpy()
    stream = _lib.stream_ptr(gpu_device)
    for B in batches:
        nbytes = int(L.damc_convT_workspace_bytes(ctypes.byref(Ld), B))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
        hin = _nhwc(h[:B]).to(gpu_device)
        gdev = _nhwc(gout[:B]).to(gpu_device)
        out = torch.empty(B, Ld.hout, Ld.wout, Ld.cout, device=gpu_device)
        gin = torch.empty(B, Ld.hin, Ld.win, Ld.cin, device=gpu_device)
        n0 = int(L.damc_x3_tapshare_launches())
        _lib.check(L.damc_convT_fwd(ctypes.byref(Ld), ptr(hin), B, ptr(out), ptr(ws), nbytes, stream), "convT_fwd")
        n1 = int(L.damc_x3_tapshare_launches())
        _lib.check(L.damc_convT_dgrad(ctypes.byref(Ld), ptr(gdev), B, ptr(hin), _lib.ACT_LRELU, 0.2, ptr(gin), ptr(ws),
                                      nbytes, stream), "convT_dgrad")
        n2 = int(L.damc_x3_tapshare_launches())
        torch.cuda.synchronize()
        e_f = rel_l2(out.cpu().numpy(), ref[:B])
        e_m = rel_l2(gin.cpu().numpy(), gref_m[:B])
        _lib.check(L.damc_convT_dgrad(ctypes.byref(Ld), ptr(gdev), B, None, 0, 0.0, ptr(gin), ptr(ws), nbytes, stream),
                   "convT_dgrad")
        n3 = int(L.damc_x3_tapshare_launches())
        torch.cuda.synchronize()
        e_u = rel_l2(gin.cpu().numpy(), gref[:B])
        print("%s ngf=%d layer %d B=%d: fwd %.3e dgrad masked %.3e unmasked %.3e, shared launches %d %d %d"
              % (ctor, ngf, layer, B, e_f, e_m, e_u, n1 - n0, n2 - n1, n3 - n2))
        assert (n1 - n0, n2 - n1, n3 - n2) == (want, want, want)  # engagement, not a silent fallback
        assert e_f < 1e-6 and e_m < 1e-6 and e_u < 1e-6


@pytest.mark.parametrize("ctor,ngf,nz,layer", [("_netG_cifar10", 32, 128, 1), ("_netG_cifar10", 32, 128, 2),
                                               ("_netG_cifar10", 128, 128, 2), ("_netG_celeba64", 32, 100, 1)])
def test_shared_staging_hooks_match_fp64(gpu_device, monkeypatch, ctor, ngf, nz, layer):
    """8^2 and 16^2 grids (CIFAR-10 layers 1 and 2; Cout 128 / 64 at ngf=32, 256 at ngf=128) and a 4^2 grid (CelebA-64's
    first k4 s2 layer, 16 images per tile).  B=5: a ragged last tile at the 4^2 and 8^2 grids and image boundaries
    inside a tile; B=1: one partial tile."""
    monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    _hooks_against_fp64(gpu_device, ctor, ngf, nz, layer, (5, 1), shared=True)


def test_large_grid_falls_back_and_matches_fp64(gpu_device, monkeypatch):
    """_netG_celebaHQ's 32^2-grid layer (layer 4) at ngf=16, the smallest width the limb engine accepts (its input
    gradient gathers 2 ngf = 32 channels, one K slice): an M tile is a strip of one image, so the launch keeps the
    per-tap staging on the same K order."""
    monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    _hooks_against_fp64(gpu_device, "_netG_celebaHQ", 16, 128, 4, (1,), shared=False)


_NETS = {"cifar10": ("_netG_cifar10", 128, 128, 32), "svhn": ("_netG_svhn", 100, 64, 32),
         "celeba64": ("_netG_celeba64", 100, 128, 64)}


@pytest.mark.parametrize("name,B,ksplit", [("cifar10", 5, "0"), ("cifar10", 5, "1"), ("cifar10", 16, "0"),
                                           ("cifar10", 16, "1"), ("svhn", 64, "1"), ("celeba64", 4, "1")])
def test_shared_staging_is_bitwise_the_per_tap_staging(gpu_device, monkeypatch, name, B, ksplit):
    """3 noisy posterior steps at full width: DAMC_X3_TAPSHARE=1 (default) against 0, unsplit (DAMC_X3_KSPLIT=0) and with
    the register-slab split-K these batches take.  Both stagings put the same fp32 values in front of the limb split on
    the same K order, so the chains agree bit for bit; the counter shows which one ran."""
    from damc import _lib, synth
    from damc import langevin as lv
    from src import diffusion_net as dn

    ctor, nz, ngf, hw = _NETS[name]
    G = synth.load_into(getattr(dn, ctor)(nz=nz, ngf=ngf, nc=3), 0).to(gpu_device).eval()
    E = synth.load_into(dn._netE(nz=nz), 10).to(gpu_device).eval()
    x = torch.from_numpy(synth.uniform_f32(11, 0, (B, 3, hw, hw))).to(gpu_device)
    z0 = torch.from_numpy(synth.normal_f32(12, 0, (B, nz))).to(gpu_device)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    monkeypatch.setenv("DAMC_X3_KSPLIT", ksplit)
    L = _lib.lib()
    out, ran = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DAMC_X3_TAPSHARE", mode)
        z = z0.clone()
        n0 = int(L.damc_x3_tapshare_launches())
        lv.posterior_langevin(z, x, G, E, 3, 0.1, 0.1, True, seed=5)
        torch.cuda.synchronize()
        ran[mode] = int(L.damc_x3_tapshare_launches()) - n0
        out[mode] = z.cpu()
    print("%s B=%d ksplit=%s: shared launches %d (off: %d)" % (name, B, ksplit, ran["1"], ran["0"]))
    assert ran["0"] == 0 and ran["1"] > 0
    assert torch.isfinite(out["1"]).all()
    assert torch.equal(out["0"], out["1"])
