"""GPU: the tap-shared K loop of the limb GEMM on the 4 (M) x 2 (N) wave grid (gemm_x3.hip X3_TAPSHARE, round 11) -- what
a wave grid newly gets wrong is a wave row or a wave column that lies partly or wholly outside the GEMM.

* two noisy posterior steps at ngf = 32, the smallest width the tap-shared path accepts, default against per-tap staging
  (DAMC_X3_TAPSHARE=0, the 8 x 1 loop this change leaves alone), bit for bit, unsplit and with register-slab split-K:
    4^2 grid  B=3  M=48   one wave row, three of its four A tiles live        (CelebA-64 layer 1)
    4^2 grid  B=5  M=80   wave row 1 has a single live 16-row tile
    8^2 grid  B=1  M=64   only wave row 0                                     (CIFAR-10 layer 1, CelebA-64 layer 2)
    8^2 grid  B=3  M=192  wave row 3 dead
    16^2 grid B=1  M=256  a full tile                                         (CIFAR-10 layer 2, CelebA-64 layer 3)
* the ConvT forward and input-gradient hooks of CIFAR-10's last k4 s2 layer at ngf = 32 (forward N = 64: wave column 1
  wholly outside N) and of its 8^2 layer, B = 1 and 3, against fp64 at the hook test's bound (rel-L2 < 1e-6), on both
  stagings.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

_NETS = {"cifar10": ("_netG_cifar10", 128, 32), "celeba64": ("_netG_celeba64", 100, 64)}


@pytest.mark.parametrize("ksplit", ["0", "1"])
@pytest.mark.parametrize("name,B", [("celeba64", 3), ("celeba64", 5), ("cifar10", 1), ("cifar10", 3)])
def test_wave_grid_is_bitwise_the_per_tap_staging(gpu_device, monkeypatch, name, B, ksplit):
    """2 noisy posterior steps at ngf = 32: the 4 x 2 grid's loop against DAMC_X3_TAPSHARE=0 with torch.equal; the
    launch counter shows which staging ran."""
    from damc import _lib, synth
    from damc import langevin as lv
    from src import diffusion_net as dn

    ctor, nz, hw = _NETS[name]
    G = synth.load_into(getattr(dn, ctor)(nz=nz, ngf=32, nc=3), 0).to(gpu_device).eval()
    E = synth.load_into(dn._netE(nz=nz), 10).to(gpu_device).eval()
    x = torch.from_numpy(synth.uniform_f32(21, 0, (B, 3, hw, hw))).to(gpu_device)
    z0 = torch.from_numpy(synth.normal_f32(22, 0, (B, nz))).to(gpu_device)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    monkeypatch.setenv("DAMC_X3_KSPLIT", ksplit)
    L = _lib.lib()
    out, ran = {}, {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
        else:
            monkeypatch.setenv("DAMC_X3_TAPSHARE", mode)
        z = z0.clone()
        n0 = int(L.damc_x3_tapshare_launches())
        lv.posterior_langevin(z, x, G, E, 2, 0.1, 0.1, True, seed=7)
        torch.cuda.synchronize()
        ran[mode] = int(L.damc_x3_tapshare_launches()) - n0
        out[mode] = z.cpu()
    print("%s ngf=32 B=%d ksplit=%s: shared launches %d (off: %d)" % (name, B, ksplit, ran[None], ran["0"]))
    assert ran["0"] == 0 and ran[None] > 0
    assert torch.isfinite(out[None]).all()
    assert torch.equal(out["0"], out[None])


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("layer", [1, 2])
def test_dead_wave_column_hooks_match_fp64(gpu_device, monkeypatch, layer):
    """_netG_cifar10 at ngf = 32: layer 2 (16^2 grid) has forward N = 64, so wave column 1 multiplies B rows that are all
    out of range; layer 1 is the 8^2 grid (M = 64 B).  B = 1 and 3, per-tap staging (the reference arm) and the default,
    each against fp64 conv_transpose2d / conv2d at rel-L2 < 1e-6."""
    from damc import _lib, plans, synth
    from damc._lib import ptr
    from src import diffusion_net as dn

    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=32, nc=3), 0).to(gpu_device).eval()
    Ld = plans.generator_plan(G).refresh(gpu_device).layers[layer]
    conv = G.gen[2 * layer]
    assert isinstance(conv, torch.nn.ConvTranspose2d) and Ld.kind == _lib.LAYER_UP2
    if layer == 2:
        assert Ld.cout == 64
    L = _lib.lib()
    assert L.damc_x3_layer_tapshare(ctypes.byref(Ld), 0) == 1 and L.damc_x3_layer_tapshare(ctypes.byref(Ld), 1) == 1
    batches = (3, 1)
    g = torch.Generator().manual_seed(51 + layer)
    h = torch.randn(3, Ld.cin, Ld.hin, Ld.win, generator=g, dtype=torch.float64).float()
    gout = torch.randn(3, Ld.cout, Ld.hout, Ld.wout, generator=g, dtype=torch.float64).float()
    w = conv.weight.detach().cpu().double()
    b = conv.bias.detach().cpu().double()
    # the references once, for the larger batch (samples are independent: B = 1 is its first row)
    ref = _nhwc(F.leaky_relu(F.conv_transpose2d(h.double(), w, b, stride=2, padding=1), 0.2)).numpy()
    gfull = F.conv2d(gout.double(), w, stride=2, padding=1)
    gref = _nhwc(gfull).numpy()
    gref_m = _nhwc(gfull * torch.where(h.double() > 0, 1.0, 0.2)).numpy()
    stream = _lib.stream_ptr(gpu_device)
    for mode, want in (("0", 0), (None, 1)):
        if mode is None:
            monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
        else:
            monkeypatch.setenv("DAMC_X3_TAPSHARE", mode)
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
            _lib.check(L.damc_convT_dgrad(ctypes.byref(Ld), ptr(gdev), B, ptr(hin), _lib.ACT_LRELU, 0.2, ptr(gin),
                                          ptr(ws), nbytes, stream), "convT_dgrad")
            n2 = int(L.damc_x3_tapshare_launches())
            torch.cuda.synchronize()
            e_f = rel_l2(out.cpu().numpy(), ref[:B])
            e_m = rel_l2(gin.cpu().numpy(), gref_m[:B])
            _lib.check(L.damc_convT_dgrad(ctypes.byref(Ld), ptr(gdev), B, None, 0, 0.0, ptr(gin), ptr(ws), nbytes,
                                          stream), "convT_dgrad")
            n3 = int(L.damc_x3_tapshare_launches())
            torch.cuda.synchronize()
            e_u = rel_l2(gin.cpu().numpy(), gref[:B])
            print("cifar10 ngf=32 layer %d B=%d tapshare=%s: fwd %.3e dgrad masked %.3e unmasked %.3e, shared launches "
                  "%d %d %d" % (layer, B, mode, e_f, e_m, e_u, n1 - n0, n2 - n1, n3 - n2))
            assert (n1 - n0, n2 - n1, n3 - n2) == (want, want, want)  # which staging ran, not a silent fallback
            assert e_f < 1e-6 and e_m < 1e-6 and e_u < 1e-6
