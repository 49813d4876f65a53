"""GPU: the LDS limb image of the tap-shared limb GEMM (gemm_x3.hip X3_TAPSHARE, round 9) -- a group's staged fp32 image is
split into its bf16 limbs once, and the four taps read their MFMA A fragments from the limb image at displaced rows.

* the per-op hooks damc_convT_fwd / damc_convT_dgrad (masked and unmasked) against fp64 conv_transpose2d / conv2d at the
  project's ConvT tolerance (rel-L2 < 1e-6), on a 4^2, an 8^2 and a 16^2 grid, B=5 (ragged last tile, image boundaries
  inside a tile) and B=1 (one partial tile); the launch counter advances by one per call;
* the shortest K loops: a k4 s2 layer of 32 -> 32 channels on a 16^2 grid (the forward's workgroup runs exactly one
  group: the conversion in the prologue only; the input gradient one 32-channel slice) and of 64 -> 64 (two groups: one
  hand-over from the staging image to the limb image);
* three noisy posterior steps at full width, default against per-tap staging (DAMC_X3_TAPSHARE=0), bit for bit, unsplit
  and with the register-slab split-K;
* the 32^2 grid still reports "not shared", launches nothing shared and matches fp64.

The fp64 comparison and the networks are those of tests/test_gpu_tapshare.py.
"""
import pytest
import torch

from test_gpu_tapshare import _NETS, _hooks_against_fp64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ctor,ngf,nz,layer", [("_netG_celeba64", 32, 100, 1), ("_netG_cifar10", 32, 128, 1),
                                               ("_netG_cifar10", 32, 128, 2)])
def test_limb_image_hooks_match_fp64(gpu_device, monkeypatch, ctor, ngf, nz, layer):
    """A 4^2 grid (16 images per 256-row tile), an 8^2 grid and a 16^2 grid; B=5 and B=1."""
    monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    _hooks_against_fp64(gpu_device, ctor, ngf, nz, layer, (5, 1), shared=True)


@pytest.mark.parametrize("ngf", [8, 16])
def test_shortest_k_loops_match_fp64(gpu_device, monkeypatch, ngf):
    """_netG_celebaHQ's layer 3 (4 ngf -> 4 ngf channels, 16^2 -> 32^2) at ngf=8, the narrowest width the limb engine
    takes in both directions (32 gathered channels: the forward's K is 4 x 32 = one group of four K tiles, so the limb
    image is only ever written by the prologue), and at twice that (two groups: the loop's one conversion)."""
    monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    _hooks_against_fp64(gpu_device, "_netG_celebaHQ", ngf, 128, 3, (5, 1), shared=True)


@pytest.mark.parametrize("name,B,ksplit", [("cifar10", 5, "0"), ("cifar10", 5, "1"), ("cifar10", 16, "0"),
                                           ("cifar10", 16, "1"), ("svhn", 64, "1"), ("celeba64", 4, "1")])
def test_limb_image_is_bitwise_the_per_tap_staging(gpu_device, monkeypatch, name, B, ksplit):
    """3 noisy posterior steps at full width, default against DAMC_X3_TAPSHARE=0, unsplit (DAMC_X3_KSPLIT=0) and with the
    register-slab split-K these batches take.  The limb image holds the limbs the per-tap loop splits in registers, in
    the same K order, so the chains agree bit for bit; the counter shows which loop ran."""
    from damc import _lib, synth
    from damc import langevin as lv
    from src import diffusion_net as dn

    ctor, nz, ngf, hw = _NETS[name]
    G = synth.load_into(getattr(dn, ctor)(nz=nz, ngf=ngf, nc=3), 0).to(gpu_device).eval()
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
        lv.posterior_langevin(z, x, G, E, 3, 0.1, 0.1, True, seed=7)
        torch.cuda.synchronize()
        ran[mode] = int(L.damc_x3_tapshare_launches()) - n0
        out[mode] = z.cpu()
    print("%s B=%d ksplit=%s: shared launches %d (off: %d)" % (name, B, ksplit, ran[None], ran["0"]))
    assert ran["0"] == 0 and ran[None] > 0
    assert torch.isfinite(out[None]).all()
    assert torch.equal(out["0"], out[None])


def test_large_grid_keeps_per_tap_staging(gpu_device, monkeypatch):
    """_netG_celebaHQ's 32^2-grid layer (layer 4) at ngf=16, B=1: an M tile is a strip of one image, so the launch keeps
    the per-tap staging with the in-register split."""
    monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    _hooks_against_fp64(gpu_device, "_netG_celebaHQ", 16, 128, 4, (1,), shared=False)
