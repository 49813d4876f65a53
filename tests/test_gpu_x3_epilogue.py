"""GPU: the tap-shared limb GEMM tile's own epilogue (gemm_x3.hip X3_TAPSHARE, round 14) -- the fused projection on
preloaded weight fragments with the output pixel from a row table, row tables by shifts, one bias load per thread, and
the read table built behind the first DMA.  None of it changes an output byte:

* two noisy posterior steps on _netG_cifar10 at ngf = 32 (L3 N = 64: half of the N tile and of the projection chunk is
  dead) and ngf = 128 (two chunks), B = 1 (one partial M tile) and B = 5 (a ragged last tile on the 8^2 grid, image
  boundaries inside a tile), unsplit (DAMC_X3_KSPLIT=0, so the tap-shared kernels run their own epilogue): the chain
  against the per-tap kernel and its untouched epilogue (DAMC_X3_TAPSHARE=0) and against the separate
  proj_rows_kernel (DAMC_SMALLC_FUSE=0), bit for bit.  The chain reads the sign bytes, the fp32 activations, the P
  partials and the input gradients;
* the per-op hooks damc_convT_fwd / damc_convT_dgrad at the same nets and batches with the output and the workspace
  inside larger NaN-patterned buffers: the guard regions are untouched (no store may pass the last live row), the
  results match fp64 at the ConvT tolerance of tests/test_gpu_tapshare.py (rel-L2 < 1e-6).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

NZ = 128


def _net(gpu_device, ngf):
    from damc import synth
    from src import diffusion_net as dn

    return synth.load_into(dn._netG_cifar10(nz=NZ, ngf=ngf, nc=3), 0).to(gpu_device).eval()


@pytest.mark.parametrize("ngf", [32, 128])
@pytest.mark.parametrize("B", [1, 5])
def test_chain_is_bitwise_the_per_tap_and_the_unfused_chain(gpu_device, monkeypatch, ngf, B):
    from damc import _lib, synth
    from damc import langevin as lv
    from src import diffusion_net as dn

    G = _net(gpu_device, ngf)
    E = synth.load_into(dn._netE(nz=NZ), 10).to(gpu_device).eval()
    x = torch.from_numpy(synth.uniform_f32(21, 0, (B, 3, 32, 32))).to(gpu_device)
    z0 = torch.from_numpy(synth.normal_f32(22, 0, (B, NZ))).to(gpu_device)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    monkeypatch.setenv("DAMC_X3_KSPLIT", "0")
    L = _lib.lib()
    out, ran = {}, {}
    for name, env in (("default", {}), ("per_tap", {"DAMC_X3_TAPSHARE": "0"}), ("unfused", {"DAMC_SMALLC_FUSE": "0"})):
        monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
        monkeypatch.delenv("DAMC_SMALLC_FUSE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        z = z0.clone()
        n0 = int(L.damc_x3_tapshare_launches())
        lv.posterior_langevin(z, x, G, E, 2, 0.1, 0.1, True, seed=7)
        torch.cuda.synchronize()
        ran[name] = int(L.damc_x3_tapshare_launches()) - n0
        out[name] = z.cpu()
    print("ngf=%d B=%d: tap-shared launches default %d, per-tap %d, unfused %d"
          % (ngf, B, ran["default"], ran["per_tap"], ran["unfused"]))
    assert ran["default"] > 0 and ran["per_tap"] == 0  # the unsplit tap-shared kernels ran, not a fallback
    assert torch.isfinite(out["default"]).all()
    assert torch.equal(out["default"], out["per_tap"])
    assert torch.equal(out["default"], out["unfused"])


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


GUARD = 4096  # guard elements (floats / bytes) on either side of a buffer; keeps the 16-byte alignment


def _guarded(n, dtype, dev):
    """n elements inside a larger buffer of all-ones bytes (a NaN pattern as fp32): (whole buffer as bytes, the view)"""
    esz = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full(((n + 2 * GUARD) * esz,), 0xFF, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD * esz:(GUARD + n) * esz].view(dtype)


def _guards_intact(whole, n, dtype):
    esz = torch.empty(0, dtype=dtype).element_size()
    return bool((whole[:GUARD * esz] == 0xFF).all()) and bool((whole[(GUARD + n) * esz:] == 0xFF).all())


@pytest.mark.parametrize("ngf", [32, 128])
@pytest.mark.parametrize("layer", [1, 2])
def test_hooks_stay_inside_their_buffers_and_match_fp64(gpu_device, monkeypatch, ngf, layer):
    from damc import _lib, plans
    from damc._lib import ptr

    monkeypatch.delenv("DAMC_X3_TAPSHARE", raising=False)
    monkeypatch.delenv("DAMC_X3_F32A", raising=False)
    monkeypatch.setenv("DAMC_X3_KSPLIT", "0")
    G = _net(gpu_device, ngf)
    Ld = plans.generator_plan(G).refresh(gpu_device).layers[layer]
    conv = G.gen[2 * layer]
    assert isinstance(conv, torch.nn.ConvTranspose2d) and Ld.kind == _lib.LAYER_UP2
    L = _lib.lib()
    assert L.damc_x3_layer_tapshare(ctypes.byref(Ld), 0) == 1 and L.damc_x3_layer_tapshare(ctypes.byref(Ld), 1) == 1
    batches = (5, 1)
    g = torch.Generator().manual_seed(51 + layer)
    h = torch.randn(max(batches), Ld.cin, Ld.hin, Ld.win, generator=g, dtype=torch.float64).float()
    gout = torch.randn(max(batches), Ld.cout, Ld.hout, Ld.wout, generator=g, dtype=torch.float64).float()
    w = conv.weight.detach().cpu().double()
    b = conv.bias.detach().cpu().double()
    # the references once, for the larger batch (samples are independent: a smaller batch is its first rows)
    ref = _nhwc(F.leaky_relu(F.conv_transpose2d(h.double(), w, b, stride=2, padding=1), 0.2)).numpy()
    gfull = F.conv2d(gout.double(), w, stride=2, padding=1)
    gref = _nhwc(gfull).numpy()
    gref_m = _nhwc(gfull * torch.where(h.double() > 0, 1.0, 0.2)).numpy()
    stream = _lib.stream_ptr(gpu_device)
    for B in batches:
        nbytes = int(L.damc_convT_workspace_bytes(ctypes.byref(Ld), B))
        assert nbytes > 0
        n_out, n_in = B * Ld.hout * Ld.wout * Ld.cout, B * Ld.hin * Ld.win * Ld.cin
        ws_all, ws = _guarded(nbytes, torch.uint8, gpu_device)
        out_all, out = _guarded(n_out, torch.float32, gpu_device)
        gin_all, gin = _guarded(n_in, torch.float32, gpu_device)
        hin = _nhwc(h[:B]).to(gpu_device)
        gdev = _nhwc(gout[:B]).to(gpu_device)
        n0 = int(L.damc_x3_tapshare_launches())
        _lib.check(L.damc_convT_fwd(ctypes.byref(Ld), ptr(hin), B, ptr(out), ptr(ws), nbytes, stream), "convT_fwd")
        _lib.check(L.damc_convT_dgrad(ctypes.byref(Ld), ptr(gdev), B, ptr(hin), _lib.ACT_LRELU, 0.2, ptr(gin), ptr(ws),
                                      nbytes, stream), "convT_dgrad")
        torch.cuda.synchronize()
        e_f = rel_l2(out.view(B, Ld.hout, Ld.wout, Ld.cout).cpu().numpy(), ref[:B])
        e_m = rel_l2(gin.view(B, Ld.hin, Ld.win, Ld.cin).cpu().numpy(), gref_m[:B])
        _lib.check(L.damc_convT_dgrad(ctypes.byref(Ld), ptr(gdev), B, None, 0, 0.0, ptr(gin), ptr(ws), nbytes, stream),
                   "convT_dgrad")
        torch.cuda.synchronize()
        n1 = int(L.damc_x3_tapshare_launches())
        e_u = rel_l2(gin.view(B, Ld.hin, Ld.win, Ld.cin).cpu().numpy(), gref[:B])
        print("ngf=%d layer %d B=%d: fwd %.3e dgrad masked %.3e unmasked %.3e, shared launches %d"
              % (ngf, layer, B, e_f, e_m, e_u, n1 - n0))
        assert n1 - n0 == 3  # the three calls each ran the tap-shared kernel
        assert _guards_intact(out_all, n_out, torch.float32), "fwd output guard"
        assert _guards_intact(gin_all, n_in, torch.float32), "dgrad output guard"
        assert _guards_intact(ws_all, nbytes, torch.uint8), "workspace guard"
        assert e_f < 1e-6 and e_m < 1e-6 and e_u < 1e-6
