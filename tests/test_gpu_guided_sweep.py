"""GPU: the guided reverse sweep (classifier-free guidance, Q(x, cond_w = w > 0), diffusion_net.py:595-620) as one
damc_guided_sweep call: the twin-row form of the row-resident sweep (csrc/denoiser_rows.hip), its per-call stages, the
seeded and the reference-draw mode of damc.amortizer.q_forward.

Two small denoisers, encoder nif 8:
  A  nz 16, nf 1, nxemb 64, ntemb 32: out2 (dout 16) and with it the hyper stage are off the limb path;
  B  nz 128, nf 4, nxemb 64, ntemb 32: the production block widths, the limb hyper path.
Batches 1, 8, 9 and 21: under one tile, one full tile of 8 latent rows, a second tile with one live pair, three tiles
with a partial last one.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

KINDS = {"A": dict(nz=16, nf=1), "B": dict(nz=128, nf=4)}
_Q = {}


def make_q(kind, n, device, with_noise=True):
    """The denoiser of a kind is the same for every n and with_noise (counter-hash weights by parameter)."""
    from damc import synth
    from src import diffusion_net as dn

    key = (kind, n, with_noise)
    if key not in _Q:
        Q = dn._netQ_U(nc=3, nxemb=64, ntemb=32, nif=8, diffusion_residual=True, n_interval=n, logsnr_min=-5.1,
                       logsnr_max=9.8, var_type="large", with_noise=with_noise, dataset="cifar10", **KINDS[kind])
        synth.load_into(Q, 20)
        _Q[key] = Q.to(device).eval()
    return _Q[key]


def images(B, device):
    from damc import synth

    return torch.from_numpy(synth.uniform_f32(93, 0, (B, 3, 32, 32))).to(device)


def latent(B, nz, device, seed=8):
    from damc import synth

    return torch.from_numpy(synth.normal_f32(seed, 0, (B, nz))).to(device)


def stock_loop(Qm, x, w, dt, eps_trace=None):
    """diffusion_net.py:585-622 with cond_w = w on stock modules in dtype dt, fp32 draws in the reference's order."""
    from src import diffusion_helper_func as dh

    b, n, dev = len(x), Qm.n_interval, x.device
    xemb = Qm.encoder(x.to(dt))
    zt = torch.randn(b, Qm.nz).to(dev).to(dt)
    for i in reversed(range(0, n)):
        it = torch.ones(b, dtype=dt).to(dev) * float(i)
        lt = dh.logsnr_schedule_fn(it / (n - 1.0), logsnr_min=Qm.logsnr_min, logsnr_max=Qm.logsnr_max)
        ls = dh.logsnr_schedule_fn(torch.clamp(it - 1.0, min=0.0) / (n - 1.0), logsnr_min=Qm.logsnr_min,
                                   logsnr_max=Qm.logsnr_max)
        e = Qm.p(z=zt, logsnr=lt, xemb=xemb)
        eu = Qm.p(z=zt, logsnr=lt, xemb=Qm.prior_emb(torch.randn(b, Qm.nz, device=dev).to(dt)))
        e = (1 + w) * e - w * eu
        if eps_trace is not None:
            eps_trace.append(e.clone())
        lt, ls = lt.reshape((b, 1)), ls.reshape((b, 1))
        pz = dh.pred_x_from_eps(z=zt, eps=e, logsnr=lt)
        if i == 0:
            zt = pz
        else:
            d = dh.diffusion_reverse(x=pz, z_t=zt, logsnr_s=ls, logsnr_t=lt, pred_var_type=Qm.var_type)
            xi = torch.randn(zt.shape, device=dev).to(dt)
            zt = d["mean"] + d["std"] * xi if Qm.with_noise else d["mean"]
    return zt.double()


# ------------------------------------------------------------------------------------------- 1. the reference's loop
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 8, 9, 21])
@pytest.mark.parametrize("kind", ["A", "B"])
def test_guided_sweep_matches_the_reference_loop(gpu_device, kind, B, n):
    """_q_forward_guided (the fused sweep, reference-draw mode) against the reference's step loop from the same torch
    seed, for w in {0.5, 2.0} and with_noise on and off: _q_forward_guided_steps under training.stock_pytorch() (the
    stock fp32 denoiser) and the loop on stock modules in fp64.  The project's bounds of the existing guidance test:
    the step-1 guided eps within 1e-5 rel-L2 of the stock fp32 one, the end point d_hip <= 3 d_ref + 1e-6 where d is
    the rel-L2 distance from fp64.

    n = 1: the reference's schedule divides by n_interval - 1 (diffusion_net.py:597-600: i / (n - 1.0) = 0 / 0), so
    its one-step sweep is NaN throughout, in fp32 and fp64 alike.  No distance exists there; the case holds the sweep
    to the reference's own outcome, NaN in every element of the eps and of the end point, and n = 2 (one noisy and the
    last step) is the shortest sweep the bounds apply to."""
    from damc import amortizer, training

    x = images(B, gpu_device)
    for w in (0.5, 2.0):
        for with_noise in (True, False):
            Q = make_q(kind, n, gpu_device, with_noise)
            torch.manual_seed(7)
            eps_hip = []
            with torch.no_grad():
                z_hip = amortizer._q_forward_guided(Q, x, w, eps_trace=eps_hip)
            assert len(eps_hip) == n and z_hip.shape == (B, Q.nz)
            with training.stock_pytorch(), torch.no_grad():
                torch.manual_seed(7)
                eps32 = []
                z32 = amortizer._q_forward_guided_steps(Q, x, w, eps_trace=eps32)
                torch.manual_seed(7)
                z64 = stock_loop(copy.deepcopy(Q).double(), x, w, torch.float64)
            if n == 1:
                assert torch.isnan(z32).all() and torch.isnan(z64).all() and torch.isnan(eps32[0]).all()
                assert torch.isnan(z_hip).all() and torch.isnan(eps_hip[0]).all()
                continue
            e1 = rel_l2(eps_hip[0].cpu().numpy(), eps32[0].cpu().numpy())
            d_hip = rel_l2(z_hip.double().cpu().numpy(), z64.cpu().numpy())
            d_ref = rel_l2(z32.double().cpu().numpy(), z64.cpu().numpy())
            print("guided %s B %d n %d w %.1f noise %d: eps1 %.2e, end point vs fp64 HIP %.2e stock fp32 %.2e"
                  % (kind, B, n, w, with_noise, e1, d_hip, d_ref))
            assert torch.isfinite(z_hip).all()
            assert e1 <= 1e-5, e1
            assert d_hip <= 3 * d_ref + 1e-6, (d_hip, d_ref)


# ----------------------------------------------------------------------------------------------- 2. the twin layout
@pytest.mark.parametrize("w", [0.5, 2.0])
@pytest.mark.parametrize("B", [9, 21])
@pytest.mark.parametrize("kind", ["A", "B"])
def test_twin_rows_are_the_two_evaluations_exactly(gpu_device, monkeypatch, kind, B, w):
    """One guided step's eps_log is bitwise (1 + w) * eps_c - w * eps_u of the two single evaluations
    (damc_denoise_step on the row-resident form, one per embedding, from the same zt), combined with eager torch ops:
    the twin rows, the plane lookup and the pair exchange change no bit of either evaluation."""
    from damc import _lib, amortizer
    from damc._lib import ptr

    Q = make_q(kind, 5, gpu_device)
    nz = Q.nz
    plan = amortizer.DenoiserPlan(Q.p)
    d = plan.pack(gpu_device)
    coef_h, temb_d = amortizer.cached_step_tables(5, Q.logsnr_min, Q.logsnr_max, Q.var_type, plan.ntemb, gpu_device)
    coef_row = np.ascontiguousarray(coef_h.numpy()[1:2])
    temb_row = temb_d[1:2].contiguous()
    xemb = latent(B, 64, gpu_device, seed=31)
    xemb_u = latent(B, 64, gpu_device, seed=32)
    zt0 = latent(B, nz, gpu_device)
    L = _lib.lib()
    stream = _lib.stream_ptr(gpu_device)
    cp = coef_row.ctypes.data_as(ctypes.c_void_p)

    nb = int(L.damc_guided_sweep_workspace_bytes(ctypes.byref(d), B, 1))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=gpu_device)
    zg = zt0.clone()
    eps_g = torch.full((1, B, nz), float("nan"), device=gpu_device)
    _lib.check(L.damc_guided_sweep(ctypes.byref(d), ptr(xemb), ptr(xemb_u), w, ptr(zg), B, 1, ptr(temb_row), cp, 0,
                                   None, 0, 0, ptr(eps_g), 1, ptr(ws), nb, stream), "damc_guided_sweep")

    monkeypatch.setenv("DAMC_SWEEP_ROWS", "1")
    nb1 = int(L.damc_sweep_workspace_bytes(ctypes.byref(d), B, 1))
    ws1 = torch.empty(nb1, dtype=torch.uint8, device=gpu_device)
    eps = []
    for xe in (xemb, xemb_u):
        z = zt0.clone()
        e = torch.full((B, nz), float("nan"), device=gpu_device)
        _lib.check(L.damc_denoise_step(ctypes.byref(d), ptr(xe), ptr(z), B, ptr(temb_row), cp, 0, None, 0, 0, 0,
                                       ptr(e), ptr(ws1), nb1, stream), "damc_denoise_step")
        eps.append(e)
    torch.cuda.synchronize()
    want = (1 + w) * eps[0] - w * eps[1]
    assert torch.isfinite(want).all() and not torch.equal(eps[0], eps[1])
    assert torch.equal(eps_g[0], want)
    # and the step both twins took is the reference's step on that eps
    c = [torch.tensor(float(v), device=gpu_device) for v in coef_row[0]]
    pred = c[0] * (zt0 - want * c[1])
    assert torch.equal(zg, c[2] * zt0 + c[3] * pred)


# ------------------------------------------------------------------------------------- 3. Philox equals injection
@pytest.mark.parametrize("kind,B", [("A", 21), ("B", 9)])
def test_seeded_mode_is_the_injected_philox_streams(gpu_device, kind, B):
    """Seeded Q(x, cond_w) is bitwise the same sweep fed damc_philox_normal's materialised streams: 0x54 through
    prior_embedding as xemb_unc, and 0x53 (the sweep's in-kernel stream) as injected step noise."""
    from damc import amortizer
    from damc.langevin import philox_normal

    n, w, seed, base = 5, 0.5, 1234, 40
    Q = make_q(kind, n, gpu_device)
    x = images(B, gpu_device)
    zt0 = latent(B, Q.nz, gpu_device)
    with torch.no_grad():
        z_seeded = amortizer.q_forward(Q, x=x, cond_w=w, zt=zt0, seed=seed, chain_base=base)
        xemb = amortizer.encoder_forward(Q.encoder, x)
        pn = philox_normal(n, B, Q.nz, seed, gpu_device, step_offset=0, chain_base=base, stream_id=0x54)
        xemb_unc = amortizer.prior_embedding(Q, pn.view(n * B, Q.nz))
        noise = philox_normal(n - 1, B, Q.nz, seed, gpu_device, step_offset=0, chain_base=base, stream_id=0x53)
        z_inj = zt0.clone()
        amortizer.guided_sweep(Q, xemb, xemb_unc, z_inj, w, noise=noise)
    torch.cuda.synchronize()
    assert torch.isfinite(z_seeded).all() and not torch.equal(z_seeded, zt0)
    assert torch.equal(z_seeded, z_inj)


# -------------------------------------------------------------------------------------------------- 4. sharding
@pytest.mark.parametrize("kind", ["A", "B"])
def test_shards_reproduce_the_whole_batch(gpu_device, kind):
    """Seeded q_forward at B = 21 against its shards (zt slices, the global seed, chain_base = slice start): bitwise
    the whole batch's rows, with cuts on and off the 8-row tiles."""
    from damc import amortizer

    n, w, seed, B = 5, 0.5, 99, 21
    Q = make_q(kind, n, gpu_device)
    x = images(B, gpu_device)
    zt0 = latent(B, Q.nz, gpu_device)
    with torch.no_grad():
        whole = amortizer.q_forward(Q, x=x, cond_w=w, zt=zt0, seed=seed)
        for cuts in ([0, 5, 21], [0, 8, 16, 21]):
            parts = [amortizer.q_forward(Q, x=x[a:b].contiguous(), cond_w=w, zt=zt0[a:b], seed=seed, chain_base=a)
                     for a, b in zip(cuts[:-1], cuts[1:])]
            assert torch.equal(torch.cat(parts, 0), whole), cuts
    assert torch.isfinite(whole).all()


# ---------------------------------------------------------------------------------------------- 5. graph replay
def test_guided_sweep_replays_from_a_captured_graph(gpu_device):
    """One seeded guided_sweep call (explicit zt, pre-made xemb_unc) captured on a single stream after an eager
    warm-up: two replays from the restored zt are bitwise the eager result."""
    from damc import amortizer as am

    n, w, B = 5, 0.5, 21
    Q = make_q("B", n, gpu_device)
    xemb = latent(B, 64, gpu_device, seed=31)
    xemb_unc = latent(n * B, 64, gpu_device, seed=32).view(n, B, 64)
    zt0 = latent(B, Q.nz, gpu_device)
    ze = zt0.clone()
    am.guided_sweep(Q, xemb, xemb_unc, ze, w, seed=42)
    torch.cuda.synchronize()
    zg = zt0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        am.guided_sweep(Q, xemb, xemb_unc, zg.clone(), w, seed=42)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        am.guided_sweep(Q, xemb, xemb_unc, zg, w, seed=42)
    for _ in range(2):
        zg.copy_(zt0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(zg).all()
        assert torch.equal(zg, ze), "guided sweep differs between graph replay and eager"


# ------------------------------------------------------------------------------------------------------ 6. path
def test_seeded_guidance_is_one_library_call(gpu_device, monkeypatch):
    """Seeded Q(x, cond_w = 0.5) never enters the denoiser module's forward (the step loop's route) and makes
    exactly one damc_guided_sweep call."""
    from damc import _lib, amortizer

    Q = make_q("A", 5, gpu_device)
    x = images(9, gpu_device)
    L = _lib.lib()
    sweeps, forwards = [], []
    orig = L.damc_guided_sweep
    monkeypatch.setattr(L, "damc_guided_sweep", lambda *a: sweeps.append(1) or orig(*a))
    orig_fwd = Q.p.forward
    monkeypatch.setattr(Q.p, "forward", lambda *a, **k: forwards.append(1) or orig_fwd(*a, **k))
    with torch.no_grad():
        z = amortizer.q_forward(Q, x=x, cond_w=0.5, seed=5)
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and z.shape == (9, Q.nz)
    assert forwards == [] and sweeps == [1]


# ----------------------------------------------------------------------------------------------------- 7. edges
@pytest.mark.parametrize("kind,B", [("A", 1), ("B", 1), ("A", 9)])
def test_edges(gpu_device, kind, B):
    """eps_log_steps = n gives n finite eps tensors; two runs of a seed are bitwise equal, another seed differs;
    B = 1."""
    from damc import amortizer

    n, w = 5, 2.0
    Q = make_q(kind, n, gpu_device)
    x = images(B, gpu_device)
    zt0 = latent(B, Q.nz, gpu_device)
    with torch.no_grad():
        xemb = amortizer.encoder_forward(Q.encoder, x)
        xemb_unc = amortizer.prior_embedding(Q, latent(n * B, Q.nz, gpu_device, seed=33))
        z = zt0.clone()
        eps = amortizer.guided_sweep(Q, xemb, xemb_unc, z, w, seed=3, eps_log_steps=n)
        assert eps.shape == (n, B, Q.nz) and torch.isfinite(eps).all() and torch.isfinite(z).all()
        za = amortizer.q_forward(Q, x=x, cond_w=w, zt=zt0, seed=11)
        zb = amortizer.q_forward(Q, x=x, cond_w=w, zt=zt0, seed=11)
        zc = amortizer.q_forward(Q, x=x, cond_w=w, zt=zt0, seed=12)
    assert za.shape == (B, Q.nz) and torch.isfinite(za).all()
    assert torch.equal(za, zb)
    assert not torch.equal(za, zc)
