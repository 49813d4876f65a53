"""GPU parity: the amortizer Q on the HIP path (encoder + prior embedding + reverse sweep) vs the
reference's golden vectors and the fp64 oracle (workspace/src/diffusion_net.py:227-622).

Tolerances: encoder xemb rel-L2 <= 1e-5 and eps of the first reverse step <= 1e-5 against the golden.  Later
steps amplify rounding by sqrt(1+e^-l) per step, and the reference's own fp32 result is already up to 2.4e-4
(step 3) / 8e-2 (end of a 10-step sweep) / 1e-2 (100 steps) away from an fp64 evaluation of the same sweep
(printed by these tests), so eps of steps 2-3 and the sweep end-point are judged accuracy-relative: the HIP
result's distance to the fp64 oracle must stay within 3x the reference golden's distance to it (+ a 1e-5 /
1e-6 floor).  The golden itself is still bounded by conftest.Q_END_TOL.
"""
import numpy as np
import pytest
import torch

from conftest import Q_END_TOL, Q_NAMES, build_q_case, rel_l2

pytestmark = pytest.mark.gpu

_FP64 = {}


def fp64_sweeps(name):
    """fp64 oracle: eps of steps 1-3 and the end-point of the posterior sweep (Q(x)) and the prior sweep
    (Q(x=None) on the case's prior-embedding noise), cached per case."""
    if name not in _FP64:
        from oracle import damc_oracle as orc

        c = build_q_case(name)
        Q, m = c["Q"].double(), c["meta"]
        args = (m["n_interval"], m["logsnr_min"], m["logsnr_max"], m["var_type"])
        with torch.no_grad():
            xemb = orc.encoder_forward(Q.encoder, c["x"].double())
            zp, ep = orc.reverse_sweep(Q, xemb, c["zt0"].double(), c["eps"].double(), *args)
            pe = orc.prior_embedding(Q, c["pe_noise"].double())
            zq, eq = orc.reverse_sweep(Q, pe, c["zt0"].double(), c["eps"].double(), *args)
        _FP64[name] = dict(post=zp.numpy(), post_eps=[e.numpy() for e in ep[:3]], prior=zq.numpy(),
                           prior_eps=[e.numpy() for e in eq[:3]])
    return _FP64[name]


@pytest.fixture(scope="module")
def am(gpu_device):
    from damc import amortizer

    return amortizer


@pytest.mark.parametrize("name", Q_NAMES)
def test_encoder_matches_reference(am, gpu_device, name):
    c = build_q_case(name, gpu_device)
    xemb = am.encoder_forward(c["Q"].encoder, c["x"])
    assert rel_l2(xemb.cpu().numpy(), c["rec"]["xemb"]) < 1e-5


def _check_sweep(name, eps, zt, rec_eps, rec_end, ref_eps, ref_end, nsteps):
    assert rel_l2(eps[0], rec_eps[0]) < 1e-5
    for k in range(1, nsteps):
        e_hip, e_ref = rel_l2(eps[k], ref_eps[k]), rel_l2(rec_eps[k], ref_eps[k])
        print("%s eps step %d: |hip-fp64| %.2e  |reference-fp64| %.2e" % (name, k + 1, e_hip, e_ref))
        assert e_hip <= 3 * e_ref + 1e-5, k
    e_hip, e_ref = rel_l2(zt, ref_end), rel_l2(rec_end, ref_end)
    print("%s sweep end: |hip-fp64| %.2e  |reference-fp64| %.2e  |hip-reference| %.2e"
          % (name, e_hip, e_ref, rel_l2(zt, rec_end)))
    assert e_hip <= 3 * e_ref + 1e-6
    assert rel_l2(zt, rec_end) < Q_END_TOL[name]


@pytest.mark.parametrize("name", Q_NAMES)
def test_posterior_sweep_matches_reference(am, gpu_device, name):
    c = build_q_case(name, gpu_device)
    Q, rec = c["Q"], c["rec"]
    ref = fp64_sweeps(name)
    xemb = am.encoder_forward(Q.encoder, c["x"])
    zt = c["zt0"].clone()
    eps = am.reverse_sweep(Q, xemb, zt, noise=c["eps"], eps_log_steps=3).cpu().numpy()
    _check_sweep(name, eps, zt.cpu().numpy(), rec["q_post_eps3"], rec["q_post"], ref["post_eps"], ref["post"], 3)


@pytest.mark.parametrize("name", Q_NAMES)
def test_prior_sweep_matches_reference(am, gpu_device, name):
    c = build_q_case(name, gpu_device)
    Q, rec = c["Q"], c["rec"]
    ref = fp64_sweeps(name)
    xemb = am.prior_embedding(Q, c["pe_noise"])
    zt = c["zt0"].clone()
    eps = am.reverse_sweep(Q, xemb, zt, noise=c["eps"], eps_log_steps=1).cpu().numpy()
    _check_sweep(name, eps, zt.cpu().numpy(), rec["q_prior_eps3"], rec["q_prior"], ref["prior_eps"], ref["prior"], 1)


@pytest.mark.parametrize("name,B", [("q_cifar10_s", 4), ("q_svhn_s", 3), ("q_cifar10_s", 37), ("q_svhn_s", 150)])
def test_shape_specialised_team_kernel_is_bitwise_the_generic(am, gpu_device, monkeypatch, name, B):
    """sweep_fast_kernel<NZ, 128> (the default at the reference's nf = 4, nz 128 / 100) against the generic team
    kernel (DAMC_SWEEP_FAST=0): the same fragments and MFMA order, so zt and the logged eps are bitwise equal, for a
    ragged last row tile (B=37) and teams with more than one row tile (B=150 on 8 teams), Philox noise and in-kernel
    eps logging."""
    from damc import synth

    c = build_q_case(name, gpu_device)
    Q = c["Q"]
    nz, nx = Q.nz, Q.nxemb
    xemb = torch.from_numpy(synth.normal_f32(71, 0, (B, nx))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(72, 0, (B, nz))).to(gpu_device)
    out = {}
    for fast in ("1", "0"):
        monkeypatch.setenv("DAMC_SWEEP_FAST", fast)
        zt = zt0.clone()
        eps = am.reverse_sweep(Q, xemb, zt, seed=17, eps_log_steps=2)
        torch.cuda.synchronize()
        out[fast] = (zt.cpu().numpy(), eps.cpu().numpy())
    assert np.isfinite(out["1"][0]).all()
    assert np.array_equal(out["1"][0], out["0"][0])
    assert np.array_equal(out["1"][1], out["0"][1])


def test_denoise_step_vs_oracle_at_baseline_width(am, gpu_device):
    """Full-width CIFAR Q (nxemb=1024, ntemb=128) at B=128: first reverse step eps vs the fp32 oracle."""
    from damc import synth
    from oracle import damc_oracle as orc
    from src import diffusion_net as dn

    Q = dn._netQ_U(nc=3, nz=128, nxemb=1024, ntemb=128, nif=64, diffusion_residual=True, n_interval=100,
                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Q, 20)
    Q.to(gpu_device).eval()
    B = 128
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 3, 32, 32))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(6, 0, (B, 128))).to(gpu_device)
    xemb = am.encoder_forward(Q.encoder, x)
    with torch.no_grad():
        xref = orc.encoder_forward(Q.encoder.cpu(), x.cpu())
        Q.to(gpu_device)
    assert rel_l2(xemb.cpu().numpy(), xref.numpy()) < 1e-5
    zt = zt0.clone()
    noise = torch.zeros(99, B, 128, device=gpu_device)
    eps = am.reverse_sweep(Q, xemb, zt, noise=noise, eps_log_steps=1)
    Qc = Q.cpu()
    with torch.no_grad():
        lt = orc.logsnr_schedule(torch.full((B,), 1.0), -5.1, 9.8)
        eref = orc.denoiser_forward(Qc.p, zt0.cpu(), lt, xemb.cpu())
    assert rel_l2(eps[0].cpu().numpy(), eref.numpy()) < 1e-5


def test_dropin_q_forward(gpu_device):
    """_netQ_U.forward keeps the reference contract: Q(x) and Q(x=None, b, device) -> (b, nz)."""
    from damc import synth
    from src import MCMC
    from src import diffusion_net as dn

    Q = dn._netQ_U(nc=3, nz=128, nxemb=64, ntemb=32, nif=8, diffusion_residual=True, n_interval=10,
                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Q, 20)
    Q.to(gpu_device).eval()
    x = torch.rand(5, 3, 32, 32, device=gpu_device) * 2 - 1
    with torch.no_grad():
        z = Q(x)
        zp = Q(x=None, b=7, device=gpu_device)
    assert z.shape == (5, 128) and zp.shape == (7, 128)
    assert torch.isfinite(z).all() and torch.isfinite(zp).all()
    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=16, nc=3), 0).to(gpu_device)
    xs, zs = MCMC.gen_samples_with_diffusion_prior(b=6, device=gpu_device, netQ=Q, netG=G)
    assert xs.shape == (6, 3, 32, 32) and zs.shape == (6, 128)


def _wide_q(gpu_device, n_interval):
    from damc import synth
    from src import diffusion_net as dn

    Q = dn._netQ_U(nc=3, nz=128, nxemb=1024, ntemb=128, nif=64, diffusion_residual=True, n_interval=n_interval,
                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Q, 20)
    return Q.to(gpu_device).eval()


@pytest.mark.parametrize("B", [1, 37, 128, 300, 600])
def test_team_sweep_matches_launch_chain(am, gpu_device, monkeypatch, B):
    """The one-launch team sweep (default) against the per-block launch chain (DAMC_SWEEP_TEAM=0) at full CIFAR
    width: B=300 gives teams 2-3 row tiles, B=37 a ragged last tile, B=1 one active team, B=600 puts B*nz past
    the setup kernel's capped thread count (z rows past thread 65536 must still be copied).  The two differ only in
    the order of the K sum of the skip blocks, so eps of step 1 agrees to rel-L2 1e-6 and of step 2 to 1e-5; a
    10-step sweep amplifies fp32 rounding far beyond that, so the end point is judged
    against the fp64 oracle on the same injected noise: the team's distance within 3x the chain's (+1e-6)."""
    from damc import synth
    from oracle import damc_oracle as orc

    n = 10
    Q = _wide_q(gpu_device, n)
    xemb = torch.from_numpy(synth.normal_f32(7, 0, (B, 1024))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(8, 0, (B, 128))).to(gpu_device)
    noise = torch.from_numpy(synth.normal_f32(9, 0, (n - 1, B, 128))).to(gpu_device)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DAMC_SWEEP_TEAM", mode)
        zt = zt0.clone()
        eps = am.reverse_sweep(Q, xemb, zt, noise=noise, eps_log_steps=2)
        torch.cuda.synchronize()
        res[mode] = (zt.cpu().numpy(), eps.cpu().numpy())
    (zt_t, eps_t), (zt_c, eps_c) = res["1"], res["0"]
    Qd = Q.cpu().double()
    with torch.no_grad():
        z64, _ = orc.reverse_sweep(Qd, xemb.cpu().double(), zt0.cpu().double(), noise.cpu().double(), n, -5.1, 9.8,
                                   "large")
    z64 = z64.numpy()
    e_t, e_c = rel_l2(zt_t, z64), rel_l2(zt_c, z64)
    print("B=%d team vs chain: eps1 %.2e eps2 %.2e; end |team-fp64| %.2e |chain-fp64| %.2e"
          % (B, rel_l2(eps_t[0], eps_c[0]), rel_l2(eps_t[1], eps_c[1]), e_t, e_c))
    assert np.isfinite(zt_t).all()
    assert rel_l2(eps_t[0], eps_c[0]) <= 1e-6
    assert rel_l2(eps_t[1], eps_c[1]) <= 1e-5
    assert e_t <= 3 * e_c + 1e-6
    tail = slice(min(B, 512), B)  # rows whose z lies past the setup grid's first 65536 threads
    if B > 512:
        assert rel_l2(zt_t[tail], z64[tail]) <= 3 * rel_l2(zt_c[tail], z64[tail]) + 1e-6
        # the tail rows as close to fp64 as the head rows (a 10-step sweep sits ~4e-2 from fp64 in fp32 either way;
        # uninitialised rows would sit at ~1)
        assert rel_l2(zt_c[tail], z64[tail]) <= 3 * rel_l2(zt_c[:512], z64[:512])


def test_team_sweep_is_deterministic(am, gpu_device):
    """Fixed-order reductions everywhere: two team sweeps of the same inputs are bitwise equal."""
    from damc import synth

    Q = _wide_q(gpu_device, 20)
    xemb = torch.from_numpy(synth.normal_f32(7, 0, (128, 1024))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(8, 0, (128, 128))).to(gpu_device)
    out = []
    for _ in range(2):
        zt = zt0.clone()
        am.reverse_sweep(Q, xemb, zt, seed=99)
        out.append(zt.cpu().numpy())
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("B", [37, 128])
def test_limb_hyper_gemms_vs_fp32_engine(am, gpu_device, monkeypatch, B):
    """The hyper GEMMs on the limb product (sweep_stages.hip hyper_x3_kernel, round 5: the PyTorch Wg / Wb rows read as
    fp32 and split in the kernel) against the fp32-MFMA grouped launch (DAMC_SWEEP_HYPER=fp32): the first step's eps
    agrees to rel-L2 1e-5, and a 10-step sweep's end point is as close to the fp64 oracle (same injected noise): within
    3x the fp32 engine's distance (+1e-6).  B=37 leaves a partial 128-row tile in every block."""
    from damc import synth
    from oracle import damc_oracle as orc

    n = 10
    Q = _wide_q(gpu_device, n)
    xemb = torch.from_numpy(synth.normal_f32(7, 1, (B, 1024))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(8, 1, (B, 128))).to(gpu_device)
    noise = torch.from_numpy(synth.normal_f32(9, 1, (n - 1, B, 128))).to(gpu_device)
    res = {}
    for mode in ("limb", "fp32"):
        monkeypatch.setenv("DAMC_SWEEP_HYPER", mode)
        zt = zt0.clone()
        eps = am.reverse_sweep(Q, xemb, zt, noise=noise, eps_log_steps=1)
        torch.cuda.synchronize()
        res[mode] = (zt.cpu().numpy(), eps.cpu().numpy())
    with torch.no_grad():
        z64, _ = orc.reverse_sweep(Q.cpu().double(), xemb.cpu().double(), zt0.cpu().double(), noise.cpu().double(), n,
                                   -5.1, 9.8, "large")
    z64 = z64.numpy()
    e_l, e_f = rel_l2(res["limb"][0], z64), rel_l2(res["fp32"][0], z64)
    d1 = rel_l2(res["limb"][1][0], res["fp32"][1][0])
    print("B=%d eps1 limb vs fp32 %.2e; end |limb-fp64| %.2e |fp32-fp64| %.2e" % (B, d1, e_l, e_f))
    assert np.isfinite(res["limb"][0]).all()
    assert d1 <= 1e-5
    assert e_l <= 3 * e_f + 1e-6


@pytest.mark.gpu
def test_grouped_hyper_gemms_are_bitwise_the_separate_launches(am, gpu_device, monkeypatch):
    """The seven hyper GEMMs on the fp32-MFMA engine (DAMC_SWEEP_HYPER=fp32) run as one grouped launch; the same tiles
    as seven launches, bit for bit."""
    from damc import synth

    monkeypatch.setenv("DAMC_SWEEP_HYPER", "fp32")
    Q = _wide_q(gpu_device, 20)
    xemb = torch.from_numpy(synth.normal_f32(7, 0, (128, 1024))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(8, 0, (128, 128))).to(gpu_device)
    out = []
    for grouped in ("1", "0"):
        monkeypatch.setenv("DAMC_SWEEP_HYPER_GROUP", grouped)
        zt = zt0.clone()
        am.reverse_sweep(Q, xemb, zt, seed=99)
        out.append(zt.cpu().numpy())
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[0], out[1])


def test_failed_team_launch_is_rescued_bitwise(am, gpu_device, monkeypatch):
    """A team member that never becomes resident makes the bounded waits give up (forced here: every wait fails
    at once).  The sweep is then recomputed on the device by team_finish_kernel with the team's own arithmetic:
    the result is bitwise the healthy team sweep (no NaN), eps_log included, and the failure is reported to the
    host (damc_sweep_team_failures) at the next sweep."""
    from damc import _lib, synth

    Q = _wide_q(gpu_device, 12)
    xemb = torch.from_numpy(synth.normal_f32(7, 0, (37, 1024))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(8, 0, (37, 128))).to(gpu_device)
    L = _lib.lib()
    dev = gpu_device.index or 0
    zt = zt0.clone()
    eps = am.reverse_sweep(Q, xemb, zt, seed=5, eps_log_steps=3)
    torch.cuda.synchronize()
    before = L.damc_sweep_team_failures(dev)
    monkeypatch.setenv("DAMC_SWEEP_TEAM_KEEP", "1")
    monkeypatch.setenv("DAMC_SWEEP_FORCE_FAIL", "1")
    zr = zt0.clone()
    epr = am.reverse_sweep(Q, xemb, zr, seed=5, eps_log_steps=3)
    torch.cuda.synchronize()
    monkeypatch.delenv("DAMC_SWEEP_FORCE_FAIL")
    assert torch.isfinite(zr).all()
    assert torch.equal(zr, zt), "the rescued sweep differs from the team sweep"
    assert torch.equal(epr, eps)
    assert L.damc_sweep_team_failures(dev) == before + 1
    zt2 = zt0.clone()  # the team launch is still used (DAMC_SWEEP_TEAM_KEEP) and healthy again
    am.reverse_sweep(Q, xemb, zt2, seed=5)
    torch.cuda.synchronize()
    assert torch.equal(zt2, zt)
    assert L.damc_sweep_team_failures(dev) == before + 1


def test_classifier_free_guidance_matches_stock_modules(gpu_device):
    """Q(x, cond_w=w > 0) (diffusion_net.py:603-606; round 5): the guided step loop with its denoiser evaluations on
    libdamc, against the reference's loop on the stock modules in fp32 and in fp64, every run from the same torch seed
    (zt on the host generator, the per-step prior-embedding and step noise on the device, drawn in fp32 in the
    reference's order).  The guided chain amplifies rounding (the 1 + w weighting and pred_x_from_eps's
    sqrt(1 + e^-logsnr) ~ 13 at logsnr_min), so the HIP end point is held to the fp32 reference's own distance from
    fp64: within 3x of it (+1e-6), as the sweep tests do.  That loose end-point bound is anchored at the first step:
    its guided eps (both denoiser evaluations and the 1 + w combination, before any amplification) is held to 1e-5
    of the stock fp32 modules' on the same draws."""
    import copy

    from damc import synth, training
    from src import diffusion_helper_func as dh
    from src import diffusion_net as dn

    Q = dn._netQ_U(nc=3, nz=128, nxemb=1024, ntemb=128, nif=64, diffusion_residual=True, n_interval=10,
                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Q, 20)
    Q.to(gpu_device).eval()
    x = torch.from_numpy(synth.uniform_f32(93, 0, (16, 3, 32, 32))).to(gpu_device)
    w = 0.5
    from damc import amortizer

    torch.manual_seed(7)
    eps_hip = []
    with torch.no_grad():
        z_hip = amortizer._q_forward_guided(Q, x, w, eps_trace=eps_hip)
    torch.manual_seed(7)
    with torch.no_grad():
        assert torch.equal(Q(x, cond_w=w), z_hip)  # the module's forward is this path, draw for draw

    def reference(Qm, dt, eps_trace=None):  # diffusion_net.py:585-622 on stock modules in dtype dt, fp32 draws
        b, n = len(x), Qm.n_interval
        xemb = Qm.encoder(x.to(dt))
        zt = torch.randn(b, Qm.nz).to(gpu_device).to(dt)
        for i in reversed(range(0, n)):
            it = torch.ones(b, dtype=dt).to(gpu_device) * float(i)
            lt = dh.logsnr_schedule_fn(it / (n - 1.0), logsnr_min=Qm.logsnr_min, logsnr_max=Qm.logsnr_max)
            ls = dh.logsnr_schedule_fn(torch.clamp(it - 1.0, min=0.0) / (n - 1.0), logsnr_min=Qm.logsnr_min,
                                       logsnr_max=Qm.logsnr_max)
            e = Qm.p(z=zt, logsnr=lt, xemb=xemb)
            eu = Qm.p(z=zt, logsnr=lt, xemb=Qm.prior_emb(torch.randn(b, Qm.nz, device=gpu_device).to(dt)))
            e = (1 + w) * e - w * eu
            if eps_trace is not None:
                eps_trace.append(e.clone())
            lt, ls = lt.reshape((b, 1)), ls.reshape((b, 1))
            pz = dh.pred_x_from_eps(z=zt, eps=e, logsnr=lt)
            if i == 0:
                zt = pz
            else:
                d = dh.diffusion_reverse(x=pz, z_t=zt, logsnr_s=ls, logsnr_t=lt, pred_var_type=Qm.var_type)
                zt = d["mean"] + d["std"] * torch.randn(zt.shape, device=gpu_device).to(dt)
        return zt.double()

    with training.stock_pytorch(), torch.no_grad():
        torch.manual_seed(7)
        eps32 = []
        z32 = reference(Q, torch.float32, eps32)
        torch.manual_seed(7)
        z64 = reference(copy.deepcopy(Q).double(), torch.float64)
    d_hip = rel_l2(z_hip.double().cpu().numpy(), z64.cpu().numpy())
    d_ref = rel_l2(z32.cpu().numpy(), z64.cpu().numpy())
    print("guided Q(x) end point vs fp64: HIP %.2e, stock fp32 %.2e; HIP vs stock fp32 %.2e"
          % (d_hip, d_ref, rel_l2(z_hip.double().cpu().numpy(), z32.cpu().numpy())))
    e1 = rel_l2(eps_hip[0].double().cpu().numpy(), eps32[0].double().cpu().numpy())
    print("guided eps of step 1, HIP vs stock fp32: %.2e" % e1)
    assert len(eps_hip) == len(eps32) == Q.n_interval and e1 <= 1e-5
    assert torch.isfinite(z_hip).all() and d_hip <= 3 * d_ref + 1e-6
