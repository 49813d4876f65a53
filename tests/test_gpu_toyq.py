"""GPU parity of the toy amortizer (_netQ_U_toy, workspace/toy_example/src/diffusion_net.py:141-263) on the HIP path:
the fused MLP (encoder, prior_emb), the row-resident reverse sweep at nz = 2 and, forced by DAMC_SWEEP_ROWS=1, on the
existing CIFAR / SVHN goldens.

Tolerances are the project's: one fp32 forward (xemb, pe, step-1 eps) within 1e-5 rel-L2 of the golden; eps of steps
2-3 and the sweep end-point accuracy-relative, the HIP result's distance to the fp64 oracle within 3x the golden's own
distance to it plus 1e-5.  The toy sweep is well conditioned (the reference sits ~1e-6 from fp64), so for n accumulated
steps the single-forward tolerance is the floor, not 1e-6.  Every distance is printed.
"""
import numpy as np
import pytest
import torch

from conftest import build_q_case, rel_l2
from toyq_util import TOY_NAMES, build_toy_case, toy_fp64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def am(gpu_device):
    from damc import amortizer

    return amortizer


@pytest.fixture(autouse=True)
def no_team_rescue(gpu_device):
    """Nothing here may cost the team sweep a rescue (damc_sweep_team_failures unchanged by every test)."""
    from damc import _lib

    dev = gpu_device.index or 0
    before = _lib.lib().damc_sweep_team_failures(dev)
    yield
    torch.cuda.synchronize()
    assert _lib.lib().damc_sweep_team_failures(dev) == before


# ------------------------------------------------------------------------------- 1. encoder and prior embedding
@pytest.mark.parametrize("name", TOY_NAMES)
def test_mlp_encoder_and_prior_embedding_match_reference(am, gpu_device, name):
    c = build_toy_case(name, gpu_device)
    Q, rec = c["Q"], c["rec"]
    xemb = am.encoder_forward(Q.encoder, c["x"]).cpu().numpy()
    pe = am.prior_embedding(Q, c["pe_noise"]).cpu().numpy()
    x1 = am.encoder_forward(Q.encoder, c["x"][:1]).cpu().numpy()
    p1 = am.prior_embedding(Q, c["pe_noise"][:1]).cpu().numpy()
    d = (rel_l2(xemb, rec["xemb"]), rel_l2(pe, rec["pe"]), rel_l2(x1, rec["xemb"][:1]), rel_l2(p1, rec["pe"][:1]))
    print("%s xemb %.2e pe %.2e  B=1: xemb %.2e pe %.2e" % ((name,) + d))
    assert xemb.shape == rec["xemb"].shape and pe.shape == rec["pe"].shape
    assert max(d) < 1e-5
    # a row's result does not depend on its place in the 16-row tile
    assert np.array_equal(x1, xemb[:1]) and np.array_equal(p1, pe[:1])


# ------------------------------------------------------------------------------------------------- 2. the sweeps
def _check_toy_sweep(name, eps, zt, rec_eps, rec_end, ref_eps, ref_end, nsteps):
    e1 = rel_l2(eps[0], rec_eps[0])
    print("%s eps step 1: |hip-reference| %.2e" % (name, e1))
    assert e1 < 1e-5
    for k in range(1, nsteps):
        e_hip, e_ref = rel_l2(eps[k], ref_eps[k]), rel_l2(rec_eps[k], ref_eps[k])
        print("%s eps step %d: |hip-fp64| %.2e  |reference-fp64| %.2e" % (name, k + 1, e_hip, e_ref))
        assert e_hip <= 3 * e_ref + 1e-5, k
    e_hip, e_ref = rel_l2(zt, ref_end), rel_l2(rec_end, ref_end)
    print("%s sweep end: |hip-fp64| %.2e  |reference-fp64| %.2e  |hip-reference| %.2e"
          % (name, e_hip, e_ref, rel_l2(zt, rec_end)))
    assert np.isfinite(zt).all()
    assert e_hip <= 3 * e_ref + 1e-5


@pytest.mark.parametrize("name", TOY_NAMES)
def test_toy_posterior_sweep_matches_reference(am, gpu_device, name):
    c = build_toy_case(name, gpu_device)
    Q, rec, ref = c["Q"], c["rec"], toy_fp64(name)
    xemb = am.encoder_forward(Q.encoder, c["x"])
    zt = c["zt0"].clone()
    eps = am.reverse_sweep(Q, xemb, zt, noise=c["eps"], eps_log_steps=3).cpu().numpy()
    _check_toy_sweep(name + " post", eps, zt.cpu().numpy(), rec["q_post_eps3"], rec["q_post"], ref["post_eps"],
                     ref["post"], 3)


@pytest.mark.parametrize("name", TOY_NAMES)
def test_toy_prior_sweep_matches_reference(am, gpu_device, name):
    c = build_toy_case(name, gpu_device)
    Q, rec, ref = c["Q"], c["rec"], toy_fp64(name)
    xemb = am.prior_embedding(Q, c["pe_noise"])
    zt = c["zt0"].clone()
    eps = am.reverse_sweep(Q, xemb, zt, noise=c["eps"], eps_log_steps=3).cpu().numpy()
    _check_toy_sweep(name + " prior", eps, zt.cpu().numpy(), rec["q_prior_eps3"], rec["q_prior"], ref["prior_eps"],
                     ref["prior"], 3)


# ------------------------------------------------------------- 3. the row form on the goldens that already exist
@pytest.mark.parametrize("name", ["q_svhn_s", "q_cifar10_s"])
def test_row_form_on_existing_goldens(am, gpu_device, monkeypatch, name):
    """DAMC_SWEEP_ROWS=1 at nz = 100 (B 3) and nz = 128 (B 4): the criteria of the default path, unchanged
    (tests/test_gpu_amortizer.py _check_sweep against the golden and the fp64 oracle)."""
    from test_gpu_amortizer import _check_sweep, fp64_sweeps

    monkeypatch.setenv("DAMC_SWEEP_ROWS", "1")
    c = build_q_case(name, gpu_device)
    Q, rec, ref = c["Q"], c["rec"], fp64_sweeps(name)
    xemb = am.encoder_forward(Q.encoder, c["x"])
    zt = c["zt0"].clone()
    eps = am.reverse_sweep(Q, xemb, zt, noise=c["eps"], eps_log_steps=3).cpu().numpy()
    print("row form, posterior sweep:")
    _check_sweep(name, eps, zt.cpu().numpy(), rec["q_post_eps3"], rec["q_post"], ref["post_eps"],
                 ref["post"], 3)
    xemb = am.prior_embedding(Q, c["pe_noise"])
    zt = c["zt0"].clone()
    eps = am.reverse_sweep(Q, xemb, zt, noise=c["eps"], eps_log_steps=1).cpu().numpy()
    print("row form, prior sweep:")
    _check_sweep(name, eps, zt.cpu().numpy(), rec["q_prior_eps3"], rec["q_prior"], ref["prior_eps"],
                 ref["prior"], 1)


def test_row_form_matches_default_path_on_ragged_batch(am, gpu_device, monkeypatch):
    """q_cifar10_s' Q on a synthetic B = 37 (two full row tiles and a ragged one): the row form against the fp64
    oracle, held to what the default path achieves on the same inputs (step-1 eps within one fp32 forward of it; later
    eps and the end-point within 3x its distance to fp64, + 1e-5 / 1e-6 as in _check_sweep)."""
    from damc import synth
    from oracle import damc_oracle as orc

    c = build_q_case("q_cifar10_s", gpu_device)
    Q, m = c["Q"], c["meta"]
    B, n, nz = 37, m["n_interval"], m["nz"]
    xemb = torch.from_numpy(synth.normal_f32(71, 0, (B, m["nxemb"]))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(72, 0, (B, nz))).to(gpu_device)
    noise = torch.from_numpy(np.stack([synth.normal_f32(73, i, (B, nz)) for i in range(n - 1)])).to(gpu_device)
    res = {}
    for rows in ("0", "1"):
        monkeypatch.setenv("DAMC_SWEEP_ROWS", rows)
        zt = zt0.clone()
        eps = am.reverse_sweep(Q, xemb, zt, noise=noise, eps_log_steps=3)
        torch.cuda.synchronize()
        res[rows] = (zt.cpu().numpy(), eps.cpu().numpy())
    Qd = build_q_case("q_cifar10_s")["Q"].double()
    with torch.no_grad():
        z64, e64 = orc.reverse_sweep(Qd, xemb.cpu().double(), zt0.cpu().double(), noise.cpu().double(), n,
                                     m["logsnr_min"], m["logsnr_max"], m["var_type"])
    (zr, er), (zd, ed) = res["1"], res["0"]
    print("B=37 eps step 1: |rows-default| %.2e" % rel_l2(er[0], ed[0]))
    assert rel_l2(er[0], ed[0]) < 1e-5
    for k in (1, 2):
        a, b = rel_l2(er[k], e64[k].numpy()), rel_l2(ed[k], e64[k].numpy())
        print("B=37 eps step %d: |rows-fp64| %.2e  |default-fp64| %.2e" % (k + 1, a, b))
        assert a <= 3 * b + 1e-5
    a, b = rel_l2(zr, z64.numpy()), rel_l2(zd, z64.numpy())
    print("B=37 sweep end: |rows-fp64| %.2e  |default-fp64| %.2e" % (a, b))
    assert np.isfinite(zr).all()
    assert a <= 3 * b + 1e-6


# -------------------------------------------------------------------------------------------------- 4. sharding
def test_toy_sweep_shards_bitwise(am, gpu_device):
    """B = 37 with Philox noise: rows [0, 21) at chain_base 0 and rows [21, 37) at chain_base 21 are bitwise the full
    call's rows (a row's arithmetic and its noise depend on its global index only); a repeat is bitwise equal and
    another seed is not."""
    from damc import synth

    Q = build_toy_case("q_toy_driver", gpu_device)["Q"]
    B = 37
    xemb = torch.from_numpy(synth.normal_f32(71, 0, (B, Q.nxemb))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(72, 0, (B, Q.nz))).to(gpu_device)

    def run(lo, hi, seed=17):
        zt = zt0[lo:hi].clone()
        eps = am.reverse_sweep(Q, xemb[lo:hi].contiguous(), zt, seed=seed, chain_base=lo, eps_log_steps=2)
        torch.cuda.synchronize()
        return zt.cpu().numpy(), eps.cpu().numpy()

    zf, ef = run(0, B)
    assert np.isfinite(zf).all()
    za, ea = run(0, 21)
    zb, eb = run(21, B)
    assert np.array_equal(np.concatenate([za, zb]), zf)
    assert np.array_equal(np.concatenate([ea, eb], axis=1), ef)
    z2, e2 = run(0, B)
    assert np.array_equal(z2, zf) and np.array_equal(e2, ef)
    z3, _ = run(0, B, seed=18)
    assert not np.array_equal(z3, zf)


# ----------------------------------------------------------------------------------------------- 5. the drop-in
def test_dropin_toy_forward(am, gpu_device):
    """Q(x) and Q(x=None, b, device) through the drop-in with torch.randn patched (as conftest.qtrain_run patches
    it) equal the direct encoder / prior_embedding + reverse_sweep on the same draws, bit for bit."""
    c = build_toy_case("q_toy", gpu_device)  # the class defaults: no noise, so no Philox seed is drawn
    Q, zt0, pe_noise = c["Q"], c["zt0"], c["pe_noise"]
    B = zt0.shape[0]

    def patched(arrays):
        it = iter(arrays)
        return lambda *a, **k: next(it).clone().to(k.get("device") or "cpu")

    orig = torch.randn
    try:
        torch.randn = patched([zt0.cpu()])
        with torch.no_grad():
            z = Q(c["x"])
        torch.randn = patched([pe_noise.cpu(), zt0.cpu()])
        with torch.no_grad():
            zp = Q(x=None, b=B, device=gpu_device)
    finally:
        torch.randn = orig
    assert z.shape == zp.shape == (B, Q.nz)
    zt = zt0.clone()
    am.reverse_sweep(Q, am.encoder_forward(Q.encoder, c["x"]), zt)
    assert torch.equal(z, zt)
    zt = zt0.clone()
    am.reverse_sweep(Q, am.prior_embedding(Q, pe_noise), zt)
    assert torch.equal(zp, zt)


# ------------------------------------------------------------------------------------------------ 6. graph capture
def test_toy_q_replays_from_a_captured_graph(am, gpu_device):
    """The toy Q(x) at B = 21 (fused MLP encoder + row-resident sweep, Philox noise) recorded into a graph after one
    warm-up call: every replay is bitwise the eager call.  The initial latent is passed in (q_forward's zt): Q(x)'s
    own draw comes from the host generator, which a replay cannot repeat."""
    c = build_toy_case("q_toy_driver", gpu_device)
    Q, x, zt0 = c["Q"], c["x"], c["zt0"]
    with torch.no_grad():
        ze = am.q_forward(Q, x=x, zt=zt0, seed=42)
    torch.cuda.synchronize()
    zin = zt0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        am.q_forward(Q, x=x, zt=zin, seed=42)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        zg = am.q_forward(Q, x=x, zt=zin, seed=42)
    for _ in range(2):
        zin.copy_(zt0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(zg).all()
        assert torch.equal(zg, ze), "toy Q(x) differs between graph replay and eager"


# ---------------------------------------------------------------------------------------------------- 7. training
def test_toy_q_update_matches_reference(gpu_device):
    """calculate_loss(x, z, mask).mean().backward() of the toy Q against q_toy_qtrain, with the tolerances
    tests/test_gpu_training.py applies to the q_*_qtrain goldens: the loss within 1e-5; per tensor 1e-4 or twice the
    error of the reference's own ops on this GPU (stock PyTorch), whichever is larger."""
    from conftest import SEED_Z0, SEED_QT, gtrain_check, gtrain_errors, load_golden

    from damc import synth, training

    rec, meta = load_golden("q_toy_qtrain")

    def run():
        c = build_toy_case(meta["q"], gpu_device)
        Q, x, m = c["Q"], c["x"], c["meta"]
        B, nz = m["B"], m["nz"]
        Q.train()
        z = torch.from_numpy(synth.normal_f32(SEED_Z0, 0, (B, nz))).to(gpu_device)
        mask = torch.ones(B, 1, device=gpu_device)
        mask[1::3] = 0.0
        pe = synth.normal_f32(SEED_QT, 0, (B, nz))
        u = synth.uniform_f32(SEED_QT, 1, (B,), 0.0, 1.0)
        eps = synth.normal_f32(SEED_QT, 2, (B, nz))
        orig = torch.randn, torch.rand, torch.randn_like
        torch.randn = lambda *a, **k: torch.from_numpy(pe.copy()).to(k.get("device") or "cpu")
        torch.rand = lambda *a, **k: torch.from_numpy(u.copy())
        torch.randn_like = lambda t, **k: torch.from_numpy(eps.copy()).to(t.device)
        try:
            Q.zero_grad()
            loss = Q.calculate_loss(x=x, z=z, mask=mask)
            loss.mean().backward()
        finally:
            torch.randn, torch.rand, torch.randn_like = orig
        return loss.detach().cpu().numpy(), [p.grad.detach().cpu().numpy() for p in Q.parameters() if p.grad is not None]

    with training.stock_pytorch():
        _, g_stock = run()
    tol = [max(1e-4, 2.0 * max(e)) for e in gtrain_errors(g_stock, rec, meta)]
    loss, grads = run()
    print("toy Q update: loss %.2e" % rel_l2(loss, rec["loss"]))
    assert rel_l2(loss, rec["loss"]) < 1e-5
    worst = gtrain_check(grads, rec, meta, tol)
    print("toy Q update: worst rel err vs reference %.2e (largest bound %.2e)" % (worst, max(tol)))
