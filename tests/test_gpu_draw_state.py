"""GPU: every drawn (draws= / _ds) entry point is bitwise the seeded one at seed = state.seed and offset = host offset +
state.counter, at counters 0, 7 and 2^32 + 3, with a nonzero host offset and a seed above 2^32.

The 16-byte state sits between guard words (dp_util.guarded): after every call the guards and the seed word are
untouched, and the counter is what the wrapper's contract says (advanced by n_steps / n_interval / 1 by the high-level
wrappers, left alone by the per-op hooks).  The last test captures a Langevin block with draws= and replays it: replay k
is the eager seeded call at offsets 2k / 3k, consecutive replays differ, and the counters read back as 3 x n_steps."""
import types

import pytest
import torch

import dp_util
from conftest import build_q_case, load_golden
from toyq_util import build_toy_case

pytestmark = pytest.mark.gpu

COUNTERS = [0, 7, 2 ** 32 + 3]
SEED = 2 ** 40 + 0x1234567  # above 2^32: the key's high word is live
OFF = 5                     # the host offset every case adds to the counter
BASE = 2 ** 32 + 11         # chain_base past 2^32 too


def _state(device, counter):
    """(guarded buffer, DrawState on the 16 bytes in its middle)."""
    from damc import graphs

    whole, view = dp_util.guarded(4, device)
    return whole, graphs.DrawState(SEED, device, counter, words=view.view(torch.int64))


def _state_ok(whole, ds, counter):
    torch.cuda.synchronize()
    assert dp_util.guards_intact(whole), "a drawn call wrote outside the 16-byte state"
    assert ds.read() == (SEED, counter), "seed word changed, or the counter is not what the wrapper promises"


_NETS = {}


def _nets(kind, device):
    """cifar: _netG_cifar10(nz=128, ngf=16) + _netE; svhn: the nz = 100 topology (SVHN w16) + _netE(100); toy: ToyG,
    no EBM.  Built once."""
    if kind not in _NETS:
        from damc import synth, toy
        from src import diffusion_net as dn

        if kind == "cifar":
            G, E, xs = dn._netG_cifar10(nz=128, ngf=16, nc=3), dn._netE(nz=128), (3, 32, 32)
        elif kind == "svhn":
            G, E, xs = dn._netG_svhn(nz=100, ngf=16, nc=3), dn._netE(nz=100), (3, 32, 32)
        else:
            G, E, xs = toy.ToyG(), None, (2,)
        synth.load_into(G, 0)
        G.to(device).eval()
        if E is not None:
            synth.load_into(E, 10)
            E.to(device).eval()
        _NETS[kind] = (G, E, xs)
    return _NETS[kind]


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("kind,B", [("cifar", 8), ("svhn", 8), ("toy", 16)])
def test_posterior_langevin_draws(gpu_device, kind, B, counter):
    """Which update kernel each case reaches (csrc/ebm.hip, damc_launch_posterior_update's two branches):
    cifar (nz 128, nh 200): ebm_reg_kernel<EB_POSTERIOR>, fused with the slab sum and the limb copy of z (nz % 8 == 0);
    svhn (nz 100): ebm_reg_kernel<EB_POSTERIOR> without the limb copy (nz % 8 != 0), slabs summed by the kernel;
    toy (ToyG, no EBM): posterior_update_kernel<2>, the streaming kernel every non-register shape takes."""
    from damc import langevin as lv
    from damc import synth

    G, E, xs = _nets(kind, gpu_device)
    nz = 2 if kind == "toy" else (128 if kind == "cifar" else 100)
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B,) + xs)).to(gpu_device)
    z0 = torch.from_numpy(synth.normal_f32(2, 0, (B, nz))).to(gpu_device)
    sigma = 0.25 if kind == "toy" else 0.1
    ze = z0.clone()
    lv.posterior_langevin(ze, x, G, E, 3, sigma, 0.1, True, seed=SEED, step_offset=OFF + counter, chain_base=BASE)
    whole, ds = _state(gpu_device, counter)
    zd = z0.clone()
    lv.posterior_langevin(zd, x, G, E, 3, sigma, 0.1, True, step_offset=OFF, chain_base=BASE, draws=ds)
    _state_ok(whole, ds, counter + 3)
    assert torch.isfinite(ze).all() and not torch.equal(ze, z0)
    assert torch.equal(zd, ze)
    # the noise really is keyed by the counter
    zo = z0.clone()
    lv.posterior_langevin(zo, x, G, E, 3, sigma, 0.1, True, seed=SEED, step_offset=OFF + counter + 1, chain_base=BASE)
    assert not torch.equal(zo, ze)


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("engine", ["valu", "mfma"])
def test_prior_langevin_draws(gpu_device, engine, counter):
    """B = 16 on the register engine (ebm_reg_kernel<EB_PRIOR>), B = mfma_min_chains() on the MFMA engine
    (prior_chain_mfma_kernel): "auto" resolves to exactly these."""
    from damc import langevin as lv
    from damc import synth

    _, E, _ = _nets("cifar", gpu_device)
    B = 16 if engine == "valu" else lv.mfma_min_chains()
    z0 = torch.from_numpy(synth.normal_f32(3, 0, (B, 128))).to(gpu_device)
    ze = z0.clone()
    lv.prior_langevin(ze, E, 3, 0.4, True, seed=SEED, step_offset=OFF + counter, chain_base=BASE, engine=engine)
    whole, ds = _state(gpu_device, counter)
    zd = z0.clone()
    lv.prior_langevin(zd, E, 3, 0.4, True, step_offset=OFF, chain_base=BASE, engine="auto", draws=ds)
    _state_ok(whole, ds, counter + 3)
    assert torch.isfinite(ze).all() and torch.equal(zd, ze)


def test_prior_langevin_streaming_kernel_draws(gpu_device):
    """An EBM wider than the register kernel holds (ndf = 256 > 208) on the "valu" engine runs the streaming
    prior_chain_kernel<2>, the third kernel the prior dispatcher can pick; B = 5 leaves its last workgroup one row."""
    from damc import langevin as lv
    from damc import synth
    from src import diffusion_net as dn

    E = synth.load_into(dn._netE(nz=128, ndf=256), 10).to(gpu_device).eval()
    z0 = torch.from_numpy(synth.normal_f32(3, 0, (5, 128))).to(gpu_device)
    ze = z0.clone()
    lv.prior_langevin(ze, E, 2, 0.4, True, seed=SEED, step_offset=OFF + 7, chain_base=BASE, engine="valu")
    whole, ds = _state(gpu_device, 7)
    zd = z0.clone()
    lv.prior_langevin(zd, E, 2, 0.4, True, step_offset=OFF, chain_base=BASE, engine="valu", draws=ds)
    _state_ok(whole, ds, 9)
    assert torch.isfinite(ze).all() and torch.equal(zd, ze)


@pytest.mark.parametrize("counter", COUNTERS)
def test_z_update_and_philox_draws(gpu_device, counter):
    from damc import _lib
    from damc import langevin as lv
    from damc import synth

    B, nz = 37, 128
    whole, ds = _state(gpu_device, counter)
    for sid in (_lib.STREAM_POSTERIOR, _lib.STREAM_QPE):
        want = lv.philox_normal(2, B, nz, SEED, gpu_device, step_offset=OFF + counter, chain_base=BASE, stream_id=sid)
        got = lv.philox_normal(2, B, nz, device=gpu_device, step_offset=OFF, chain_base=BASE, stream_id=sid, draws=ds)
        assert torch.equal(got, want)
    want = lv.philox_uniform(2, B, SEED, gpu_device, step_offset=OFF + counter, chain_base=BASE)
    got = lv.philox_uniform(2, B, device=gpu_device, step_offset=OFF, chain_base=BASE, draws=ds)
    assert torch.equal(got, want) and float(want.min()) >= 0.0 and float(want.max()) < 1.0
    z0 = torch.from_numpy(synth.normal_f32(4, 0, (B, nz))).to(gpu_device)
    g = torch.from_numpy(synth.normal_f32(5, 0, (B, nz))).to(gpu_device)
    ze, zd = z0.clone(), z0.clone()
    lv.z_update(ze, g, 0.3, True, seed=SEED, step_index=OFF + counter, chain_base=BASE)
    lv.z_update(zd, g, 0.3, True, step_index=OFF, chain_base=BASE, draws=ds)
    assert torch.equal(zd, ze) and not torch.equal(ze, z0)
    _state_ok(whole, ds, counter)  # the per-op hooks do not advance


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("B,nz,ntemb", [(5, 6, 128), (21, 128, 128)])
def test_glue_draws(gpu_device, B, nz, ntemb, counter):
    from damc import synth, training

    q = types.SimpleNamespace(logsnr_min=-5.1, logsnr_max=9.8, p=types.SimpleNamespace(ntemb=ntemb))
    z = torch.from_numpy(synth.normal_f32(71, B, (B, nz))).to(gpu_device)
    ue, le = torch.empty(B, device=gpu_device), torch.empty(B, device=gpu_device)
    ud, ld = torch.empty(B, device=gpu_device), torch.empty(B, device=gpu_device)
    want = training.q_noise_glue_seeded(q, z, SEED, OFF + counter, BASE, u_out=ue, logsnr_out=le)
    whole, ds = _state(gpu_device, counter)
    got = training.q_noise_glue_seeded(q, z, draw_index=OFF, chain_base=BASE, u_out=ud, logsnr_out=ld, draws=ds)
    _state_ok(whole, ds, counter)
    for a, b in zip(got + (ud, ld), want + (ue, le)):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def _small_cifar_q(device):
    """q_cifar10_s' amortizer (the small CIFAR Q) with n_interval = 4."""
    from damc import synth
    from src import diffusion_net as dn

    _, m = load_golden("q_cifar10_s")
    Q = dn._netQ_U(nc=m["nc"], nz=m["nz"], nxemb=m["nxemb"], ntemb=m["ntemb"], nif=m["nif"], diffusion_residual=True,
                   n_interval=4, logsnr_min=m["logsnr_min"], logsnr_max=m["logsnr_max"], var_type=m["var_type"],
                   with_noise=True, cond_w=0.0, net_arch="A", dataset=m["dataset"])
    synth.load_into(Q, 20)
    return Q.to(device).eval()


def _sweep_case(gpu_device, Q, B, counter):
    """The seeded sweep has no host offset, so its reference at a nonzero counter is the sweep fed the noise its own
    stream (0x53) holds at step_offset = counter -- bitwise the in-kernel draw, which counter 0 also checks against
    the seeded sweep itself."""
    from damc import _lib
    from damc import amortizer as am
    from damc import langevin as lv
    from damc import synth

    n = int(Q.n_interval)
    xemb = torch.from_numpy(synth.normal_f32(7, 0, (B, Q.nxemb))).to(gpu_device)
    zt0 = torch.from_numpy(synth.normal_f32(8, 0, (B, Q.nz))).to(gpu_device)
    noise = lv.philox_normal(n - 1, B, Q.nz, SEED, gpu_device, step_offset=counter, chain_base=BASE,
                             stream_id=_lib.STREAM_SWEEP)
    ze = zt0.clone()
    am.reverse_sweep(Q, xemb, ze, noise=noise, seed=0, chain_base=BASE)
    if counter == 0:
        zs = zt0.clone()
        am.reverse_sweep(Q, xemb, zs, seed=SEED, chain_base=BASE)
        assert torch.equal(zs, ze)
    whole, ds = _state(gpu_device, counter)
    zd = zt0.clone()
    am.reverse_sweep(Q, xemb, zd, chain_base=BASE, draws=ds)
    _state_ok(whole, ds, counter + n)
    assert torch.isfinite(ze).all() and not torch.equal(ze, zt0)
    assert torch.equal(zd, ze)


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("form", ["team", "chain", "rows"])
def test_reverse_sweep_draws(gpu_device, monkeypatch, form, counter):
    """team: the default team launch; chain: the launch chain (DAMC_SWEEP_TEAM=0) -- both read the state in
    sweep_setup_kernel; rows: the toy Q (nz = 2), whose row-resident kernel reads it itself."""
    if form == "rows":
        Q = build_toy_case("q_toy_driver", gpu_device)["Q"]
        assert Q.with_noise
        Q.n_interval = 4
    else:
        Q = _small_cifar_q(gpu_device)
        if form == "chain":
            monkeypatch.setenv("DAMC_SWEEP_TEAM", "0")
    _sweep_case(gpu_device, Q, 16, counter)


def test_q_forward_draws_is_the_seeded_q_forward(gpu_device):
    from damc import amortizer as am
    from damc import synth

    c = build_q_case("q_cifar10_s", gpu_device)
    Q, x = c["Q"], c["x"]
    zt0 = torch.from_numpy(synth.normal_f32(8, 0, (x.shape[0], Q.nz))).to(gpu_device)
    want = am.q_forward(Q, x=x, zt=zt0, seed=SEED, chain_base=BASE)
    whole, ds = _state(gpu_device, 0)
    got = am.q_forward(Q, x=x, zt=zt0, chain_base=BASE, draws=ds)
    _state_ok(whole, ds, int(Q.n_interval))
    assert torch.equal(got, want)


@pytest.mark.parametrize("which", ["q_cifar10_s", "q_toy"])
def test_calculate_loss_draws(gpu_device, which):
    """_netQ_U and _netQ_U_toy: calculate_loss(draws=) is calculate_loss(seed=, draw_index = OFF + counter), loss and
    every gradient, and the counter advances by 1 after the three draws."""
    from damc import synth

    c = build_q_case(which, gpu_device) if which != "q_toy" else build_toy_case(which, gpu_device)
    Q, x = c["Q"].train(), c["x"]
    B = x.shape[0]
    z = torch.from_numpy(synth.normal_f32(2, 0, (B, Q.nz))).to(gpu_device)
    mask = torch.ones(B, 1, device=gpu_device)
    mask[1::3] = 0.0

    def run(**kw):
        for p in Q.parameters():
            p.grad = None
        loss = Q.calculate_loss(x=x, z=z, mask=mask, chain_base=40, **kw)
        loss.mean().backward()
        return loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in Q.parameters()]

    for counter in (7, 2 ** 32 + 3):
        loss_s, grads_s = run(seed=SEED, draw_index=OFF + counter)
        whole, ds = _state(gpu_device, counter)
        loss_d, grads_d = run(draw_index=OFF, draws=ds)
        _state_ok(whole, ds, counter + 1)
        assert torch.isfinite(loss_s).all() and torch.equal(loss_d, loss_s)
        for a, b in zip(grads_d, grads_s):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def test_out_of_scope_forms_raise(gpu_device):
    """The guided sweep and train-mode spectral-norm chains refuse draws= (DamcError), before any launch."""
    from damc import _lib
    from damc import amortizer as am
    from damc import langevin as lv
    from src import diffusion_net as dn

    whole, ds = _state(gpu_device, 0)
    c = build_q_case("q_cifar10_s", gpu_device)
    with pytest.raises(_lib.DamcError):
        am.q_forward(c["Q"], x=c["x"], cond_w=1.0, draws=ds)
    E = dn._netE(nz=128, e_sn=True).to(gpu_device).train()
    with pytest.raises(_lib.DamcError):
        lv.prior_langevin(torch.zeros(4, 128, device=gpu_device), E, 2, 0.4, True, draws=ds)
    _state_ok(whole, ds, 0)


def test_captured_langevin_block_draws_anew_on_every_replay(gpu_device):
    """posterior (2 steps) + prior (3 steps) captured once with draws=: replay k is the eager seeded pair at step
    offsets 2k / 3k, consecutive replays differ, and after 3 replays the counters read 3 x n_steps."""
    from damc import graphs
    from damc import langevin as lv
    from damc import synth

    G, E, _ = _nets("cifar", gpu_device)
    B = 8
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 3, 32, 32))).to(gpu_device)
    z0 = torch.from_numpy(synth.normal_f32(2, 0, (B, 128))).to(gpu_device)
    p0 = torch.from_numpy(synth.normal_f32(3, 0, (16, 128))).to(gpu_device)
    wa, ds_post = _state(gpu_device, 0)
    wb, ds_prior = _state(gpu_device, 0)
    zg, pg = z0.clone(), p0.clone()

    def body():
        lv.posterior_langevin(zg, x, G, E, 2, 0.1, 0.1, True, draws=ds_post)
        lv.prior_langevin(pg, E, 3, 0.4, True, draws=ds_prior)

    graph = graphs.capture(body)  # the warm-up ran body once for real: put the counters back
    ds_post.set(SEED, 0)
    ds_prior.set(SEED, 0)
    prev = None
    for k in range(3):
        zg.copy_(z0)
        pg.copy_(p0)
        graph.replay()
        torch.cuda.synchronize()
        ze, pe = z0.clone(), p0.clone()
        lv.posterior_langevin(ze, x, G, E, 2, 0.1, 0.1, True, seed=SEED, step_offset=2 * k)
        lv.prior_langevin(pe, E, 3, 0.4, True, seed=SEED, step_offset=3 * k)
        assert torch.equal(zg, ze), "posterior replay %d is not the eager call at offset %d" % (k, 2 * k)
        assert torch.equal(pg, pe), "prior replay %d is not the eager call at offset %d" % (k, 3 * k)
        if prev is not None:
            assert not torch.equal(zg, prev[0]) and not torch.equal(pg, prev[1])
        prev = (zg.clone(), pg.clone())
    _state_ok(wa, ds_post, 6)
    _state_ok(wb, ds_prior, 9)
