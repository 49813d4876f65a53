"""GPU capstone: a whole update -- zero_grad, loss forward, backward, clip + Adam step -- recorded into ONE graph and
replayed, against the same update run eagerly.

Q update: Q.calculate_loss(x, z, mask, draws=ds) draws from the device-resident key, so replay k is the eager seeded
update with draw_index = k; the G and E updates have no draws and replay on the parameters the previous replay left.
After the warm-up and the capture, parameters, moments, the step count and the draw counter are restored IN PLACE (the
graph holds their addresses); three replays then equal three eager updates bit for bit: every parameter, both moments
and `step`.  The eager side steps the same capturable optimiser class, so both sides run the same kernels.

A capture the runtime rejects raises a HIP error from torch.cuda.graph; nothing here retries."""
import pytest
import torch

from conftest import build_q_case

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 99
MAX_NORM = 1.0
N_UPDATES = 3


def _snapshot(params, opt):
    return ([p.detach().clone() for p in params],
            [opt.state[p]["exp_avg"].clone() for p in params if p in opt.state],
            [opt.state[p]["exp_avg_sq"].clone() for p in params if p in opt.state],
            [float(opt.state[p]["step"]) for p in params if p in opt.state])


def _replay_against_eager(params, make_opt, eager_update, make_body, reset_draws=None):
    """eager_update(opt, k) runs update k; make_body(opt) returns the captured body.  Returns nothing: asserts."""
    from damc import graphs

    start = [p.detach().clone() for p in params]
    opt = make_opt(params)
    for k in range(N_UPDATES):
        eager_update(opt, k)
    torch.cuda.synchronize()
    want = _snapshot(params, opt)
    assert all(torch.isfinite(p).all() for p in want[0])
    assert any(not torch.equal(a, b) for a, b in zip(want[0], start)), "the eager updates changed nothing"

    def restore(o):
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
            for st in o.state.values():
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
                st["step"].zero_()
        if reset_draws is not None:
            reset_draws()

    for p in params:
        p.grad = None
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
    cap = make_opt(params)
    if reset_draws is not None:
        reset_draws()
    graph = graphs.capture(make_body(cap))  # the warm-up ran one update for real
    restore(cap)
    for _ in range(N_UPDATES):
        graph.replay()
    torch.cuda.synchronize()
    got = _snapshot(params, cap)
    assert got[3] == want[3] and set(want[3]) == {float(N_UPDATES)}
    for name, a, b in (("parameter", got[0], want[0]), ("exp_avg", got[1], want[1]), ("exp_avg_sq", got[2], want[2])):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), "%s %d differs between %d replays and %d eager updates" % (name, i, N_UPDATES,
                                                                                                  N_UPDATES)


def test_q_update_replays_from_one_graph(gpu_device):
    from damc import graphs, synth
    from damc import optim as dopt

    c = build_q_case("q_cifar10_s", gpu_device)
    Q = c["Q"].train()
    B = 8
    m = c["meta"]
    # the golden case's own batch is smaller than 8: same recipe, B rows
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, m["nc"], m["H"], m["H"]))).to(gpu_device)
    z = torch.from_numpy(synth.normal_f32(2, 0, (B, Q.nz))).to(gpu_device)
    mask = torch.ones(B, 1, device=gpu_device)
    mask[1::3] = 0.0  # both values: encoder rows and prior-embedding rows
    params = [p for p in Q.parameters()]
    ds = graphs.DrawState(SEED, gpu_device)

    def make_opt(ps):
        return dopt.AdamW(ps, lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-4, capturable=True)

    def eager_update(opt, k):
        opt.zero_grad()
        Q.calculate_loss(x, z, mask, seed=SEED, draw_index=k).mean().backward()
        opt.clip_and_step(MAX_NORM)

    def make_body(opt):
        def body():
            opt.zero_grad()
            Q.calculate_loss(x, z, mask, draws=ds).mean().backward()
            opt.clip_and_step(MAX_NORM)
        return body

    _replay_against_eager(params, make_opt, eager_update, make_body, reset_draws=lambda: ds.set(SEED, 0))
    assert ds.read() == (SEED, N_UPDATES)


def test_g_update_replays_from_one_graph(gpu_device):
    from damc import optim as dopt
    from damc import synth
    from src import diffusion_net as dn

    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=16, nc=3), 0).to(gpu_device).train()
    B = 8
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 3, 32, 32))).to(gpu_device)
    z = torch.from_numpy(synth.normal_f32(2, 0, (B, 128))).to(gpu_device)
    params = list(G.parameters())

    def make_opt(ps):
        return dopt.Adam(ps, lr=2e-4, betas=(0.5, 0.999), capturable=True)

    def update(opt):
        opt.zero_grad()
        torch.sum((G(z) - x) ** 2, dim=[1, 2, 3]).mean().backward()
        opt.clip_and_step(MAX_NORM)

    _replay_against_eager(params, make_opt, lambda opt, k: update(opt), lambda opt: (lambda: update(opt)))


def test_e_update_replays_from_one_graph(gpu_device):
    from damc import optim as dopt
    from damc import synth
    from src import diffusion_net as dn

    E = synth.load_into(dn._netE(nz=128), 10).to(gpu_device).train()
    zp = torch.from_numpy(synth.normal_f32(81, 0, (8, 128))).to(gpu_device)
    zn = torch.from_numpy(synth.normal_f32(81, 1, (16, 128))).to(gpu_device)
    params = list(E.parameters())

    def make_opt(ps):
        return dopt.Adam(ps, lr=2e-4, betas=(0.5, 0.999), capturable=True)

    def update(opt):
        opt.zero_grad()
        e_pos, e_neg = E(zp), E(zn)  # both forwards before the one backward
        (e_pos.mean() - e_neg.mean()).backward()
        opt.clip_and_step(MAX_NORM)

    _replay_against_eager(params, make_opt, lambda opt, k: update(opt), lambda opt: (lambda: update(opt)))
