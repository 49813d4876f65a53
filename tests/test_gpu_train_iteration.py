"""GPU capstone: the WHOLE training iteration (train_gen_recon.py:187-261) recorded into one graph by
damc.loop.TrainIteration and replayed six times, against a host-driven loop written out here.

The host loop makes the seeded calls damc.loop documents for each noise consumer (seed= / step_offset= / draw_index=
at loop.offsets(it, ...)), decides the two "every Nth iteration" branches with `if (it + 1) % period == 0` on the host,
moves the target with the torch expression of train_gen_recon.py:261 and writes the Python lr chain into the
optimisers' lr tensors.  Both sides step the same capturable optimiser class, so they run the same kernels, and replay
k must BE iteration k: every parameter of Q, the target, G and E, both Adam moments and `step`, the final zk_pos, the
lr doubles, the clock and every DrawState counter are compared exactly (torch.equal / ==).

EMA period 2 and lr period 3: six iterations cross each gate more than once, on different iterations.  The batch x is
rewritten in place before every replay.  After the warm-up and the capture, all state is restored IN PLACE (the graph
holds the addresses).  A capture the runtime rejects raises a HIP error from torch.cuda.graph; nothing here retries."""
import copy

import pytest
import torch

from conftest import build_q_case

pytestmark = pytest.mark.gpu

BASE_SEED = 2 ** 41 + 1234
N_IT = 6
B = 8
G_L_STEPS, E_L_STEPS = 3, 4
SIGMA, G_STEP, E_STEP = 0.1, 0.1, 0.4
P_MASK = 0.5
MAX_NORM = 1.0
RHO, EMA_PERIOD = 0.005, 2
LR_FACTOR, LR_FLOOR, LR_PERIOD = 0.99, 1e-5, 3
LR0 = dict(G=2e-4, Q=3e-4, E=1.02e-5)  # E's reaches the floor at its second decay


def _nets(device):
    from damc import synth
    from src import diffusion_net as dn

    Q = build_q_case("q_cifar10_s", device)["Q"]
    Qt = copy.deepcopy(Q)  # the target starts as a copy (train_gen_recon.py:145-146)
    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=16, nc=3), 0).to(device).eval()
    E = synth.load_into(dn._netE(nz=128), 10).to(device).eval()
    return G, E, Q, Qt


def _optimizers(G, E, Q, device, tensor_lr):
    from damc import optim as dopt

    def lr(name):
        return torch.tensor(LR0[name], dtype=torch.float32, device=device) if tensor_lr else LR0[name]

    return (dopt.Adam(G.parameters(), lr=lr("G"), betas=(0.5, 0.999), capturable=True),
            dopt.AdamW(Q.parameters(), lr=lr("Q"), betas=(0.5, 0.999), weight_decay=1e-4, capturable=True),
            dopt.Adam(E.parameters(), lr=lr("E"), betas=(0.5, 0.999), capturable=True))


def _state(nets, opts):
    params = [[p.detach().clone() for p in net.parameters()] for net in nets]
    moments = []
    for opt in opts:
        for group in opt.param_groups:
            for p in group["params"]:
                st = opt.state.get(p)
                if st:
                    moments.append((st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])))
    return params, moments


def _host_iteration(it, nets, opts, lrs, x, masks):
    """Iteration `it` of the reference driver with every draw a seeded call at the documented offset."""
    from damc import _lib, loop
    from damc import amortizer as am
    from damc import langevin as lv

    G, E, Q, Qt = nets
    G_opt, Q_opt, E_opt = opts
    dev, nz, n = x.device, Q.nz, int(Q.n_interval)
    s = loop.seeds(BASE_SEED)
    o = loop.offsets(it, n, G_L_STEPS, E_L_STEPS, 6)

    def normal(name):
        return lv.philox_normal(1, B, nz, seed=s[name], device=dev, step_offset=o[name])[0]

    def sweep(net, xemb, zt, name):
        # the seeded sweep has no host offset: it is fed the noise its own stream holds from that offset on
        noise = lv.philox_normal(n - 1, B, nz, seed=s[name], device=dev, step_offset=o[name],
                                 stream_id=_lib.STREAM_SWEEP)
        am.reverse_sweep(net, xemb, zt, noise=noise, seed=0)
        return zt

    z_mask_prob = lv.philox_uniform(1, B, seed=s["mask"], device=dev, step_offset=o["mask"])[0]
    z_mask = torch.ones(B, device=dev)
    z_mask[z_mask_prob < P_MASK] = 0.0
    z_mask = z_mask.unsqueeze(-1)
    masks.append(z_mask.clone())
    Q.eval(), G.eval(), E.eval()
    with torch.no_grad():
        z0 = sweep(Qt, am.encoder_forward(Qt.encoder, x), normal("zt_target"), "sweep_target")
        xemb = am.prior_embedding(Q, normal("pe_prior"))
        sweep(Q, xemb, normal("zt_prior"), "sweep_prior")  # zp: drawn and swept as the driver does, then unused
        zk_pos = z0.clone()
        lv.posterior_langevin(zk_pos, x, G, E, G_L_STEPS, SIGMA, G_STEP, True, seed=s["posterior"],
                              step_offset=o["posterior"])
        zk_neg = torch.cat([z0, normal("fresh")], dim=0)
        lv.prior_langevin(zk_neg, E, E_L_STEPS, E_STEP, True, seed=s["prior"], step_offset=o["prior"])
    for j in range(6):
        Q_opt.zero_grad()
        Q.train()
        Q.calculate_loss(x=x, z=zk_pos, mask=z_mask, seed=s["q"], draw_index=o["q"] + j).mean().backward()
        Q_opt.clip_and_step(MAX_NORM)
    G_opt.zero_grad()
    G.train()
    torch.sum((G(zk_pos) - x) ** 2, dim=[1, 2, 3]).mean().backward()
    G_opt.clip_and_step(MAX_NORM)
    E_opt.zero_grad()
    E.train()
    e_pos, e_neg = E(zk_pos), E(zk_neg)
    (e_pos.mean() - e_neg.mean()).backward()
    E_opt.clip_and_step(MAX_NORM)
    Q.eval(), G.eval(), E.eval()
    if (it + 1) % LR_PERIOD == 0:
        for k in ("G", "Q", "E"):
            lrs[k] = max(lrs[k] * LR_FACTOR, LR_FLOOR)
        for opt, k in zip(opts, ("G", "Q", "E")):
            for group in opt.param_groups:
                group["lr"].fill_(lrs[k])
    if (it + 1) % EMA_PERIOD == 0:
        for param, target_param in zip(Q.parameters(), Qt.parameters()):
            target_param.data.copy_(RHO * param.data + (1 - RHO) * target_param.data)
    return zk_pos


def test_whole_iteration_replays_from_one_graph(gpu_device):
    from damc import loop, schedule, synth

    xs = [torch.from_numpy(synth.uniform_f32(1, k, (B, 3, 32, 32))).to(gpu_device) for k in range(N_IT)]

    # ---- the host-driven loop
    nets = _nets(gpu_device)
    n = int(nets[2].n_interval)
    opts = _optimizers(nets[0], nets[1], nets[2], gpu_device, tensor_lr=True)
    lrs, masks = dict(LR0), []
    x = xs[0].clone()
    for it in range(N_IT):
        x.copy_(xs[it])
        zk_want = _host_iteration(it, nets, opts, lrs, x, masks)
    torch.cuda.synchronize()
    want = _state(nets, opts)
    seen = torch.cat(masks).unique().tolist()
    assert seen == [0.0, 1.0], "the six masks must hold both values (encoder rows and prior-embedding rows)"
    assert all(torch.isfinite(p).all() for ps in want[0] for p in ps) and torch.isfinite(zk_want).all()
    assert lrs["G"] == 2e-4 * 0.99 * 0.99 and lrs["E"] == 1e-5
    start_nets = _nets(gpu_device)
    for a, b, name in zip(want[0], start_nets, "GEQT"):
        assert any(not torch.equal(u, v.detach()) for u, v in zip(a, b.parameters())), "%s never changed" % name

    # ---- the captured iteration
    G, E, Q, Qt = cap_nets = start_nets
    start = [[p.detach().clone() for p in net.parameters()] for net in cap_nets]
    cap_opts = _optimizers(G, E, Q, gpu_device, tensor_lr=False)  # LrDecay installs the lr tensors
    clock = schedule.TrainClock(gpu_device)
    draws = loop.make_draws(BASE_SEED, gpu_device)
    xc = xs[0].clone()
    step = loop.TrainIteration(G, E, Q, Qt, cap_opts, clock, draws, xc, p_mask=P_MASK, g_l_steps=G_L_STEPS,
                               g_llhd_sigma=SIGMA, g_l_step_size=G_STEP, e_l_steps=E_L_STEPS, e_l_step_size=E_STEP,
                               q_max_norm=MAX_NORM, g_max_norm=MAX_NORM, e_max_norm=MAX_NORM, rho=RHO,
                               ema_period=EMA_PERIOD, lr_factor=LR_FACTOR, lr_floor=LR_FLOOR, lr_period=LR_PERIOD)
    lr_start = step.lr_decay.state_dict()
    assert lr_start["lr"] == [LR0["G"], LR0["Q"], LR0["E"]]
    graph = step.capture()  # the warm-up ran one iteration for real: everything it moved goes back, in place
    with torch.no_grad():
        for net, saved in zip(cap_nets, start):
            for p, s0 in zip(net.parameters(), saved):
                p.copy_(s0)
        for opt in cap_opts:
            for st in opt.state.values():
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
                st["step"].zero_()
    step.lr_decay.load_state_dict(lr_start)
    seeds = loop.seeds(BASE_SEED)
    for name in loop.CONSUMERS:
        draws[name].set(seeds[name], 0)
    clock.set(0)
    for it in range(N_IT):
        xc.copy_(xs[it])
        graph.replay()
    torch.cuda.synchronize()

    got = _state(cap_nets, cap_opts)
    for name, a, b in zip(("G", "E", "Q", "Q_target"), got[0], want[0]):
        assert len(a) == len(b)
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), "%s parameter %d differs after %d replays" % (name, i, N_IT)
    assert len(got[1]) == len(want[1]) and len(got[1]) > 0
    for i, ((m1, v1, t1), (m2, v2, t2)) in enumerate(zip(got[1], want[1])):
        assert t1 == t2 and t1 in (float(N_IT), float(6 * N_IT)), "step of state %d: %r vs %r" % (i, t1, t2)
        assert torch.equal(m1, m2), "exp_avg %d" % i
        assert torch.equal(v1, v2), "exp_avg_sq %d" % i
    assert torch.equal(step.zk_pos, zk_want)
    assert step.lr_decay.values() == [lrs["G"], lrs["Q"], lrs["E"]]
    for opt, k in zip(cap_opts, ("G", "Q", "E")):
        assert torch.equal(opt.param_groups[0]["lr"].cpu(), torch.tensor(lrs[k], dtype=torch.float32))
    assert clock.read() == N_IT
    counters = loop.offsets(N_IT, n, G_L_STEPS, E_L_STEPS, 6)
    for name in loop.CONSUMERS:
        assert draws[name].read() == (seeds[name], counters[name]), name
