"""Six Q updates and the Langevin block, as eager seeded calls against ONE replayed graph, in one process.

The CIFAR amortizer (_netQ_U nxemb 1024, ntemb 128, nif 64) at B = 128, train mode.  Q leg: the six Q updates of an
iteration (zero_grad; Q.calculate_loss(x, z, mask, ...).mean().backward(); clip_and_step) with AdamW(capturable=True) --
eager with seed= / draw_index=, or one graph of the six with draws= (damc.graphs.DrawState), replayed.  Langevin leg:
the headline block, 30 posterior steps on B chains of _netG_cifar10(ngf 128) and 60 prior steps on 2B chains, eager with
seed= / step_offset= or one graph with draws=.  Both legs of a pair run the same kernels on the same values (the
draw-state and capstone tests pin that); what differs is who issues the launches.

Times are host wall clock around the work, a device synchronise before and after: the eager Q update is host-bound, so
device events around it would time the same thing less directly.  Median (min .. max) of --reps after --warmup, the
legs alternating within each repeat.

usage: python tools/graph_update_ab.py [--reps 15] [--warmup 3] [--batch 128] [--out FILE]
"""
import argparse
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "diffusion-amortized-mcmc_amd"), HERE]
from damc import graphs, synth  # noqa: E402
from damc import langevin as lv  # noqa: E402
from damc import optim as dopt  # noqa: E402
from src import diffusion_net as dn  # noqa: E402

SEED = 2 ** 40 + 7
N_Q = 6


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch

    # ---- the six Q updates
    Q = dn._netQ_U(nc=3, nz=128, nxemb=1024, ntemb=128, nif=64, diffusion_residual=True, n_interval=20,
                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Q, 20)
    Q.to(dev).train()
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 3, 32, 32))).to(dev)
    z = torch.from_numpy(synth.normal_f32(2, 0, (B, 128))).to(dev)
    mask = torch.ones(B, 1, device=dev)
    mask[1::3] = 0.0
    opt = dopt.AdamW(Q.parameters(), lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-4, capturable=True)
    ds_q = graphs.DrawState(SEED, dev)
    it = [0]

    def q_eager():
        for k in range(N_Q):
            opt.zero_grad()
            Q.calculate_loss(x, z, mask, seed=SEED, draw_index=N_Q * it[0] + k).mean().backward()
            opt.clip_and_step(1.0)
        it[0] += 1

    def q_body():
        for _ in range(N_Q):
            opt.zero_grad()
            Q.calculate_loss(x, z, mask, draws=ds_q).mean().backward()
            opt.clip_and_step(1.0)

    q_graph = graphs.capture(q_body)

    # ---- the Langevin block
    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=128, nc=3), 0).to(dev).eval()
    E = synth.load_into(dn._netE(nz=128), 10).to(dev).eval()
    zp0 = torch.from_numpy(synth.normal_f32(3, 0, (B, 128))).to(dev)
    zn0 = torch.from_numpy(synth.normal_f32(4, 0, (2 * B, 128))).to(dev)
    zp, zn = zp0.clone(), zn0.clone()
    ds_a, ds_b = graphs.DrawState(SEED + 1, dev), graphs.DrawState(SEED + 2, dev)
    lit = [0]

    def l_eager():
        zp.copy_(zp0)
        zn.copy_(zn0)
        lv.posterior_langevin(zp, x, G, E, 30, 0.1, 0.1, True, seed=SEED + 1, step_offset=30 * lit[0])
        lv.prior_langevin(zn, E, 60, 0.4, True, seed=SEED + 2, step_offset=60 * lit[0])
        lit[0] += 1

    def l_body():
        zp.copy_(zp0)
        zn.copy_(zn0)
        lv.posterior_langevin(zp, x, G, E, 30, 0.1, 0.1, True, draws=ds_a)
        lv.prior_langevin(zn, E, 60, 0.4, True, draws=ds_b)

    l_graph = graphs.capture(l_body)

    groups = [("six Q updates, CIFAR amortizer B=%d" % B,
               [("eager seeded calls", q_eager), ("one replayed graph", q_graph.replay)]),
              ("Langevin block 30 + 60 steps, B=%d / %d" % (B, 2 * B),
               [("eager seeded calls", l_eager), ("one replayed graph", l_graph.replay)])]
    lines = ["graph replay against eager seeded calls: host wall clock around the work (device synchronise before and "
             "after), median (min .. max) ms of %d after %d warm-ups, legs alternating within each repeat, one process"
             % (a.reps, a.warmup)]
    for title, legs in groups:
        for _ in range(a.warmup):
            for _, fn in legs:
                wall(fn)
        times = {name: [] for name, _ in legs}
        for _ in range(a.reps):
            for name, fn in legs:
                times[name].append(wall(fn))
        base = sorted(times[legs[0][0]])[a.reps // 2]
        for name, _ in legs:
            t = sorted(times[name])
            lines.append("%-44s %-20s %8.3f ms (%.3f .. %.3f)  x%.2f of the eager leg"
                         % (title, name, t[a.reps // 2], t[0], t[-1], t[a.reps // 2] / base))
    finite = all(bool(torch.isfinite(p).all()) for p in Q.parameters()) and bool(torch.isfinite(zp).all())
    lines.append("parameters and chains finite after the run: %s" % finite)
    out = "\n".join(lines)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
