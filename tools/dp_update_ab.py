"""What the data-parallel update costs on ONE GPU: damc.dist.sharded_step at world 1 against optimizer.clip_and_step,
the pack kernel alone, and the seeded Q.calculate_loss against the unseeded one, legs alternating in one process.

Nets: _netG_cifar10(ngf = 128), _netQ_U(cifar10) and _netE(nz = 128) at B = 128, counter-hash weights.  The gradients
of one backward are kept; before every timed step each parameter gets a fresh copy of them (untimed), so both legs
clip and step the same values.  Device events around the timed call, on an idle stream: the figure holds the host's
launch work as well as the kernels.  Launches per Q update are the device kernels torch.profiler sees in one update.
Nothing here measures more than one GPU: there is no collective at world 1.

usage: python tools/dp_update_ab.py [--reps 15] [--warmup 3] [--out FILE]
"""
import argparse
import copy
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "diffusion-amortized-mcmc_amd"), HERE]
from damc import dist, optim, synth  # noqa: E402
from src import diffusion_net as dn  # noqa: E402

B, MAX_NORM = 128, 100.0


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def alternate(legs, reps, warmup):
    """legs: [(name, prepare, fn)]; returns {name: [ms]} with the legs alternating within each repeat."""
    times = {name: [] for name, _, _ in legs}
    for i in range(warmup + reps):
        for name, prepare, fn in legs:
            prepare()
            t = timed(fn)
            if i >= warmup:
                times[name].append(t)
    return times


def kernels_per_call(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=128, nc=3), 0).to(dev).train()
    E = synth.load_into(dn._netE(nz=128), 10).to(dev).train()
    Q = synth.load_into(dn._netQ_U(nc=3, nz=128, dataset="cifar10", with_noise=True), 20).to(dev).train()
    z = torch.from_numpy(synth.normal_f32(2, 7, (B, 128))).to(dev)
    x = torch.from_numpy(synth.uniform_f32(1, 7, (B, 3, 32, 32))).to(dev)
    zn = torch.from_numpy(synth.normal_f32(81, 1, (2 * B, 128))).to(dev)
    mask = (torch.from_numpy(synth.uniform_f32(53, 0, (B, 1), 0.0, 1.0)) >= 0.1).float().to(dev)

    def q_loss(net, seed=None, k=0):
        for p in net.parameters():
            p.grad = None
        net.calculate_loss(x=x, z=z, mask=mask, seed=seed, draw_index=k).mean().backward()

    backward = {
        "G": lambda net: torch.sum((net(z) - x) ** 2, dim=[1, 2, 3]).mean().backward(),
        "E": lambda net: (net(z).mean() - net(zn).mean()).backward(),
        "Q": lambda net: q_loss(net, seed=12345),
    }
    make_opt = {
        "G": lambda net: optim.Adam(net.parameters(), lr=2e-4, betas=(0.5, 0.999)),
        "E": lambda net: optim.Adam(net.parameters(), lr=2e-5, betas=(0.5, 0.999)),
        "Q": lambda net: optim.AdamW(net.parameters(), lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-4),
    }
    lines = ["data-parallel update at world 1 on one GPU, B = %d: device events on an idle stream around each call, "
             "median (min .. max) ms of %d after %d warm-ups, legs alternating within each repeat, one process"
             % (B, a.reps, a.warmup)]
    for name, net in (("G", G), ("Q", Q), ("E", E)):
        nets = [net, copy.deepcopy(net)]
        opts = [make_opt[name](n) for n in nets]
        backward[name](nets[0])
        saved = [None if p.grad is None else p.grad.detach().clone() for p in nets[0].parameters()]
        numel = sum(g.numel() for g in saved if g is not None)

        def refill(n):
            for p, g in zip(n.parameters(), saved):
                p.grad = None if g is None else g.clone()

        bucket = dist.GradBucket(list(nets[1].parameters()))
        legs = [("clip_and_step", lambda: refill(nets[0]), lambda: opts[0].clip_and_step(MAX_NORM)),
                ("sharded_step", lambda: refill(nets[1]), lambda: dist.sharded_step(opts[1], B, B, max_norm=MAX_NORM)),
                ("pack alone", lambda: refill(nets[1]), lambda: bucket.pack(1.0))]
        t = alternate(legs, a.reps, a.warmup)
        base = stats(t["clip_and_step"])[0]
        for leg, _, _ in legs:
            m, lo, hi = stats(t[leg])
            extra = "  %+.3f ms on clip_and_step" % (m - base) if leg == "sharded_step" else ""
            if leg == "pack alone":
                extra = "  %.1f MB moved (4 B read + 4 B written per element), %.0f GB/s at the median" % (
                    8e-6 * numel, 8e-9 * numel / (m * 1e-3))
            lines.append("%s update (%d gradient tensors, %.2f M elements)  %-14s %8.3f ms (%.3f .. %.3f)%s"
                         % (name, sum(g is not None for g in saved), numel / 1e6, leg, m, lo, hi, extra))
    # the Q update's forward + backward: torch's draws against the seeded ones
    k = [0]

    def seeded():
        k[0] += 1
        q_loss(Q, seed=12345, k=k[0])

    legs = [("unseeded", lambda: None, lambda: q_loss(Q)), ("seeded", lambda: None, seeded)]
    t = alternate(legs, a.reps, a.warmup)
    for leg, _, fn in legs:
        m, lo, hi = stats(t[leg])
        try:
            launches = "%d device kernels per update" % kernels_per_call(fn)
        except Exception as e:  # the profiler is optional equipment: say so in the record, never guess
            launches = "launches not counted (%s: %s)" % (type(e).__name__, e)
        lines.append("Q.calculate_loss(...).mean().backward()  %-9s %8.3f ms (%.3f .. %.3f)  %s"
                     % (leg, m, lo, hi, launches))
    out = "\n".join(lines)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
