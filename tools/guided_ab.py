"""Guided sampling Q(x, cond_w = 0.5) three ways at the bench's CIFAR amortizer (nz 128, nxemb 1024, ntemb 128, nif 64,
100 steps): the reference's step loop on libdamc (amortizer._q_forward_guided_steps), the fused guided sweep with the
reference's torch draws (amortizer._q_forward_guided) and with the library's Philox streams (q_forward with a seed);
the unguided Q(x) for scale.  Device events around whole calls, warm-ups first, the variants alternating within each
repeat; then, in a pass of its own with the profiler on, the kernel launches of one call of each (clock-independent).

usage: python tools/guided_ab.py [--batches 128,16] [--reps 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "diffusion-amortized-mcmc_amd"), HERE]
from damc import amortizer, synth  # noqa: E402
from src import diffusion_net as dn  # noqa: E402

W = 0.5


def variants(Q, x, zt0):
    return [
        ("step loop (_q_forward_guided_steps)", lambda: amortizer._q_forward_guided_steps(Q, x, W)),
        ("fused, reference draws (seed=None)", lambda: amortizer._q_forward_guided(Q, x, W)),
        ("fused, seeded (Philox)", lambda: amortizer.q_forward(Q, x=x, cond_w=W, zt=zt0, seed=11)),
        ("unguided Q(x), seeded", lambda: amortizer.q_forward(Q, x=x, zt=zt0, seed=11)),
    ]


def launches(fn):
    """Kernel launches of one call, from the profiler's device activity (every kernel of the process is recorded)."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() \
                and "memset" not in e.name.lower():
            n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Q = dn._netQ_U(nc=3, nz=128, nxemb=1024, ntemb=128, nif=64, diffusion_residual=True, n_interval=100,
                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Q, 20)
    Q.to(dev).eval()
    lines = ["guided sampling Q(x, cond_w=%.1f): CIFAR amortizer nz 128 nxemb 1024 ntemb 128 nif 64, n = 100; device "
             "events around whole calls, median (min .. max) of %d after %d warm-ups, variants alternating"
             % (W, a.reps, a.warmup)]
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            x = torch.from_numpy(synth.uniform_f32(93, 0, (B, 3, 32, 32))).to(dev)
            zt0 = torch.from_numpy(synth.normal_f32(8, 0, (B, 128))).to(dev)
            vs = variants(Q, x, zt0)
            for _ in range(a.warmup):
                for _, fn in vs:
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in vs}
            for _ in range(a.reps):
                for name, fn in vs:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn()
                    t1.record()
                    t1.synchronize()
                    times[name].append(t0.elapsed_time(t1))
            # the seeded fused sweep is the step loop's arithmetic on other draws; the two reference-draw forms see
            # the same draws
            torch.manual_seed(7)
            za = vs[0][1]()
            torch.manual_seed(7)
            zb = vs[1][1]()
            diff = float((za - zb).norm() / za.norm())
            base = sorted(times[vs[0][0]])[a.reps // 2]
            for name, fn in vs:
                t = sorted(times[name])
                try:
                    nl = "%d" % launches(fn)
                except Exception as e:  # the profiler is not part of the measurement
                    nl = "not measured (%s)" % type(e).__name__
                lines.append("B=%-4d %-38s %9.3f ms (%.3f .. %.3f)  x%.2f of the step loop  kernel launches %s"
                             % (B, name, t[a.reps // 2], t[0], t[-1], t[a.reps // 2] / base, nl))
            lines.append("B=%-4d fused vs step loop on the same torch draws: end point rel-L2 %.2e" % (B, diff))
    out = "\n".join(lines)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
