"""The whole training iteration as ONE replayed graph against the same calls issued by the host, and the fused EMA of
the target against the reference's per-parameter torch expression, in one process.

The bench configuration: CIFAR-10 nets (_netG_cifar10 ngf 128, _netE, _netQ_U nxemb 1024 / ntemb 128 / nif 64 with the
driver's 100 sweep steps) at B = 128, 30 posterior and 60 prior Langevin steps, six Q updates, clip at 100.

(a) EMA leg: damc.schedule.EmaTarget.update() (one launch per 96 tensors) against
    `for p, t in zip(Q.parameters(), Q_target.parameters()): t.data.copy_(rho * p.data + (1 - rho) * t.data)`
    (train_gen_recon.py:260-261: three kernels and a copy per tensor) over the same tensors; --ema-inner applications per
    sample so a sample is not a fraction of a millisecond, reported per application.
(b) Iteration leg: damc.loop.TrainIteration.body() issued eagerly against its recorded graph replayed.  Both legs run
    the same kernels on the same state (tests/test_gpu_train_iteration.py pins replay k to iteration k); what differs
    is who issues the launches.

Times are host wall clock around the work, a device synchronise before and after.  Median (min .. max) of --reps after
--warmup, the legs alternating within each repeat.  The shader clock is read from in-kernel stamps (damc_clock_probe)
over one more, untimed, eager iteration behind the timed ones.

usage: python tools/train_iteration_ab.py [--reps 20] [--warmup 3] [--batch 128] [--out FILE]
"""
import argparse
import copy
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "diffusion-amortized-mcmc_amd"), HERE]
from damc import _lib, loop, schedule, synth  # noqa: E402
from damc import optim as dopt  # noqa: E402
from src import diffusion_net as dn  # noqa: E402

SEED = 2 ** 40 + 11
RHO = 0.005


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab(title, legs, reps, warmup, per=1, unit="ms"):
    for _ in range(warmup):
        for _, fn in legs:
            wall(fn)
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, fn in legs:
            times[name].append(wall(fn) / per)
    base = sorted(times[legs[0][0]])[reps // 2]
    lines = []
    for name, _ in legs:
        t = sorted(times[name])
        lines.append("%-40s %-34s %9.4f %s (%.4f .. %.4f)  x%.3f of the first leg"
                     % (title, name, t[reps // 2], unit, t[0], t[-1], t[reps // 2] / base))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--ngf", type=int, default=128)
    ap.add_argument("--n-interval", type=int, default=100)
    ap.add_argument("--ema-inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_iteration_ab: needs a ROCm device; there is no CPU path to time")
    dev = torch.device("cuda:0")
    B = a.batch

    Q = dn._netQ_U(nc=3, nz=128, nxemb=1024, ntemb=128, nif=64, diffusion_residual=True, n_interval=a.n_interval,
                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Q, 20)
    Q.to(dev).eval()
    Qt = copy.deepcopy(Q)
    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=a.ngf, nc=3), 0).to(dev).eval()
    E = synth.load_into(dn._netE(nz=128), 10).to(dev).eval()
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 3, 32, 32))).to(dev)
    nq = sum(p.numel() for p in Q.parameters())
    lines = ["whole iteration and EMA A/B: host wall clock around the work (device synchronise before and after), median "
             "(min .. max) of %d after %d warm-ups, legs alternating within each repeat, one process; CIFAR-10, ngf %d, "
             "B = %d, %d sweep steps, 30 + 60 Langevin steps, 6 Q updates; amortizer: %d tensors, %d elements"
             % (a.reps, a.warmup, a.ngf, B, a.n_interval, len(list(Q.parameters())), nq)]

    # ---- (a) the EMA of the target, applied always (no clock), on a scratch copy of the target
    Qs = copy.deepcopy(Qt)
    ema = schedule.EmaTarget(list(Q.parameters()), list(Qs.parameters()), rho=RHO)

    def ema_fused():
        for _ in range(a.ema_inner):
            ema.update()

    def ema_torch():
        for _ in range(a.ema_inner):
            for param, target_param in zip(Q.parameters(), Qs.parameters()):
                target_param.data.copy_(RHO * param.data + (1 - RHO) * target_param.data)

    lines += ab("EMA of the target, per application", [("torch expression per parameter", ema_torch),
                                                      ("damc_ema_update, 96 tensors a launch", ema_fused)],
                a.reps, a.warmup, per=a.ema_inner)
    lines.append("  (12 B per element: %.2f MB per application)" % (12.0 * nq / 1e6))

    # ---- (b) the whole iteration
    opts = (dopt.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999), capturable=True),
            dopt.AdamW(Q.parameters(), lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-4, capturable=True),
            dopt.Adam(E.parameters(), lr=1e-4, betas=(0.5, 0.999), capturable=True))
    clock = schedule.TrainClock(dev)
    draws = loop.make_draws(SEED, dev)
    step = loop.TrainIteration(G, E, Q, Qt, opts, clock, draws, x, p_mask=0.2, g_l_steps=30, g_llhd_sigma=0.1,
                               g_l_step_size=0.1, e_l_steps=60, e_l_step_size=0.4, q_max_norm=100.0, g_max_norm=100.0,
                               e_max_norm=100.0)
    graph = step.capture()
    lines += ab("whole iteration", [("body() issued by the host", step.body), ("one replayed graph", graph.replay)],
                a.reps, a.warmup)

    # the clock the generator's K loops hold, one untimed eager iteration right behind the timed ones
    L = _lib.lib()
    clk = torch.zeros(4096 * 4, dtype=torch.int64, device=dev)
    L.damc_clock_probe(clk.data_ptr(), 4096)
    step.body()
    torch.cuda.synchronize()
    L.damc_clock_probe(None, 0)
    cs = clk.view(-1, 4).cpu().double()
    ok = cs[:, 3] > cs[:, 1]
    ghz = float(((cs[ok, 2] - cs[ok, 0]) / (cs[ok, 3] - cs[ok, 1])).median()) * 0.1 if ok.any() else None
    lines.append("shader clock in the generator's K loops (in-kernel stamps, one untimed iteration): %s"
                 % ("%.2f GHz" % ghz if ghz else "not measured"))
    n_it = clock.read()
    finite = all(bool(torch.isfinite(p).all()) for net in (G, E, Q, Qt) for p in net.parameters())
    finite = finite and bool(torch.isfinite(step.zk_pos).all())
    lines.append("iterations run: %d (clock); lr %s; parameters and chains finite after the run: %s"
                 % (n_it, ", ".join("%.6g" % v for v in step.lr_decay.values()), finite))
    out = "\n".join(lines)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
