"""The anomaly drivers' scoring loop body two ways at the MNIST driver's shape (_netG_mnist ngf 128 nz 8, _netE, Q nif
128 nxemb 1024 ntemb 128, 100-step sweep, B = 500, 5 noiseless posterior steps; eval_anomaly_det.py:102-119):

  (a) as the drivers write it on the public API without damc.anomaly: Q(x), sample_langevin_post_z_with_prior, G(z),
      E(z) and the torch sums;
  (b) damc.anomaly.score.

Device events around whole calls, warm-ups first, the legs alternating within each repeat.  After the timing both legs
run once more on the same draws (the host generator reseeded) and their scores are compared.

usage: python tools/anomaly_ab.py [--batch 500] [--reps 5] [--warmup 2] [--out FILE]
       python tools/anomaly_ab.py --leg-b-only N          N calls of leg (b) and nothing else (a kernel-trace run)
       python tools/anomaly_ab.py --stats kernel_stats.csv --out FILE     append the new kernels' rows of such a trace
"""
import argparse
import csv
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "diffusion-amortized-mcmc_amd"), HERE]

NEW_KERNELS = ("recon_rows_kernel", "energy_finish_kernel")


def append_stats(path, out):
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Name"] for k in NEW_KERNELS)]
    lines = ["kernel trace of leg (b) (rocprofv3 --kernel-trace --stats), the two kernels of csrc/energy.hip:"]
    for r in rows:
        lines.append("  %-60s calls %5s  average %8.2f us  total %9.3f ms  %5.2f %% of kernel time"
                     % (r["Name"][:60], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6,
                        float(r["Percentage"])))
    if not rows:
        lines.append("  not measured: no such kernel in %s" % path)
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--leg-b-only", type=int, default=0)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stats:
        return append_stats(a.stats, a.out)

    import torch

    from damc import anomaly, synth
    from src import MCMC as mc
    from src import diffusion_net as dn

    dev = torch.device("cuda:0")
    B, nz = a.batch, 8
    G = synth.load_into(dn._netG_mnist(nz=nz, ngf=128, nc=1), 0).to(dev).eval()
    E = synth.load_into(dn._netE(nz=nz), 10).to(dev).eval()
    Q = synth.load_into(dn._netQ_U(nc=1, nz=nz, nxemb=1024, ntemb=128, nif=128, diffusion_residual=True, n_interval=100,
                                   logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, cond_w=0.0,
                                   dataset="mnist"), 20).to(dev).eval()
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 1, 28, 28))).to(dev)

    def leg_a():  # eval_anomaly_det.py:104-117
        with torch.no_grad():
            z0 = Q(x)
        zk = z0.detach().clone()
        zk.requires_grad = True
        zk = mc.sample_langevin_post_z_with_prior(z=zk, x=x, netG=G, netE=E, g_l_steps=a.steps, g_llhd_sigma=1.0,
                                                  g_l_with_noise=False, g_l_step_size=0.1, verbose=False)
        with torch.no_grad():
            x_hat = G(zk)
            s_hat = E(zk)
            return torch.sum((x_hat - x) ** 2, dim=[1, 2, 3]) * 1 + s_hat + torch.sum(zk ** 2, dim=-1) * 0.5

    def leg_b():
        return anomaly.score(Q, G, E, x, g_l_steps=a.steps, g_l_step_size=0.1, g_llhd_sigma=1.0)[0]

    if a.leg_b_only:
        for _ in range(a.leg_b_only):
            leg_b()
        torch.cuda.synchronize()
        return
    legs = [("(a) driver loop body, public API", leg_a), ("(b) anomaly.score", leg_b)]
    for _ in range(a.warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(a.reps):
        for name, fn in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))
    torch.manual_seed(7)
    sa = leg_a()
    torch.manual_seed(7)
    sb = leg_b()
    lines = ["anomaly scoring loop body at the MNIST driver's shape: _netG_mnist ngf 128 nz 8, Q nif 128 nxemb 1024 "
             "ntemb 128 n = 100, B = %d, %d noiseless posterior steps; device events around whole calls, median "
             "(min .. max) of %d after %d warm-ups, legs alternating" % (B, a.steps, a.reps, a.warmup)]
    for name, _ in legs:
        t = sorted(times[name])
        lines.append("%-36s %9.3f ms (%.3f .. %.3f)" % (name, t[len(t) // 2], t[0], t[-1]))
    ta, tb = sorted(times[legs[0][0]]), sorted(times[legs[1][0]])
    lines.append("(b) median %s (a) maximum: %.3f vs %.3f ms" % ("<=" if tb[len(tb) // 2] <= ta[-1] else ">",
                                                                 tb[len(tb) // 2], ta[-1]))
    lines.append("scores of (b) vs (a) on the same draws: rel-L2 %.2e" % float((sa - sb).norm() / sa.norm()))
    out = "\n".join(lines)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
