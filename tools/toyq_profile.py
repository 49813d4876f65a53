#!/usr/bin/env python3
"""Time the toy amortizer's Q(x) on libdamc against the same module on stock PyTorch layers (one GPU).

usage: python tools/toyq_profile.py [--batch 500] [--repeats 20] [--out profiles/toyq/toyq_profile.json]

  * toy Q(x), the driver's arguments (workspace/toy_example/toy_example.py:71-76, 318-324: n_interval 100, logsnr
    -5.1 / 9.8, 'large', noise, residual) at B = 500 (toy_example.py:197): the drop-in's forward (fused MLP encoder +
    row-resident sweep) against the reference's step loop (toy_example/src/diffusion_net.py:188-239) on the module's
    own nn layers with damc.training.ENABLED = False, alternating, HIP events around each call, median of repeats
    after warm-up.  Both include the host-generator draw of zt and its copy, as a caller sees them.
  * for information: the row-resident form (DAMC_SWEEP_ROWS=1) against the default team sweep of the CIFAR amortizer
    (nz 128, nxemb 1024, 100 steps) at B = 128, the whole damc_reverse_sweep call, alternating.
No thresholds: the figures go to the output file and to DESIGN.md §4.

       python tools/toyq_profile.py --leg q_update [--out profiles/toyq/toyq_qupdate.json] [--launches counts.json]

  * the toy's Q update as the driver runs it (toy_example.py:91, 209-219): six back-to-back calculate_loss -> backward
    -> clip_grad_norm_(100) -> AdamW.step at B = 500, on libdamc against the same module under
    damc.training.stock_pytorch() (what ran before the update moved to the library), alternating in one process; ms per
    update = the six-update time / 6.  --launches merges the kernel counts of a separate trace into the file.

       rocprofv3 --kernel-trace ... -- python tools/toyq_profile.py --leg q_update_trace --path libdamc|stock --updates N

  * N updates of one path and nothing else, for a kernel trace: launches per update = the difference of two traces'
    kernel counts over the difference of their N (start-up kernels cancel).  tools/toyq_launches.py turns the four traces
    into the --launches file.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "diffusion-amortized-mcmc_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def stock_q_forward(Q, x):
    """_netQ_U_toy.forward as the reference writes it (no guidance), on the module's stock layers."""
    from src.diffusion_helper_func import diffusion_reverse, logsnr_schedule_fn, pred_x_from_eps

    b, device, n = len(x), x.device, int(Q.n_interval)
    xemb = Q.encoder(x)
    zt = torch.randn(b, Q.nz).to(device)
    for i in reversed(range(0, n)):
        i_tensor = torch.ones(b, dtype=torch.float).to(device) * float(i)
        logsnr_t = logsnr_schedule_fn(i_tensor / (n - 1.0), logsnr_min=Q.logsnr_min, logsnr_max=Q.logsnr_max)
        logsnr_s = logsnr_schedule_fn(torch.clamp(i_tensor - 1.0, min=0.0) / (n - 1.0), logsnr_min=Q.logsnr_min,
                                      logsnr_max=Q.logsnr_max)
        eps_pred = Q.p(z=zt, logsnr=logsnr_t, xemb=xemb)
        logsnr_t = logsnr_t.reshape((b, 1))
        logsnr_s = logsnr_s.reshape((b, 1))
        pred_z = pred_x_from_eps(z=zt, eps=eps_pred, logsnr=logsnr_t)
        if i == 0:
            zt = pred_z
        else:
            dist = diffusion_reverse(x=pred_z, z_t=zt, logsnr_s=logsnr_s, logsnr_t=logsnr_t, pred_var_type=Q.var_type)
            eps = torch.randn_like(zt)
            zt = dist["mean"] + dist["std"] * eps if Q.with_noise else dist["mean"]
    return zt


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, warmup, repeats):
    """Median and spread (ms) of each callable, run in turn so that drift hits all alike."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t[k].append(timed(f))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), repeats=len(v)) for k, v in t.items()}


def toy_update_case(dev, B):
    """The driver's Q (toy_example.py:71-76, 318-324), its AdamW (:91) and one batch; step() is one update (:213-219)."""
    from damc import synth
    from src import diffusion_net as dn

    Q = dn._netQ_U_toy(nz=2, nxemb=128, ntemb=128, diffusion_residual=True, n_interval=100, logsnr_min=-5.1,
                       logsnr_max=9.8, var_type="large", with_noise=True, cond_w=0.0)
    synth.load_into(Q, 20)
    Q.to(dev).train()
    opt = torch.optim.AdamW(Q.parameters(), weight_decay=1e-2, lr=2e-4, betas=(0.5, 0.999))
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 2))).to(dev)
    z = torch.from_numpy(synth.normal_f32(2, 0, (B, 2))).to(dev)
    mask = (torch.from_numpy(synth.uniform_f32(3, 0, (B, 1), 0.0, 1.0)) >= 0.1).float().to(dev)

    def step():
        opt.zero_grad()
        Q.calculate_loss(x=x, z=z, mask=mask).mean().backward()
        torch.nn.utils.clip_grad_norm_(Q.parameters(), max_norm=100)
        opt.step()

    return step


def q_update_leg(args):
    from damc import training

    dev = torch.device("cuda:0")
    hip_step, stock_step = toy_update_case(dev, args.batch), toy_update_case(dev, args.batch)

    def hip():
        for _ in range(6):
            hip_step()

    def stock():
        with training.stock_pytorch():
            for _ in range(6):
                stock_step()

    r = alternate({"libdamc": hip, "stock_torch": stock}, args.warmup, args.repeats)
    for v in r.values():  # per update
        for k in ("median_ms", "min_ms", "max_ms"):
            v[k] /= 6.0
    out = dict(device=torch.cuda.get_device_name(0), batch=args.batch, updates_per_timed_unit=6,
               unit="ms per update (calculate_loss, backward, clip_grad_norm_, AdamW.step)", **r)
    out["stock_over_libdamc"] = r["stock_torch"]["median_ms"] / r["libdamc"]["median_ms"]
    if args.launches:
        with open(args.launches) as f:
            out["kernel_launches_per_update"] = json.load(f)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


def q_update_trace_leg(args):
    from damc import training

    step = toy_update_case(torch.device("cuda:0"), args.batch)
    if args.path == "stock":
        with training.stock_pytorch():
            for _ in range(args.updates):
                step()
    else:
        for _ in range(args.updates):
            step()
    torch.cuda.synchronize()
    print("%d updates on %s" % (args.updates, args.path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("forward", "q_update", "q_update_trace"), default="forward")
    ap.add_argument("--path", choices=("libdamc", "stock"), default="libdamc")
    ap.add_argument("--updates", type=int, default=6)
    ap.add_argument("--launches", default=None, help="JSON of kernel launches per update, merged into the q_update file")
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "toyq",
                                "toyq_qupdate.json" if args.leg == "q_update" else "toyq_profile.json")
    if not torch.cuda.is_available():
        sys.exit("toyq_profile.py needs a ROCm device: timings are GPU timings")
    if args.leg == "q_update":
        return q_update_leg(args)
    if args.leg == "q_update_trace":
        return q_update_trace_leg(args)
    from damc import amortizer as am
    from damc import synth, training
    from src import diffusion_net as dn

    dev = torch.device("cuda:0")
    B = args.batch
    Q = dn._netQ_U_toy(nz=2, nxemb=128, ntemb=128, diffusion_residual=True, n_interval=100, logsnr_min=-5.1,
                       logsnr_max=9.8, var_type="large", with_noise=True, cond_w=0.0)
    synth.load_into(Q, 20)
    Q.to(dev).eval()
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, 2))).to(dev)

    def hip():
        with torch.no_grad():
            Q(x)

    def stock():
        with torch.no_grad(), training.stock_pytorch():
            stock_q_forward(Q, x)

    out = dict(device=torch.cuda.get_device_name(0), toy=dict(batch=B, n_interval=100))
    out["toy"].update(alternate({"libdamc": hip, "stock_torch": stock}, args.warmup, args.repeats))
    out["toy"]["stock_over_libdamc"] = out["toy"]["stock_torch"]["median_ms"] / out["toy"]["libdamc"]["median_ms"]
    # the sweep alone (per-call stages 1-3 + the row-resident chain), on a fixed xemb
    xemb = am.encoder_forward(Q.encoder, x)
    zt0 = torch.from_numpy(synth.normal_f32(6, 0, (B, 2))).to(dev)
    out["toy"]["sweep_only"] = alternate({"rows": lambda: am.reverse_sweep(Q, xemb, zt0.clone(), seed=1)}, args.warmup,
                                         args.repeats)["rows"]
    # one 16-row tile alone: what a workgroup's dependent chain takes when nothing else runs
    x16, z16 = xemb[:16].contiguous(), zt0[:16].contiguous()
    out["toy"]["sweep_only_b16"] = alternate({"rows": lambda: am.reverse_sweep(Q, x16, z16.clone(), seed=1)},
                                             args.warmup, args.repeats)["rows"]

    # for information: row-resident against the team sweep at the CIFAR shape
    Qc = dn._netQ_U(nc=3, nz=128, nxemb=1024, ntemb=128, nif=64, diffusion_residual=True, n_interval=100,
                    logsnr_min=-5.1, logsnr_max=9.8, var_type="large", with_noise=True, dataset="cifar10")
    synth.load_into(Qc, 20)
    Qc.to(dev).eval()
    Bc = 128
    xe = torch.from_numpy(synth.normal_f32(7, 0, (Bc, 1024))).to(dev)
    z0 = torch.from_numpy(synth.normal_f32(8, 0, (Bc, 128))).to(dev)

    def sweep(rows):
        def f():
            os.environ["DAMC_SWEEP_ROWS"] = rows
            am.reverse_sweep(Qc, xe, z0.clone(), seed=1)
        return f

    try:
        out["cifar_b128"] = alternate({"team": sweep("0"), "rows": sweep("1")}, args.warmup, args.repeats)
    finally:
        os.environ.pop("DAMC_SWEEP_ROWS", None)
    out["cifar_b128"]["rows_over_team"] = out["cifar_b128"]["rows"]["median_ms"] / out["cifar_b128"]["team"]["median_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
