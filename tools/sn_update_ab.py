"""The G and E updates of spectral-norm nets, this tree's path against the stock PyTorch modules in one process.

G update (train_gen_recon.py:222-231: x_hat = G(z), the squared-error loss, backward) of _netG_cifar10(ngf = 128,
use_spc_norm=True) at B = 128; E update (:233-241: e_pos, e_neg = E(a), E(b), (e_pos.mean() - e_neg.mean()).backward())
of _netE(nz = 128, e_sn=True) at B = 128 / 256; train mode, so every forward runs one power iteration.  Legs: libdamc
(damc_specnorm_* around the training kernels), the stock modules (damc.training.stock_pytorch(): nn.utils.spectral_norm's
hook and MIOpen / rocBLAS, what the parent tree ran) and, for the cost of spectral norm itself, the same update of the
plain net on libdamc.  Device events around whole updates, warm-ups first, the legs alternating within each repeat.

usage: python tools/sn_update_ab.py [--reps 15] [--warmup 3] [--ngf 128] [--out FILE]
"""
import argparse
import contextlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "diffusion-amortized-mcmc_amd"), HERE]
from damc import synth, training  # noqa: E402
from src import diffusion_net as dn  # noqa: E402


def g_update(G, z, x):
    for p in G.parameters():
        p.grad = None
    loss = torch.sum((G(z) - x) ** 2, dim=[1, 2, 3]).mean()
    loss.backward()


def e_update(E, a, b):
    for p in E.parameters():
        p.grad = None
    e_pos, e_neg = E(a), E(b)
    (e_pos.mean() - e_neg.mean()).backward()


def timed(fn, ctx):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with ctx():
        t0.record()
        fn()
        t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ngf", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 128
    G_sn = synth.load_into(dn._netG_cifar10(nz=128, ngf=a.ngf, nc=3, use_spc_norm=True), 4).to(dev).train()
    G_pl = synth.load_into(dn._netG_cifar10(nz=128, ngf=a.ngf, nc=3), 0).to(dev).train()
    E_sn = synth.load_into(dn._netE(nz=128, e_sn=True), 5).to(dev).train()
    E_pl = synth.load_into(dn._netE(nz=128), 10).to(dev).train()
    z = torch.from_numpy(synth.normal_f32(2, 7, (B, 128))).to(dev)
    x = torch.from_numpy(synth.uniform_f32(1, 7, (B, 3, 32, 32))).to(dev)
    za = torch.from_numpy(synth.normal_f32(81, 0, (B, 128))).to(dev)
    zb = torch.from_numpy(synth.normal_f32(81, 1, (2 * B, 128))).to(dev)
    here, stock = contextlib.nullcontext, training.stock_pytorch
    groups = [
        ("G update, _netG_cifar10 ngf=%d B=%d" % (a.ngf, B),
         [("spectral norm, libdamc", lambda: g_update(G_sn, z, x), here),
          ("spectral norm, stock PyTorch", lambda: g_update(G_sn, z, x), stock),
          ("plain net, libdamc", lambda: g_update(G_pl, z, x), here)]),
        ("E update, _netE nz=128 B=%d/%d" % (B, 2 * B),
         [("spectral norm, libdamc", lambda: e_update(E_sn, za, zb), here),
          ("spectral norm, stock PyTorch", lambda: e_update(E_sn, za, zb), stock),
          ("plain net, libdamc", lambda: e_update(E_pl, za, zb), here)]),
    ]
    lines = ["spectral-norm G and E updates: device events around whole updates (forward, loss, backward), median "
             "(min .. max) ms of %d after %d warm-ups, legs alternating within each repeat, one process" % (a.reps, a.warmup)]
    for title, legs in groups:
        for _ in range(a.warmup):
            for _, fn, ctx in legs:
                timed(fn, ctx)
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in legs}
        for _ in range(a.reps):
            for name, fn, ctx in legs:
                times[name].append(timed(fn, ctx))
        base = sorted(times[legs[1][0]])[a.reps // 2]
        for name, _, _ in legs:
            t = sorted(times[name])
            lines.append("%-38s %-30s %8.3f ms (%.3f .. %.3f)  x%.2f of the stock leg"
                         % (title, name, t[a.reps // 2], t[0], t[-1], t[a.reps // 2] / base))
    out = "\n".join(lines)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
