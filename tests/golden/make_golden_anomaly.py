#!/usr/bin/env python
"""Capture the golden vectors of the anomaly-detection scoring loop from the REFERENCE implementation (build
container only).

The loop body of workspace/eval_anomaly_det.py:100-119 (train_anomaly_det.py:211-228 is the same with 10 steps):
z0 = Q(x) under no_grad, 5 noiseless steps of sample_langevin_post_z_with_prior (MCMC.py:48-74; step 0.1, sigma 1,
the driver's defaults), then the per-sample score with the driver's own expression.  A child process imports the
reference's `src` from REF_WS (the drop-in package carries the same name) and only calls it.

  * anomaly_mnist_s.npz   _netG_mnist(nz 8, ngf 16, nc 1), _netE(nz 8), _netQ_U(mnist, nz 8, nxemb 64, ntemb 32,
                          nif 8, n_interval 10, 'large', noise, residual, cond_w 0; logsnr -5.1 / 9.8), B = 21
      z0 (B, nz)   Q(x)                     zK (B, nz)    after the 5 steps
      terms (B, 3) {sum (G(zK)-x)^2, E(zK), sum zK^2 / 2}   score (B)   the driver's expression

Weights: synth.load_into with conftest's seeds; x and the injected draws of Q(x): the counter-hash recipe, as
make_golden.py capture_q.  Nothing in tests/, bench.py or __graft_entry__ imports this script.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_anomaly.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import REF_WS  # noqa: E402  (the reference checkout make_golden.py reads)

CHILD = r"""
import sys, os, json
import numpy as np
sys.dont_write_bytecode = True
here, ws, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, here)
import make_golden as mg                  # damc.synth, then our `src` off the path; the noise-injection helpers
import torch
torch.set_num_threads(8)
dn, mc = mg.import_reference()            # workspace/src/diffusion_net.py, workspace/src/MCMC.py
assert dn.__file__.startswith(ws) and mc.__file__.startswith(ws), (dn.__file__, mc.__file__)
synth = mg.synth

B, nz, ngf, nc, H = 21, 8, 16, 1, 28
qkw = dict(nc=nc, nz=nz, nxemb=64, ntemb=32, nif=8, diffusion_residual=True, n_interval=10, logsnr_min=-5.1,
           logsnr_max=9.8, var_type='large', with_noise=True, cond_w=0.0, net_arch='A', dataset='mnist')
steps, step, sigma = 5, 0.1, 1.0

G = dn._netG_mnist(nz=nz, ngf=ngf, nc=nc)
E = dn._netE(nz=nz)
Q = dn._netQ_U(**qkw)
synth.load_into(G, mg.SEED_G)
synth.load_into(E, mg.SEED_E)
synth.load_into(Q, mg.SEED_Q)
G.eval(), E.eval(), Q.eval()
x = torch.from_numpy(synth.uniform_f32(mg.SEED_X, 0, (B, nc, H, H)))

q = mg.NoiseQueue()                       # Q(x): randn for zt, then randn_like per step i > 0
q.push(synth.normal_f32(mg.SEED_QN, 0, (B, nz)))
for i in range(qkw['n_interval'] - 1):
    q.push(synth.normal_f32(mg.SEED_QN, 100 + i, (B, nz)))
saved = mg.patch_randn(torch, q)
try:
    with torch.no_grad():
        z0 = Q(x)
finally:
    torch.randn, torch.randn_like = saved
assert not q.items

zk_pos = z0.detach().clone()
zk_pos.requires_grad = True
zk_pos = mc.sample_langevin_post_z_with_prior(z=zk_pos, x=x, netG=G, netE=E, g_l_steps=steps, g_llhd_sigma=sigma,
                                              g_l_with_noise=False, g_l_step_size=step, verbose=False)
with torch.no_grad():
    x_hat = G(zk_pos)
    s_hat = E(zk_pos)
    recon = torch.sum((x_hat - x) ** 2, dim=[1, 2, 3])
    half_z2 = torch.sum(zk_pos ** 2, dim=-1) * 0.5
    score = recon * 1 + s_hat + half_z2

meta = dict(kind='anomaly', ctor='_netG_mnist', nz=nz, ngf=ngf, nc=nc, H=H, B=B, q=qkw, steps=steps, step=step,
            sigma=sigma, recon_weight=1.0,
            g_keys=[[k, list(v.shape)] for k, v in G.state_dict().items()],
            e_keys=[[k, list(v.shape)] for k, v in E.state_dict().items()],
            q_keys=[[k, list(v.shape)] for k, v in Q.state_dict().items()])
np.savez(os.path.join(out, 'anomaly_mnist_s.npz'), meta=json.dumps(meta), z0=z0.numpy(), zK=zk_pos.numpy(),
         terms=torch.stack([recon, s_hat, half_z2], dim=1).numpy(), score=score.numpy())
print('anomaly_mnist_s done', float(score.min()), float(score.max()))
"""


def main():
    subprocess.check_call([sys.executable, "-c", CHILD, HERE, REF_WS, HERE],
                          env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    print("done")


if __name__ == "__main__":
    main()
