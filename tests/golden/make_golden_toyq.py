#!/usr/bin/env python
"""Capture golden vectors of the toy amortizer from the REFERENCE implementation (build container only).

The reference's toy tree (workspace/toy_example) names its package `src` like the main tree and like the drop-in,
so it is imported in a process of its own, as make_golden.py does for the toy generator.  Recorded, with the field
names of the q_* goldens (make_golden.py capture_q / capture_qtrain):

  * q_toy.npz          _netQ_U_toy at its class defaults (n_interval 20, logsnr -20 / 20, 'small', no noise, no
                       residual; workspace/toy_example/src/diffusion_net.py:141-186), B = 21
  * q_toy_driver.npz   the driver's arguments (toy_example.py:71-76, 318-324: n_interval 100, logsnr -5.1 / 9.8,
                       'large', noise, residual), B = 21
  * q_toy_qtrain.npz   one calculate_loss(x, z, mask).mean().backward() of the driver's Q (toy_example.py:215-217)

Weights: synth.load_into(Q, SEED_Q); inputs: the counter-hash recipe with conftest's seeds.  B = 21 is one full
16-row tile plus a ragged one.  Nothing in tests/, bench.py or __graft_entry__ imports this script.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_toyq.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import REF_WS  # noqa: E402  (the reference checkout make_golden.py reads)

CHILD = r"""
import sys, types, os, json
import numpy as np
sys.dont_write_bytecode = True
repo, ws, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, os.path.join(repo, 'diffusion-amortized-mcmc_amd'))
import torch
torch.set_num_threads(8)
from damc import synth
sys.path.pop(0)
sys.path.insert(0, os.path.join(ws, 'toy_example'))
import src.diffusion_net as dn          # workspace/toy_example/src/diffusion_net.py
assert dn.__file__.startswith(ws), dn.__file__

SEED_Q, SEED_X, SEED_Z0, SEED_QN, SEED_QT = 20, 1, 2, 6, 7
B, nz = 21, 2
CONFIGS = {
    'q_toy': dict(),
    'q_toy_driver': dict(diffusion_residual=True, n_interval=100, logsnr_min=-5.1, logsnr_max=9.8, var_type='large',
                         with_noise=True, cond_w=0.0),
}


def patched(arrays):
    it = iter(arrays)
    saved = torch.randn, torch.randn_like
    torch.randn = lambda *a, **k: torch.from_numpy(next(it).copy())
    torch.randn_like = lambda t, **k: torch.from_numpy(next(it).copy())
    return saved


for name, kw in CONFIGS.items():
    Q = dn._netQ_U_toy(nz=nz, nxemb=128, ntemb=128, **kw)
    synth.load_into(Q, SEED_Q)
    Q.eval()
    n = Q.n_interval
    x = torch.from_numpy(synth.uniform_f32(SEED_X, 0, (B, 2)))
    zt0 = synth.normal_f32(SEED_QN, 0, (B, nz))
    pe_noise = synth.normal_f32(SEED_QN, 1, (B, nz))
    eps = [synth.normal_f32(SEED_QN, 100 + i, (B, nz)) for i in range(n - 1)]
    rec, log = {}, []
    h = Q.p.register_forward_hook(lambda m, i, o: log.append(o.detach().numpy().copy()))
    with torch.no_grad():
        rec['xemb'] = Q.encoder(x).numpy()
        rec['pe'] = Q.prior_emb(torch.from_numpy(pe_noise.copy())).numpy()
        saved = patched([zt0] + eps)                    # Q(x): randn for zt, then randn_like per step i > 0
        try:
            rec['q_post'] = Q(x).numpy()
        finally:
            torch.randn, torch.randn_like = saved
        rec['q_post_eps3'] = np.stack(log[:3])
        del log[:]
        saved = patched([pe_noise, zt0] + eps)          # Q(x=None, b): randn for prior_emb's input, randn for zt
        try:
            rec['q_prior'] = Q(x=None, b=B, device=torch.device('cpu')).numpy()
        finally:
            torch.randn, torch.randn_like = saved
        rec['q_prior_eps3'] = np.stack(log[:3])
    h.remove()
    meta = dict(kind='Qtoy', nz=nz, nxemb=128, ntemb=128, nf=4, B=B, residual=bool(Q.p.residual), var_type=Q.var_type,
                with_noise=bool(Q.with_noise), n_interval=n, logsnr_min=Q.logsnr_min, logsnr_max=Q.logsnr_max,
                q_keys=[[k, list(v.shape)] for k, v in Q.state_dict().items()])
    np.savez(os.path.join(out, name + '.npz'), meta=json.dumps(meta), **rec)
    print(name, 'done', flush=True)

# the Q update's loss (toy_example.py:215-217) with a mixed mask and injected draws, as make_golden.py capture_qtrain
Q = dn._netQ_U_toy(nz=nz, nxemb=128, ntemb=128, **CONFIGS['q_toy_driver'])
synth.load_into(Q, SEED_Q)
Q.train()
x = torch.from_numpy(synth.uniform_f32(SEED_X, 0, (B, 2)))
z = torch.from_numpy(synth.normal_f32(SEED_Z0, 0, (B, nz)))
mask = torch.ones(B, 1)
mask[1::3] = 0.0
pe = synth.normal_f32(SEED_QT, 0, (B, nz))
u = synth.uniform_f32(SEED_QT, 1, (B,), 0.0, 1.0)
eps = synth.normal_f32(SEED_QT, 2, (B, nz))
orig = torch.randn, torch.rand, torch.randn_like
torch.randn = lambda *a, **k: torch.from_numpy(pe.copy())
torch.rand = lambda *a, **k: torch.from_numpy(u.copy())
torch.randn_like = lambda t, **k: torch.from_numpy(eps.copy())
try:
    Q.zero_grad()
    loss = Q.calculate_loss(x=x, z=z, mask=mask)
    loss.mean().backward()
finally:
    torch.randn, torch.rand, torch.randn_like = orig
rec = {'loss': loss.detach().numpy()}
params = []
for pname, p in Q.named_parameters():
    if p.grad is None:
        continue
    g = p.grad.detach().numpy().reshape(-1)
    st = max(1, g.size // 512)
    rec['grad%d_sub' % len(params)] = g[::st].copy()
    rec['grad%d_norm' % len(params)] = np.float64(np.linalg.norm(g.astype(np.float64)))
    params.append([pname, st, list(p.shape)])
np.savez(os.path.join(out, 'q_toy_qtrain.npz'), meta=json.dumps(dict(kind='Qtrain', q='q_toy_driver', params=params)),
         **rec)
print('q_toy_qtrain done')
"""


def main():
    subprocess.check_call([sys.executable, "-c", CHILD, REPO, REF_WS, HERE],
                          env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    print("done")


if __name__ == "__main__":
    main()
