"""Shared by tests/test_anomaly_cpu.py and tests/test_gpu_anomaly.py: the anomaly golden's nets and inputs, the
driver's score expression on stock modules, and a host-side generator descriptor."""
import numpy as np

from conftest import SEED_E, SEED_G, SEED_Q, SEED_X, load_golden

RR_CHUNK = 16384  # csrc/energy.hip: elements of a row one workgroup sums


def build_anomaly_case(device="cpu"):
    """Drop-in G, E, Q of tests/golden/anomaly_mnist_s.npz (counter-hash weights, eval mode), its x, and the record."""
    import torch

    from damc import synth
    from src import diffusion_net as dn

    rec, meta = load_golden("anomaly_mnist_s")
    G = synth.load_into(getattr(dn, meta["ctor"])(nz=meta["nz"], ngf=meta["ngf"], nc=meta["nc"]), SEED_G)
    E = synth.load_into(dn._netE(nz=meta["nz"]), SEED_E)
    Q = synth.load_into(dn._netQ_U(**meta["q"]), SEED_Q)
    for m in (G, E, Q):
        m.to(device).eval()
    B, nc, H = meta["B"], meta["nc"], meta["H"]
    x = torch.from_numpy(synth.uniform_f32(SEED_X, 0, (B, nc, H, H))).to(device)
    return dict(G=G, E=E, Q=Q, x=x, rec=rec, meta=meta)


def driver_terms(G, E, z, x, recon_weight=1.0):
    """The drivers' expression (eval_anomaly_det.py:115-117) on the modules themselves, in their dtype:
    (terms (B, 3), score (B,)) as numpy."""
    import torch

    with torch.no_grad():
        x_hat = G(z)
        recon = torch.sum((x_hat - x) ** 2, dim=list(range(1, x.dim())))
        e = E(z).reshape(-1) if E is not None else torch.zeros_like(recon)
        hz = torch.sum(z ** 2, dim=-1) * 0.5
        score = recon * recon_weight + e + hz
    return torch.stack([recon, e, hz], dim=1).cpu().numpy(), score.cpu().numpy()


def oracle_terms(G, E, z, x, recon_weight=1.0, dtype=None):
    """The same terms on the oracle (oracle/damc_oracle.py) in dtype (default fp64), from CPU copies of the nets."""
    import torch

    from oracle import damc_oracle as orc

    dtype = dtype or torch.float64
    z, x = z.detach().cpu().to(dtype), x.detach().cpu().to(dtype)
    xh = orc.generator_sample(orc.generator_layers(G, dtype), z)
    recon = ((xh - x.reshape(xh.shape)) ** 2).reshape(len(z), -1).sum(1)
    e = orc.ebm_energy_grad(orc.ebm_params(E, dtype), z)[0] if E is not None else torch.zeros_like(recon)
    hz = 0.5 * (z ** 2).sum(1)
    return torch.stack([recon, e, hz], dim=1).numpy(), (recon_weight * recon + e + hz).numpy()


def host_generator_desc(G):
    """damc_generator_t of a generator module with no device pointers (host-side size queries and argument checks)."""
    from damc import _lib
    from damc.plans import GeneratorPlan

    p = GeneratorPlan(G)
    g = _lib.Generator()
    g.n_layers, g.nz, g.nc, g.h, g.w = len(p.layers), p.nz, p.nc, p.h, p.w
    for i, spec in enumerate(p.layers):
        d = g.layers[i]
        d.kind, d.cin, d.cout, d.k, d.stride, d.pad = (spec[k] for k in ("kind", "cin", "cout", "k", "stride", "pad"))
        d.hin = d.win = spec["hin"]
        d.hout = d.wout = spec["hout"]
        d.act, d.slope = spec["act"], spec["slope"]
    return g


def l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))
