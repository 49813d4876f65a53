"""Shared by tests/test_toyq_cpu.py and tests/test_gpu_toyq.py: the toy amortizer's golden cases
(tests/golden/q_toy*.npz, captured by tests/golden/make_golden_toyq.py) and their fp64 oracle."""
import numpy as np

from conftest import SEED_Q, SEED_QN, SEED_X, load_golden

TOY_NAMES = ["q_toy", "q_toy_driver"]
_FP64 = {}


def build_toy_case(name, device="cpu"):
    """The drop-in _netQ_U_toy of a golden case with counter-hash weights, and the case's inputs."""
    import torch

    from damc import synth
    from src import diffusion_net as dn

    rec, m = load_golden(name)
    Q = dn._netQ_U_toy(nz=m["nz"], nxemb=m["nxemb"], ntemb=m["ntemb"], nf=m["nf"], diffusion_residual=m["residual"],
                       n_interval=m["n_interval"], logsnr_min=m["logsnr_min"], logsnr_max=m["logsnr_max"],
                       var_type=m["var_type"], with_noise=m["with_noise"], cond_w=0.0)
    synth.load_into(Q, SEED_Q)
    Q.to(device).eval()
    B, nz, n = m["B"], m["nz"], m["n_interval"]
    x = torch.from_numpy(synth.uniform_f32(SEED_X, 0, (B, 2))).to(device)
    zt0 = torch.from_numpy(synth.normal_f32(SEED_QN, 0, (B, nz))).to(device)
    pe_noise = torch.from_numpy(synth.normal_f32(SEED_QN, 1, (B, nz))).to(device)
    eps = torch.from_numpy(np.stack([synth.normal_f32(SEED_QN, 100 + i, (B, nz)) for i in range(n - 1)]))
    return dict(Q=Q, x=x, zt0=zt0, pe_noise=pe_noise, eps=eps.to(device), rec=rec, meta=m)


def toy_fp64(name):
    """fp64 evaluation of the case on the drop-in (orc.reverse_sweep / orc.prior_embedding, Q.encoder.double() for the
    MLP): xemb, pe, and eps of steps 1-3 and the end-point of the posterior and the prior sweep.  Cached per case."""
    if name not in _FP64:
        import torch

        from oracle import damc_oracle as orc

        c = build_toy_case(name)
        Q, m = c["Q"].double(), c["meta"]
        args = (m["n_interval"], m["logsnr_min"], m["logsnr_max"], m["var_type"])
        with torch.no_grad():
            xemb = Q.encoder(c["x"].double())
            zp, ep = orc.reverse_sweep(Q, xemb, c["zt0"].double(), c["eps"].double(), *args,
                                       with_noise=m["with_noise"])
            pe = orc.prior_embedding(Q, c["pe_noise"].double())
            zq, eq = orc.reverse_sweep(Q, pe, c["zt0"].double(), c["eps"].double(), *args, with_noise=m["with_noise"])
        _FP64[name] = dict(xemb=xemb.numpy(), pe=pe.numpy(), post=zp.numpy(), post_eps=[e.numpy() for e in ep[:3]],
                           prior=zq.numpy(), prior_eps=[e.numpy() for e in eq[:3]])
    return _FP64[name]
