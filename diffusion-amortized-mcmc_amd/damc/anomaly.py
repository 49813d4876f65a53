"""Anomaly scoring (workspace/eval_anomaly_det.py:100-126, train_anomaly_det.py:206-248) on libdamc.

Per test image the drivers take z0 = Q(x), a few noiseless posterior Langevin steps, the per-sample score
|G(z)-x|^2 + E(z) + |z|^2/2, and the area under the precision-recall curve of the scores over the test set.
``posterior_energy`` is the per-sample read-out (damc_posterior_energy: fixed summation order, no atomics, no host
synchronisation, a row's value independent of the batch it sits in), ``score`` the drivers' loop body as one call,
``pr_auc`` the host-side metric (numpy, fp64; scikit-learn's precision_recall_curve + auc without scikit-learn).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .langevin import _f32c, posterior_langevin
from .plans import ebm_plan, generator_plan, spectral_norm_step


def posterior_energy(z, x, G, E, recon_weight=1.0, return_xhat=False):
    """Per-sample terms of U at z: returns (terms (B, 3) = {|G(z)-x|^2, E(z), |z|^2/2}, score (B,)) with
    score = recon_weight * terms[:, 0] + terms[:, 1] + terms[:, 2] (fp32, left to right), and G(z) as a third value
    if return_xhat.  E=None (the toy model) leaves terms[:, 1] at 0.  z and x are only read."""
    z = _f32c(z.detach(), "z")
    dev = z.device
    x = x.detach().to(device=dev, dtype=torch.float32).contiguous()
    B = z.shape[0]
    gp = generator_plan(G)
    if z.dim() != 2 or z.shape[1] != gp.nz or x.shape[0] != B or x.numel() != B * gp.nc * gp.h * gp.w:
        raise _lib.DamcError("shape mismatch: z %s x %s for generator nz=%d out=(%d,%d,%d)"
                             % (tuple(z.shape), tuple(x.shape), gp.nz, gp.nc, gp.h, gp.w))
    ep = ebm_plan(E) if E is not None else None
    with spectral_norm_step(gp.sn_train()):  # one G forward (train-mode spectral norm: one power iteration)
        gdesc = gp.refresh(dev)
    edesc = None
    if ep is not None:
        with spectral_norm_step(ep.sn_train()):  # one E forward
            edesc = ep.refresh(dev)
    L = _lib.lib()
    nbytes = int(L.damc_posterior_energy_workspace_bytes(ctypes.byref(gdesc), B))
    if nbytes == 0:
        raise _lib.DamcError("unsupported generator configuration for the HIP path")
    if getattr(gp, "_ws_energy", None) is None:
        gp._ws_energy = _lib.WorkspaceCache()
    ws = gp._ws_energy.get(dev, nbytes, B)
    terms = torch.empty(B, 3, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    xhat = None
    if return_xhat:
        xhat = torch.empty((B, gp.nc, gp.h, gp.w) if gp.is_conv else (B, gp.nc), dtype=torch.float32, device=dev)
    check(L.damc_posterior_energy(ctypes.byref(gdesc), ctypes.byref(edesc) if edesc is not None else None, ptr(z),
                                  ptr(x), B, float(recon_weight), ptr(terms), ptr(score), ptr(xhat), ptr(ws), nbytes,
                                  _lib.stream_ptr(dev)), "damc_posterior_energy")
    return (terms, score, xhat) if return_xhat else (terms, score)


def recon_rows(xhat, x):
    """Per-op hook: sum_j (xhat[b, j] - x[b, j])^2 per row of two (B, ...) tensors (damc_recon_rows)."""
    xhat, x = _f32c(xhat, "xhat"), _f32c(x, "x")
    if xhat.shape != x.shape or xhat.dim() < 2:
        raise _lib.DamcError("xhat and x must share a (B, ...) shape")
    B, n = xhat.shape[0], xhat[0].numel()
    L = _lib.lib()
    nbytes = int(L.damc_recon_rows_workspace_bytes(B, n))
    if nbytes == 0:
        raise _lib.DamcError("recon_rows: empty or oversize shape %s" % (tuple(x.shape),))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    check(L.damc_recon_rows(ptr(xhat), ptr(x), B, n, ptr(out), ptr(ws), nbytes, _lib.stream_ptr(x.device)),
          "damc_recon_rows")
    return out


def score(Q, G, E, x, g_l_steps=5, g_l_step_size=0.1, g_llhd_sigma=1.0, recon_weight=1.0, zt=None, seed=None,
          chain_base=0):
    """The drivers' scoring loop body: z0 = Q(x) under no_grad, g_l_steps noiseless posterior Langevin steps, the
    per-sample score.  Returns (score (B,), z (B, nz)).  The defaults are eval_anomaly_det.py's (the training
    driver's evaluation runs 10 steps).  Draws exactly what q_forward draws, in its order; zt / seed / chain_base as
    in q_forward (a shard passes its slice of the global zt, the global seed and its slice start)."""
    from . import amortizer

    with torch.no_grad():
        z = amortizer.q_forward(Q, x=x, zt=zt, seed=seed, chain_base=chain_base)
    posterior_langevin(z, x, G, E, g_l_steps, g_llhd_sigma, g_l_step_size, False, chain_base=chain_base)
    _, s = posterior_energy(z, x, G, E, recon_weight=recon_weight)
    return s, z


def pr_auc(labels, scores):
    """Area under the precision-recall curve as sklearn.metrics.precision_recall_curve followed by
    auc(recall, precision) computes it (the drivers' metric), in fp64 on the host: one curve point per distinct score
    (a threshold takes every sample that ties with it), the end point (recall 0, precision 1) appended, trapezoids
    over recall.  labels: 1 (or True) marks a positive.  Raises ValueError for a length mismatch, a non-finite score
    or a label vector without a positive."""
    y = np.asarray(labels).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if y.shape[0] != s.shape[0]:
        raise ValueError("labels and scores differ in length: %d vs %d" % (y.shape[0], s.shape[0]))
    if not np.all(np.isfinite(s)):
        raise ValueError("scores must be finite")
    pos = (y == 1).astype(np.float64)
    if pos.sum() == 0:
        raise ValueError("labels hold no positive sample: recall is undefined")
    order = np.argsort(s, kind="mergesort")[::-1]  # decreasing score
    s, pos = s[order], pos[order]
    last = np.r_[np.nonzero(np.diff(s))[0], s.size - 1]  # last sample of each run of equal scores
    tp = np.cumsum(pos)[last]
    fp = (1.0 + last) - tp
    precision = tp / (tp + fp)
    recall = tp / tp[-1]
    # the curve runs from the lowest threshold (recall 1) to the highest, then to (recall 0, precision 1)
    precision = np.r_[precision[::-1], 1.0]
    recall = np.r_[recall[::-1], 0.0]
    # auc(recall, precision): x decreases, so the trapezoid sum is negated
    return float(-np.sum(np.diff(recall) * (precision[1:] + precision[:-1]) * 0.5))
