"""GPU: the toy amortizer's Q update on libdamc (workspace/toy_example/src/diffusion_net.py:241-263 as the driver runs
it, toy_example.py:209-219): the fused MLP's training calls (damc_mlp_train_*) for the encoder and prior_emb, and the
denoiser's training kernels at an even nz that is no multiple of 4.

Gradient criterion, the one tests/test_gpu_training.py applies to the q_*_qtrain goldens: per tensor, the error
relative to the tensor's norm (floored at 1e-3 x the largest gradient norm of the module, so an analytically zero
gradient is held to that floor) is below 1e-4 or twice the error of the stock PyTorch layers' fp32 autograd on this
GPU, whichever is larger.  Every figure is printed before it is asserted."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import SEED_Q, rel_l2
from toyq_util import build_toy_case

pytestmark = pytest.mark.gpu

DRIVER_LR, DRIVER_WD, DRIVER_BETAS, DRIVER_MAX_NORM = 2e-4, 1e-2, (0.5, 0.999), 100.0  # toy_example.py:91, 334-336


def _errs(got, ref):
    """Per-tensor |got - ref| / max(|ref|, 1e-3 x the largest |ref|) (conftest.gtrain_check's measure, whole tensors)."""
    ref = [np.asarray(r, dtype=np.float64) for r in ref]
    floor = 1e-3 * max(np.linalg.norm(r) for r in ref)
    return [float(np.linalg.norm(np.asarray(g, dtype=np.float64) - r) / max(np.linalg.norm(r), floor, 1e-30))
            for g, r in zip(got, ref)]


def _check(label, names, got, stock, ref):
    e_hip, e_stock = _errs(got, ref), _errs(stock, ref)
    worst = 0.0
    for n, a, b in zip(names, e_hip, e_stock):
        tol = max(1e-4, 2.0 * b)
        worst = max(worst, a / tol)
        if a >= 0.25 * tol:
            print("%s %s: |hip - fp64| %.2e  |stock fp32 - fp64| %.2e  bound %.2e" % (label, n, a, b, tol))
    print("%s: worst |hip - fp64| %.2e (largest share of its bound %.2f), worst |stock - fp64| %.2e"
          % (label, max(e_hip), worst, max(e_stock)))
    for n, a, b in zip(names, e_hip, e_stock):
        assert a < max(1e-4, 2.0 * b), (label, n, a, b)


# --------------------------------------------------------------------- 1. the update against the reference's golden
def test_toy_q_update_runs_on_libdamc_and_matches_reference(gpu_device, monkeypatch):
    """test_gpu_toyq.test_toy_q_update_matches_reference's case and tolerances (q_toy_qtrain: the driver config at
    B = 21, mask rows 1::3 zeroed), with the path pinned: no nn.Linear of Q runs its forward, and the encoder, prior_emb
    and the denoiser each went through libdamc (mlp_apply twice, denoiser_apply once, none declined)."""
    from conftest import SEED_QT, SEED_Z0, gtrain_check, gtrain_errors, load_golden

    from damc import synth, training

    rec, meta = load_golden("q_toy_qtrain")
    fired, calls = [], []

    def run(hooks):
        c = build_toy_case(meta["q"], gpu_device)
        Q, x, m = c["Q"], c["x"], c["meta"]
        B, nz = m["B"], m["nz"]
        Q.train()
        if hooks:
            for name, mod in Q.named_modules():
                if isinstance(mod, torch.nn.Linear):
                    mod.register_forward_hook(lambda _m, _i, _o, name=name: fired.append(name))
        z = torch.from_numpy(synth.normal_f32(SEED_Z0, 0, (B, nz))).to(gpu_device)
        mask = torch.ones(B, 1, device=gpu_device)
        mask[1::3] = 0.0
        pe = synth.normal_f32(SEED_QT, 0, (B, nz))
        u = synth.uniform_f32(SEED_QT, 1, (B,), 0.0, 1.0)
        eps = synth.normal_f32(SEED_QT, 2, (B, nz))
        orig = torch.randn, torch.rand, torch.randn_like
        torch.randn = lambda *a, **k: torch.from_numpy(pe.copy()).to(k.get("device") or "cpu")
        torch.rand = lambda *a, **k: torch.from_numpy(u.copy())
        torch.randn_like = lambda t, **k: torch.from_numpy(eps.copy()).to(t.device)
        try:
            Q.zero_grad()
            loss = Q.calculate_loss(x=x, z=z, mask=mask)
            loss.mean().backward()
        finally:
            torch.randn, torch.rand, torch.randn_like = orig
        return loss.detach().cpu().numpy(), [p.grad.detach().cpu().numpy() for p in Q.parameters() if p.grad is not None]

    with training.stock_pytorch():
        _, g_stock = run(False)
    tol = [max(1e-4, 2.0 * max(e)) for e in gtrain_errors(g_stock, rec, meta)]

    def recording(fn_name):
        fn = getattr(training, fn_name)

        def wrapped(*a, **k):
            out = fn(*a, **k)
            calls.append((fn_name, out is not None))
            return out
        return wrapped

    monkeypatch.setattr(training, "mlp_apply", recording("mlp_apply"))
    monkeypatch.setattr(training, "denoiser_apply", recording("denoiser_apply"))
    loss, grads = run(True)
    print("toy Q update on libdamc: loss %.2e, calls %s" % (rel_l2(loss, rec["loss"]), calls))
    assert not fired, "stock nn.Linear forwards ran: %s" % fired
    assert sorted(calls) == [("denoiser_apply", True), ("mlp_apply", True), ("mlp_apply", True)]
    assert rel_l2(loss, rec["loss"]) < 1e-5
    worst = gtrain_check(grads, rec, meta, tol)
    print("toy Q update on libdamc: worst rel err vs reference %.2e (largest bound %.2e)" % (worst, max(tol)))


# ------------------------------------------------------------------------------------------ 2. the MLP in isolation
def _toy_mlp(which):
    from damc import synth

    if which == "encoder":  # toy_example/src/diffusion_net.py:166-174
        seq = torch.nn.Sequential(torch.nn.Linear(2, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128), torch.nn.ReLU(),
                                  torch.nn.Linear(128, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128))
    else:                   # :180-184
        seq = torch.nn.Sequential(torch.nn.Linear(2, 128), torch.nn.LeakyReLU(), torch.nn.Linear(128, 128))
    synth.load_into(seq, SEED_Q + (1 if which == "encoder" else 2))
    return seq


_MLP_REF = {}


def _mlp_reference(which, B):
    """(x, grad_out, fp64 out and parameter gradients by autograd on the host), computed once per case."""
    if (which, B) not in _MLP_REF:
        from damc import synth

        seq = _toy_mlp(which)
        x = synth.normal_f32(31, B, (B, 2))
        g = synth.normal_f32(32, B, (B, 128))
        s64 = copy.deepcopy(seq).double()
        out = s64(torch.from_numpy(x).double())
        out.backward(torch.from_numpy(g).double())
        _MLP_REF[(which, B)] = (x, g, out.detach().numpy(), [p.grad.numpy() for p in s64.parameters()])
    return _MLP_REF[(which, B)]


@pytest.mark.parametrize("B", [1, 16, 21, 37])
@pytest.mark.parametrize("which", ["encoder", "prior_emb"])
def test_mlp_train_forward_and_backward(gpu_device, which, B):
    from damc import _lib
    from damc import amortizer as am

    L = _lib.lib()
    x_np, g_np, out64, grads64 = _mlp_reference(which, B)
    seq = _toy_mlp(which).to(gpu_device)
    x = torch.from_numpy(x_np).to(gpu_device)
    g = torch.from_numpy(g_np).to(gpu_device)
    d, keep = am.mlp_desc(seq, gpu_device)
    nsaved = int(L.damc_mlp_train_saved_floats(ctypes.byref(d), B))
    nws = int(L.damc_mlp_train_workspace_bytes(ctypes.byref(d), B))
    assert nsaved > 0 and nws > 0
    stream = _lib.stream_ptr(gpu_device)
    saved = torch.full((nsaved,), float("nan"), device=gpu_device)
    out = torch.empty(B, 128, device=gpu_device)
    _lib.check(L.damc_mlp_train_forward(ctypes.byref(d), _lib.ptr(x), B, _lib.ptr(saved), _lib.ptr(out), stream))
    # out is the plain forward's, bit for bit; saved holds every hidden layer's post-activation rows
    assert torch.equal(out, am.mlp_forward(seq, x))
    lins = [i for i, m in enumerate(seq) if isinstance(m, torch.nn.Linear)]
    off = 0
    for i in lins[:-1]:
        h = am.mlp_forward(seq[:i + 2], x)  # Linear i and its activation
        assert torch.equal(saved[off:off + h.numel()].view_as(h), h), "saved activations of module %d" % i
        off += h.numel()
    assert rel_l2(out.cpu().numpy(), out64) < 1e-5

    params = list(seq.parameters())
    sizes = [p.numel() for p in params]
    SENTINEL = -777.0

    def backward(skip=None):
        flat = torch.full((sum(sizes),), SENTINEL, device=gpu_device)
        parts = [t.view(p.shape) for t, p in zip(flat.split(sizes), params)]
        grads = _lib.MlpGrads()
        for k, t in enumerate(parts):
            if k != skip:
                getattr(grads, "w" if k % 2 == 0 else "b")[k // 2] = t.data_ptr()
        ws = torch.empty(nws, dtype=torch.uint8, device=gpu_device)
        _lib.check(L.damc_mlp_train_backward(ctypes.byref(d), _lib.ptr(x), _lib.ptr(saved), _lib.ptr(g), B,
                                             ctypes.byref(grads), _lib.ptr(ws), nws, stream))
        torch.cuda.synchronize()
        return parts

    got = backward()
    assert all(torch.isfinite(t).all() for t in got)
    # stock fp32 autograd on this GPU: the yardstick's own error
    stock = copy.deepcopy(seq)
    stock(x).backward(g)
    names = [n for n, _ in seq.named_parameters()]
    _check("%s B=%d" % (which, B), names, [t.cpu().numpy() for t in got],
           [p.grad.cpu().numpy() for p in stock.parameters()], grads64)
    # the same bits every run
    again = backward()
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # a NULL entry is skipped: its tensor keeps what it held, every other gradient is unchanged
    for skip in (2, len(params) - 1):  # the second layer's weight, the last layer's bias
        part = backward(skip=skip)
        assert bool((part[skip] == SENTINEL).all())
        assert all(torch.equal(a, b) for k, (a, b) in enumerate(zip(got, part)) if k != skip)


# ------------------------------------------------------------------------------- 3. the denoiser at a narrow nz
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("B", [1, 21])
@pytest.mark.parametrize("nz", [2, 6])
def test_denoiser_train_narrow_nz(gpu_device, nz, B, residual):
    """Diffusion_Unet(nz) for nz % 4 != 0 (nz = 6: an odd nz / 2) through damc_denoiser_train_*: eps_pred and the
    gradients w.r.t. zt, xemb and every parameter against fp64 autograd on the drop-in's stock layers."""
    from damc import synth, training
    from src import diffusion_net as dn

    def make():
        p = dn.Diffusion_Unet(nz=nz, nxemb=128, ntemb=128, residual=residual)
        synth.load_into(p, SEED_Q + nz)
        return p

    zt_np = synth.normal_f32(41, nz, (B, nz))
    xe_np = synth.normal_f32(42, nz, (B, 128))
    ls_np = synth.uniform_f32(43, nz, (B,), -5.0, 9.0)
    go_np = synth.normal_f32(44, nz, (B, nz))

    def run(p, device, dtype):
        zt = torch.from_numpy(zt_np).to(device=device, dtype=dtype).requires_grad_(True)
        xe = torch.from_numpy(xe_np).to(device=device, dtype=dtype).requires_grad_(True)
        ls = torch.from_numpy(ls_np).to(device=device, dtype=dtype)
        eps = p(z=zt, logsnr=ls, xemb=xe)
        eps.backward(torch.from_numpy(go_np).to(device=device, dtype=dtype))
        return ([eps.detach().cpu().numpy(), zt.grad.cpu().numpy(), xe.grad.cpu().numpy()] +
                [q.grad.cpu().numpy() for q in p.parameters()])

    ref = run(make().double(), "cpu", torch.float64)
    with training.stock_pytorch():
        stock = run(make().to(gpu_device), gpu_device, torch.float32)
    calls = []
    orig = training.denoiser_apply
    training.denoiser_apply = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        got = run(make().to(gpu_device), gpu_device, torch.float32)
        again = run(make().to(gpu_device), gpu_device, torch.float32)
    finally:
        training.denoiser_apply = orig
    assert len(calls) == 2, "the denoiser did not run on libdamc"
    names = ["eps_pred", "d zt", "d xemb"] + [n for n, _ in make().named_parameters()]
    label = "denoiser nz=%d B=%d residual=%d" % (nz, B, residual)
    assert all(np.isfinite(t).all() for t in got)
    # eps_pred is a forward value: against its own norm; the gradients share the module's floor
    _check(label, names[:1], got[:1], stock[:1], ref[:1])
    _check(label, names[1:], got[1:], stock[1:], ref[1:])
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------------------- 4. six updates, as the driver's
def _driver_case(gpu_device, B=500):
    from damc import synth

    c = build_toy_case("q_toy_driver", gpu_device)
    Q = c["Q"]
    x = torch.from_numpy(synth.uniform_f32(51, 0, (B, 2))).to(gpu_device)
    z = torch.from_numpy(synth.normal_f32(52, 0, (B, Q.nz))).to(gpu_device)
    mask = (torch.from_numpy(synth.uniform_f32(53, 0, (B, 1), 0.0, 1.0)) >= 0.1).float().to(gpu_device)  # p_mask 0.1
    draws = [(synth.normal_f32(54, k, (B, Q.nz)), synth.uniform_f32(55, k, (B,), 0.0, 1.0),
              synth.normal_f32(56, k, (B, Q.nz))) for k in range(6)]
    return Q, x, z, mask, draws


class _pinned_draws:
    """torch.randn / rand / randn_like return the given arrays, in calculate_loss's order (prior_emb's noise on the
    device, u on the host unless `u_on_device`, eps like z)."""

    def __init__(self, pe, u, eps, device, u_on_device=False):
        self.pe, self.u, self.eps = (torch.as_tensor(t) for t in (pe, u, eps))
        self.device, self.u_dev = device, u_on_device
        if u_on_device:  # nothing crosses from the host inside a capture
            self.pe, self.u, self.eps = (t.to(device) for t in (self.pe, self.u, self.eps))

    def __enter__(self):
        self.orig = torch.randn, torch.rand, torch.randn_like
        torch.randn = lambda *a, **k: self.pe.clone().to(k.get("device") or "cpu")
        torch.rand = lambda *a, **k: self.u.clone().to(self.device) if self.u_dev else self.u.clone()
        torch.randn_like = lambda t, **k: self.eps.clone().to(t.device)

    def __exit__(self, *exc):
        torch.randn, torch.rand, torch.randn_like = self.orig


def _update(Q, opt, x, z, mask):
    opt.zero_grad(set_to_none=True)
    loss = Q.calculate_loss(x=x, z=z, mask=mask).mean()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(Q.parameters(), max_norm=DRIVER_MAX_NORM)
    opt.step()
    return loss.detach()


def test_six_driver_updates_match_stock(gpu_device):
    """Six updates at the driver's B = 500 with AdamW and clip_grad_norm_ (toy_example.py:91, 211-219), draws pinned:
    libdamc and the stock layers from the same initial weights.  Losses within 1e-5 each, final parameters within 1e-4
    rel-L2 per tensor (the project's per-tensor floor)."""
    from damc import training

    def six(stock):
        Q, x, z, mask, draws = _driver_case(gpu_device)
        Q.train()
        opt = torch.optim.AdamW(Q.parameters(), weight_decay=DRIVER_WD, lr=DRIVER_LR, betas=DRIVER_BETAS)
        losses = []
        for pe, u, eps in draws:
            with _pinned_draws(pe, u, eps, gpu_device):
                if stock:
                    with training.stock_pytorch():
                        losses.append(_update(Q, opt, x, z, mask))
                else:
                    losses.append(_update(Q, opt, x, z, mask))
        torch.cuda.synchronize()
        return ([float(v) for v in losses], [n for n, _ in Q.named_parameters()],
                [p.detach().cpu().numpy() for p in Q.parameters()])

    l_stock, names, p_stock = six(True)
    l_hip, _, p_hip = six(False)
    dl = [abs(a - b) / max(abs(b), 1e-30) for a, b in zip(l_hip, l_stock)]
    dp = [rel_l2(a, b) for a, b in zip(p_hip, p_stock)]
    k = int(np.argmax(dp))
    print("six updates B=500: loss rel diff %s; worst parameter %s %.2e" % (["%.1e" % v for v in dl], names[k], dp[k]))
    assert all(np.isfinite(l_hip))
    assert max(dl) <= 1e-5
    for n, v in zip(names, dp):
        assert v <= 1e-4, (n, v)


def test_one_update_replays_from_a_captured_graph(gpu_device):
    """calculate_loss -> backward -> clip_grad_norm_ -> AdamW.step at B = 500 recorded into a graph (the u draw handed
    over as a device tensor; AdamW capturable): from the same weights and optimiser state, the replay's loss and
    parameters are bitwise the eager update's."""
    pe, u, eps = _driver_case(gpu_device)[4][0]

    def fresh():
        Q, x, z, mask, _ = _driver_case(gpu_device)
        Q.train()
        opt = torch.optim.AdamW(Q.parameters(), weight_decay=DRIVER_WD, lr=DRIVER_LR, betas=DRIVER_BETAS,
                                capturable=True)
        return Q, opt, x, z, mask

    eager, replayed = fresh(), fresh()  # built before torch.randn is pinned: the constructors draw from it
    draws = _pinned_draws(pe, u, eps, gpu_device, u_on_device=True)  # kept: the replays read its device tensors
    with draws:
        Q, opt, x, z, mask = eager
        loss_e = _update(Q, opt, x, z, mask).clone()
        torch.cuda.synchronize()
        p_eager = [p.detach().clone() for p in Q.parameters()]

        Q, opt, x, z, mask = replayed
        w0 = [p.detach().clone() for p in Q.parameters()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                _update(Q, opt, x, z, mask)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss_g = _update(Q, opt, x, z, mask)
    for _ in range(2):
        with torch.no_grad():  # back to the initial weights and a fresh optimiser state
            for p, w in zip(Q.parameters(), w0):
                p.copy_(w)
            for st in opt.state.values():
                for t in st.values():
                    t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e), "loss differs between graph replay and eager"
        for (n, p), e in zip(Q.named_parameters(), p_eager):
            assert torch.equal(p.detach(), e), "%s differs between graph replay and eager" % n
