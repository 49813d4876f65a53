"""GPU: spectral-norm nets in the G and E updates on libdamc (include/damc.h damc_specnorm_forward / _backward,
damc.training.specnorm_apply; the reference's use_spc_norm / e_sn flags, diffusion_net.py:8-16, 21-44, 208-210).

Per-op: every case of specnorm_util.CASES with 0, 1 and 2 power iterations in guarded buffers, u, v, sigma, W_hat and
dL/dW_orig under the project's rule (encoder_ops_util.check: |hip - fp64| <= 3 |torch fp32 - fp64| + 1e-6 in rel-L2, both
references PyTorch-CPU on the same fp32 inputs), W_hat bitwise W / sigma_hip, and bitwise repeatability.
Updates: two consecutive G updates (train_gen_recon.py:222-231) and an E update (:233-241) against deep copies of the
stock modules on the CPU in fp32 and fp64 under the same rule, with forward hooks on the stock layers pinning the path.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import encoder_ops_util as eo
import specnorm_util as su
from conftest import rel_l2

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ per-op
def _alloc(case, dev, lead=256):
    """Guarded device buffers of one layer and its table entry's fields."""
    a, r, k = case
    w, u, v, g = su.inputs(case)
    b = dict(w=eo.guarded((a, r, k), dev, lead=lead), u=eo.guarded((r,), dev), v=eo.guarded((a * k,), dev, lead=lead),
             w_hat=eo.guarded((a, r, k), dev, lead=lead), sigma=eo.guarded((1,), dev), u_used=eo.guarded((r,), dev),
             v_used=eo.guarded((a * k,), dev, lead=lead), g=eo.guarded((a, r, k), dev, lead=lead))
    b["w"].copy_(w)
    b["u"].copy_(u)
    b["v"].copy_(v)
    b["g"].copy_(g)
    return b


def _run(cases, npi, dev, lead=256):
    """One grouped forward and backward over `cases`; per layer a dict of CPU arrays."""
    from damc import _lib

    L = _lib.lib()
    eo.reset_guards()
    n = len(cases)
    bufs = [_alloc(c, dev, lead) for c in cases]
    tab = (_lib.SpecNormLayer * n)()
    for t, c, b in zip(tab, cases, bufs):
        t.w_orig, t.u, t.v = b["w"].data_ptr(), b["u"].data_ptr(), b["v"].data_ptr()
        t.w_hat, t.sigma, t.u_used, t.v_used = (b[key].data_ptr() for key in ("w_hat", "sigma", "u_used", "v_used"))
        t.a, t.r, t.k, t.eps = c[0], c[1], c[2], su.EPS
    nb = int(L.damc_specnorm_workspace_bytes(tab, n))
    assert nb > 0
    ws = eo.guarded(nb, dev)
    stream = _lib.stream_ptr(dev)
    _lib.check(L.damc_specnorm_forward(tab, n, npi, _lib.ptr(ws), nb, stream), "damc_specnorm_forward")
    eo.assert_guards_intact()
    fwd = [{key: b[key].cpu().numpy().copy() for key in ("u", "v", "w_hat", "sigma", "u_used", "v_used")} for b in bufs]
    for b, c in zip(bufs, cases):
        assert torch.equal(b["w"].cpu(), su.inputs(c)[0])  # read in place, never written
    garr = (ctypes.c_void_p * n)(*[b["g"].data_ptr() for b in bufs])
    _lib.check(L.damc_specnorm_backward(tab, n, garr, _lib.ptr(ws), nb, stream), "damc_specnorm_backward")
    eo.assert_guards_intact()
    for f, b in zip(fwd, bufs):
        f["dw"] = b["g"].cpu().numpy().copy()
        for key in ("w_hat", "sigma", "u_used", "v_used"):  # the backward only reads them
            assert np.array_equal(f[key], b[key].cpu().numpy())
    return fwd


def _check_layer(tag, case, npi, out):
    a, r, k = case
    w, u0, v0, _ = su.inputs(case)
    r32, r64 = su.refs(case, npi)
    assert np.array_equal(out["u"], out["u_used"]) and np.array_equal(out["v"], out["v_used"])
    if npi == 0:
        assert np.array_equal(out["u"], u0.numpy()) and np.array_equal(out["v"], v0.numpy())
    if r == 1 and npi > 0:
        assert abs(float(out["u"][0])) == 1.0
    # an IEEE divide by the sigma the library wrote, as weight / sigma is
    assert np.array_equal(out["w_hat"], (w / torch.from_numpy(out["sigma"])).numpy())
    eo.check(tag + " u", out["u"], r32["u"], r64["u"])
    eo.check(tag + " v", out["v"], r32["v"], r64["v"], (("lastslab", (slice((a - 1) * k, None),)),))
    eo.check(tag + " sigma", out["sigma"], r32["sigma"], r64["sigma"])
    eo.check(tag + " w_hat", out["w_hat"], r32["w_hat"], r64["w_hat"])
    eo.check(tag + " dw", out["dw"], r32["dw"], r64["dw"],
             (("lastrow", (slice(None), -1)), ("lastslab", (-1,)), ("lastcol", (Ellipsis, -1))))


@pytest.mark.parametrize("npi", [0, 1, 2])
@pytest.mark.parametrize("case", su.CASES, ids=su.case_id)
def test_specnorm_forward_backward_per_layer(gpu_device, case, npi):
    out = _run([case], npi, gpu_device)[0]
    _check_layer("specnorm %s it%d" % (su.case_id(case), npi), case, npi, out)
    again = _run([case], npi, gpu_device)[0]
    for key in out:
        assert np.array_equal(out[key], again[key]), key


@pytest.mark.parametrize("npi", [0, 1])
def test_specnorm_grouped_call_is_bitwise_the_single_layer_calls(gpu_device, npi):
    """Eight layers in one table: every launch covers all of them, and a layer's results do not depend on its
    neighbours (the same tiles, the same summation order)."""
    cases = su.CASES[:8]
    grouped = _run(cases, npi, gpu_device)
    for c, g in zip(cases, grouped):
        single = _run([c], npi, gpu_device)[0]
        for key in g:
            assert np.array_equal(g[key], single[key]), (c, key)


@pytest.mark.parametrize("case", [(33, 7, 16), (1, 200, 128)], ids=su.case_id)
def test_specnorm_misaligned_pointers_take_the_scalar_path(gpu_device, case):
    """Weights, v and the gradient one float off 16-byte alignment with K % 4 == 0: scalar accesses, same rule."""
    out = _run([case], 1, gpu_device, lead=260)[0]
    _check_layer("specnorm misaligned %s" % su.case_id(case), case, 1, out)


def test_specnorm_backward_skips_null_gradients(gpu_device):
    from damc import _lib

    cases = [(4, 3, 9), (1, 200, 128)]
    full = _run(cases, 1, gpu_device)
    L = _lib.lib()
    eo.reset_guards()
    bufs = [_alloc(c, gpu_device) for c in cases]
    tab = (_lib.SpecNormLayer * 2)()
    for t, c, b in zip(tab, cases, bufs):
        t.w_orig, t.u, t.v = b["w"].data_ptr(), b["u"].data_ptr(), b["v"].data_ptr()
        t.w_hat, t.sigma, t.u_used, t.v_used = (b[key].data_ptr() for key in ("w_hat", "sigma", "u_used", "v_used"))
        t.a, t.r, t.k, t.eps = c[0], c[1], c[2], su.EPS
    nb = int(L.damc_specnorm_workspace_bytes(tab, 2))
    ws = eo.guarded(nb, gpu_device)
    stream = _lib.stream_ptr(gpu_device)
    _lib.check(L.damc_specnorm_forward(tab, 2, 1, _lib.ptr(ws), nb, stream), "forward")
    garr = (ctypes.c_void_p * 2)(None, bufs[1]["g"].data_ptr())
    _lib.check(L.damc_specnorm_backward(tab, 2, garr, _lib.ptr(ws), nb, stream), "backward")
    eo.assert_guards_intact()
    assert torch.equal(bufs[0]["g"].cpu(), su.inputs(cases[0])[3])
    assert np.array_equal(bufs[1]["g"].cpu().numpy(), full[1]["dw"])


# ------------------------------------------------------------------------------------------------------ updates
def _sn_buffers(net):
    return [(n, t) for n, t in net.named_buffers() if n.endswith("weight_u") or n.endswith("weight_v")]


def _count_calls(net, kind):
    calls = []
    handles = [m.register_forward_hook(lambda mod, i, o: calls.append(type(mod).__name__))
               for m in net.modules() if isinstance(m, kind)]
    return calls, handles


def _g_update(G, z0, x):
    for p in G.parameters():
        p.grad = None
    z = z0.clone().requires_grad_(True)
    loss = torch.sum((G(z) - x) ** 2, dim=[1, 2, 3]).mean()
    loss.backward()
    out = {"loss": loss.detach().reshape(1), "dz": z.grad}
    for n, p in G.named_parameters():
        out["grad " + n] = p.grad
    for n, t in _sn_buffers(G):
        out[n] = t.detach().clone()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


G_NETS = {"cifar10": ("_netG_cifar10", dict(nz=128, ngf=16, nc=3), 32),
          "svhn": ("_netG_svhn", dict(nz=100, ngf=16, nc=3), 32),
          "mnist": ("_netG_mnist", dict(nz=8, ngf=16, nc=1), 28)}  # a one-row output layer


def _g_net(name, B, seed):
    from damc import synth
    from src import diffusion_net as dn

    ctor, kw, H = G_NETS[name]
    G = synth.load_into(getattr(dn, ctor)(use_spc_norm=True, **kw), seed)
    z0 = torch.from_numpy(synth.normal_f32(41 + seed, 0, (B, kw["nz"])))
    x = torch.from_numpy(synth.uniform_f32(41 + seed, 1, (B, kw["nc"], H, H)))
    return G, z0, x


@pytest.mark.parametrize("B", [8, 5])
@pytest.mark.parametrize("name", sorted(G_NETS))
def test_g_update_of_a_spectral_norm_generator(gpu_device, name, B):
    """Two consecutive G updates in train mode (no optimiser step in between: what carries over is the in-place u, v):
    loss, every weight_orig / bias gradient, dz and u, v against deep copies of the stock modules on the CPU in fp64,
    with the fp32 CPU copy as the yardstick.  Path pin: no stock ConvTranspose2d runs and weight_orig.grad is set."""
    G, z0, x = _g_net(name, B, 4)
    G.train()
    stock = {dt: copy.deepcopy(G).to(dt) for dt in (torch.float32, torch.float64)}
    Gd = G.to(gpu_device)
    ptrs = [t.data_ptr() for _, t in _sn_buffers(Gd)]
    calls, handles = _count_calls(Gd, torch.nn.ConvTranspose2d)
    zd, xd = z0.to(gpu_device), x.to(gpu_device)
    for it in range(2):
        hip = _g_update(Gd, zd, xd)
        torch.cuda.synchronize()
        r32 = _g_update(stock[torch.float32], z0, x)
        r64 = _g_update(stock[torch.float64], z0.double(), x.double())
        assert sorted(hip) == sorted(r64)
        assert any(k.endswith("weight_orig") for k in hip)
        for k in sorted(hip):
            eo.check("G %s B=%d update %d %s" % (name, B, it, k), hip[k], r32[k], r64[k])
    for h in handles:
        h.remove()
    assert calls == []  # the stock layers never ran
    assert [t.data_ptr() for _, t in _sn_buffers(Gd)] == ptrs
    assert all(p.grad is not None for n, p in Gd.named_parameters() if n.endswith("weight_orig"))


def test_two_g_forwards_before_one_backward(gpu_device):
    """x1, x2 = G(z1), G(z2) in train mode, then one backward: the second forward has advanced u, v and packed other
    weights into the plan's buffers, and each forward's backward still runs on its own weights, sigma, u, v."""
    G, z0, x = _g_net("svhn", 8, 7)
    G.train()

    def run(net, z, xx):
        for p in net.parameters():
            p.grad = None
        z1 = z.clone().requires_grad_(True)
        z2 = (0.5 * z).flip(0).clone().requires_grad_(True)
        x1, x2 = net(z1), net(z2)
        (torch.sum((x1 - xx) ** 2) + 2.0 * torch.sum((x2 - xx) ** 2)).backward()
        out = {"dz1": z1.grad, "dz2": z2.grad}
        for n, p in net.named_parameters():
            out["grad " + n] = p.grad
        return {k: v.detach().cpu().numpy() for k, v in out.items()}

    stock = {dt: copy.deepcopy(G).to(dt) for dt in (torch.float32, torch.float64)}
    Gd = G.to(gpu_device)
    calls, handles = _count_calls(Gd, torch.nn.ConvTranspose2d)
    hip = run(Gd, z0.to(gpu_device), x.to(gpu_device))
    for h in handles:
        h.remove()
    assert calls == []
    r32 = run(stock[torch.float32], z0, x)
    r64 = run(stock[torch.float64], z0.double(), x.double())
    for k in sorted(hip):
        eo.check("G two forwards %s" % k, hip[k], r32[k], r64[k])


def test_g_update_in_eval_mode_keeps_u_v_and_the_sigma_term(gpu_device):
    """Eval mode with grad: no power iteration (u, v bitwise unchanged), and the gradient still goes through sigma --
    G / sigma alone is far from the fp64 reference."""
    G, z0, x = _g_net("cifar10", 8, 6)
    with torch.no_grad():
        for _ in range(3):  # train-mode forwards first: with the initial random u, v sigma = u^T W v is near zero
            G.train()(z0)
    G.eval()
    stock ={dt: copy.deepcopy(G).to(dt) for dt in (torch.float32, torch.float64)}
    Gd = G.to(gpu_device)
    before = [t.clone() for _, t in _sn_buffers(Gd)]
    calls, handles = _count_calls(Gd, torch.nn.ConvTranspose2d)
    hip = _g_update(Gd, z0.to(gpu_device), x.to(gpu_device))
    for h in handles:
        h.remove()
    assert calls == []
    for a, (_, b) in zip(before, _sn_buffers(Gd)):
        assert torch.equal(a, b)
    r32 = _g_update(stock[torch.float32], z0, x)
    r64 = _g_update(stock[torch.float64], z0.double(), x.double())
    for k in sorted(hip):
        eo.check("G eval %s" % k, hip[k], r32[k], r64[k])
    assert np.linalg.norm(r64["grad gen.0.weight_orig"]) > 1e-3  # a live gradient, not a saturated tanh
    # without the sigma term the weight gradient would be dL/dW_hat / sigma: the fp64 modules say how far that is
    m = stock[torch.float64].gen[0]
    loss = torch.sum((stock[torch.float64](z0.double()) - x.double()) ** 2, dim=[1, 2, 3]).mean()
    what = m.weight  # set by the hook in the forward above
    gw = torch.autograd.grad(loss, what)[0]
    sigma = (m.weight_orig / what).flatten()[0]
    assert rel_l2((gw / sigma).detach().numpy(), r64["grad gen.0.weight_orig"]) > 1e-3


def _e_update(E, a, b):
    for p in E.parameters():
        p.grad = None
    e_pos, e_neg = E(a), E(b)
    (e_pos.mean() - e_neg.mean()).backward()
    out = {"e_pos": e_pos, "e_neg": e_neg}
    for n, p in E.named_parameters():
        out["grad " + n] = p.grad
    for n, t in _sn_buffers(E):
        out[n] = t.detach().clone()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("nz", [128, 100])
def test_e_update_of_a_spectral_norm_ebm(gpu_device, nz):
    """e_pos, e_neg = E(a), E(b) at B = 8 / 16, then one backward: each forward keeps its own sigma, u, v (the module's
    u, v advance twice), every gradient within the rule against fp64 stock modules run the same way; no stock Linear
    runs."""
    from damc import synth
    from src import diffusion_net as dn

    E = synth.load_into(dn._netE(nz=nz, e_sn=True), 5).train()
    a = torch.from_numpy(synth.normal_f32(83, 0, (8, nz)))
    b = torch.from_numpy(synth.normal_f32(83, 1, (16, nz)))
    stock = {dt: copy.deepcopy(E).to(dt) for dt in (torch.float32, torch.float64)}
    once = copy.deepcopy(E)
    with torch.no_grad():
        once(a)  # one forward's worth of power iteration
    Ed = E.to(gpu_device)
    ptrs = [t.data_ptr() for _, t in _sn_buffers(Ed)]
    calls, handles = _count_calls(Ed, torch.nn.Linear)
    hip = _e_update(Ed, a.to(gpu_device), b.to(gpu_device))
    for h in handles:
        h.remove()
    assert calls == []
    assert [t.data_ptr() for _, t in _sn_buffers(Ed)] == ptrs
    r32 = _e_update(stock[torch.float32], a, b)
    r64 = _e_update(stock[torch.float64], a.double(), b.double())
    assert sorted(hip) == sorted(r64) and any(k.endswith("weight_orig") for k in hip)
    for k in sorted(hip):
        eo.check("E nz=%d %s" % (nz, k), hip[k], r32[k], r64[k])
    for (n, t), (_, t1) in zip(_sn_buffers(Ed), _sn_buffers(once)):
        if n.startswith("ebm.4."):  # the one-row layer: u = +-1 and v = +-w / |w| from the first iteration on
            continue
        assert not np.allclose(t.cpu().numpy(), t1.numpy(), rtol=0, atol=1e-6), n  # two advances, not one


def test_stock_pytorch_switches_spectral_norm_nets_back(gpu_device):
    from damc import synth, training
    from src import diffusion_net as dn

    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=16, nc=3, use_spc_norm=True), 4).to(gpu_device).train()
    E = synth.load_into(dn._netE(nz=128, e_sn=True), 5).to(gpu_device).train()
    z = torch.from_numpy(synth.normal_f32(85, 0, (8, 128))).to(gpu_device)
    gcalls, gh = _count_calls(G, torch.nn.ConvTranspose2d)
    ecalls, eh = _count_calls(E, torch.nn.Linear)
    with training.stock_pytorch():
        G(z).sum().backward()
        E(z).sum().backward()
    assert len(gcalls) == 4 and len(ecalls) == 3
    assert G.gen[0].weight_orig.grad is not None and E.ebm[0].weight_orig.grad is not None
    G(z).sum().backward()
    E(z).sum().backward()
    assert len(gcalls) == 4 and len(ecalls) == 3  # back on libdamc
    for h in gh + eh:
        h.remove()


def test_chains_after_an_update_of_spectral_norm_nets(gpu_device):
    """A 2-step eval-mode posterior chain on G, E after a G and an E update on libdamc still matches the oracle on the
    weights the layers' own hooks compute (the tolerance of test_spectral_norm_nets_in_eval_mode)."""
    from damc import langevin as lv
    from damc import synth, training
    from oracle import damc_oracle as orc
    from src import diffusion_net as dn

    G = synth.load_into(dn._netG_cifar10(nz=128, ngf=16, nc=3, use_spc_norm=True), 4).to(gpu_device).train()
    E = synth.load_into(dn._netE(nz=128, e_sn=True), 5).to(gpu_device).train()
    z0 = torch.from_numpy(synth.normal_f32(91, 0, (8, 128))).to(gpu_device)
    x = torch.from_numpy(synth.uniform_f32(91, 1, (8, 3, 32, 32))).to(gpu_device)
    _g_update(G, z0, x)
    _e_update(E, z0, torch.cat([z0, z0]))
    G.eval()
    E.eval()
    z = z0.clone()
    lv.posterior_langevin(z, x, G, E, 2, 0.3, 0.1, False)
    with training.stock_pytorch(), torch.no_grad():
        G(z0)  # the hooks set every layer's weight (eval: no power iteration)
        E(z0)
    ref = orc.posterior_langevin(orc.generator_layers(G), orc.ebm_params(E), z0.cpu(), x.cpu(), 2, 0.3, 0.1)
    assert rel_l2(z.cpu().numpy(), ref.numpy()) < 2e-4
