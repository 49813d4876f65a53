"""CPU: the host side of the spectral-norm training path (damc.training.specnorm_apply, include/damc.h
damc_specnorm_*): the in-place [A][R][K] view against the hook's own matrix, the gradient formula the kernels implement
against autograd through the stock hooked module, the workspace query, and which _netE route takes an e_sn net."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

import specnorm_util as su


def _hook(m):
    from damc import plans

    return plans._sn_hook(m)


def _layers():
    out = [("linear-%d-%d" % (o, i), nn.Linear(i, o)) for o, i in ((1, 200), (200, 128), (3, 5))]
    for cin, cout, k in ((8, 1, 3), (8, 3, 3), (5, 3, 4), (4, 6, 7), (3, 1, 7), (6, 5, 8), (2, 3, 8), (7, 1, 4)):
        out.append(("convT-%d-%d-k%d" % (cin, cout, k), nn.ConvTranspose2d(cin, cout, k, 1, 0)))
    return out


@pytest.mark.parametrize("name,mod", _layers(), ids=[n for n, _ in _layers()])
def test_view_reproduces_the_hooks_matrix_bitwise(name, mod):
    """specnorm_view's [A][R][K] reading of weight_orig, row = middle index and column = a K + k, is
    SpectralNorm.reshape_weight_to_matrix (dim 0 for Linear, dim 1 for ConvTranspose2d), without the permuted copy."""
    from damc import plans

    torch.manual_seed(3)
    m = nn.utils.spectral_norm(mod)
    h = _hook(m)
    assert h.dim == (1 if isinstance(mod, nn.ConvTranspose2d) else 0)
    w = m.weight_orig.detach()
    a, r, k = plans.specnorm_view(w.shape, h.dim)
    if isinstance(mod, nn.ConvTranspose2d):
        assert (a, r, k) == (mod.in_channels, mod.out_channels, mod.kernel_size[0] ** 2)
    else:
        assert (a, r, k) == (1, mod.out_features, mod.in_features)
    want = h.reshape_weight_to_matrix(w)
    got = su.matrix(w.reshape(a, r, k))  # reshape of a contiguous tensor: a view, the memory order untouched
    assert got.shape == want.shape == (m.weight_u.numel(), m.weight_v.numel())
    assert torch.equal(got, want)
    flat = w.reshape(-1)
    for ai, ri, ki in ((0, 0, 0), (a - 1, r - 1, k - 1), (a // 2, r // 2, k // 2)):
        assert flat[(ai * r + ri) * k + ki] == want[ri, ai * k + ki]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name,mod", _layers()[1:6], ids=[n for n, _ in _layers()[1:6]])
def test_restated_backward_is_autograd_through_the_hook_fp64(name, mod, train):
    """The forward restatement and dL/dW_orig = (G - <G, W_hat> u v^T) / sigma equal the stock hooked module and
    autograd through it in fp64 to 1e-12, in train mode (one power iteration, u and v advanced in place) and in eval
    mode (none: u, v untouched, the sigma term still there)."""
    from damc import plans

    torch.manual_seed(5)
    m = nn.utils.spectral_norm(copy.deepcopy(mod)).double()
    m.train(train)
    h = _hook(m)
    a, r, k = plans.specnorm_view(m.weight_orig.shape, h.dim)
    w0, u0, v0 = m.weight_orig.detach().clone(), m.weight_u.clone(), m.weight_v.clone()
    x = torch.randn(4, mod.in_features, dtype=torch.float64) if isinstance(mod, nn.Linear) else \
        torch.randn(2, mod.in_channels, 3, 3, dtype=torch.float64)
    y = m(x)
    what = m.weight
    g = torch.autograd.grad(y.square().sum(), what, retain_graph=True)[0]  # dL/dW_hat
    (y.square().sum()).backward()
    u, v, sigma, what_ref = su.forward_ref(w0.reshape(a, r, k), u0, v0, 1 if train else 0, h.eps, torch.float64)
    assert torch.equal(m.weight_u, u) and torch.equal(m.weight_v, v)
    if not train:
        assert torch.equal(u, u0) and torch.equal(v, v0)
    assert torch.allclose(what.detach().reshape(a, r, k), what_ref, rtol=1e-12, atol=0)
    dw = su.backward_ref(g.reshape(a, r, k), what_ref, sigma, u, v).reshape(w0.shape)
    err = float((dw - m.weight_orig.grad).norm() / m.weight_orig.grad.norm())
    assert err <= 1e-12, err
    # dropping the sigma term is not the gradient
    assert float((g / sigma - m.weight_orig.grad).norm() / m.weight_orig.grad.norm()) > 1e-3


def _table(cases, ptr=256):
    from damc import _lib

    tab = (_lib.SpecNormLayer * max(len(cases), 1))()
    for t, (a, r, k) in zip(tab, cases):
        t.w_orig = t.u = t.v = t.w_hat = t.sigma = t.u_used = t.v_used = ptr  # host-only size query
        t.a, t.r, t.k, t.eps = a, r, k, 1e-12
    return tab


def test_workspace_query_and_abi_version():
    from damc import _lib

    L = _lib.lib()
    assert L.damc_abi_version() == _lib.ABI_VERSION == 3
    q = L.damc_specnorm_workspace_bytes
    one = q(_table(su.CASES[:1]), 1)
    assert one > 0
    assert q(_table(su.CASES[:8]), 8) > one
    assert q(_table(su.CASES[:3]), 3) == q(_table(su.CASES[:3], ptr=260), 3)  # by the extents, not the alignment
    assert q(_table(su.CASES[:1]), 0) == 0
    assert q(_table(su.CASES[:9]), 9) == 0
    assert q(None, 1) == 0
    for bad in ((0, 3, 5), (1, 0, 5), (1, 3, 0), (1, -2, 5)):
        assert q(_table([su.CASES[0], bad]), 2) == 0
    nul = _table(su.CASES[:2])
    nul[1].w_hat = None
    assert q(nul, 2) == 0
    # argument checks of the calls themselves run on the host
    assert L.damc_specnorm_forward(_table(su.CASES[:1]), 1, 1, None, 0, None) == _lib.DAMC_ERR_ARG
    assert L.damc_specnorm_forward(_table(su.CASES[:1]), 1, -1, 256, one, None) == _lib.DAMC_ERR_ARG
    assert L.damc_specnorm_forward(_table(su.CASES[:1]), 1, 1, 256, one - 16, None) == _lib.DAMC_ERR_WORKSPACE
    assert L.damc_specnorm_backward(_table(su.CASES[:1]), 1, None, 256, one, None) == _lib.DAMC_ERR_ARG
    assert ctypes.sizeof(_lib.SpecNormLayer) == 7 * 8 + 4 * 4 + 0  # damc_specnorm_layer_t, no padding on LP64


def test_ebm_routes_for_spectral_norm_nets():
    """_ebm_layers keeps refusing a net with reparametrised layers; the second route takes _netE(e_sn=True) -- all three
    Linears under nn.utils.spectral_norm -- and nothing else."""
    from damc import training
    from src import diffusion_net as dn

    E = dn._netE(nz=128, e_sn=True)
    assert training._ebm_layers(E) is None
    lay = training._ebm_layers(E, spectral=True)
    assert lay is not None and len(lay[0]) == 3 and lay[1] == pytest.approx(0.2)
    assert training._ebm_layers(dn._netE(nz=128), spectral=True) is None
    assert training._ebm_layers(dn._netE(nz=128, nez=2, e_sn=True), spectral=True) is None
    half = dn._netE(nz=128)
    half.ebm[0] = nn.utils.spectral_norm(half.ebm[0])
    assert training._ebm_layers(half) is None and training._ebm_layers(half, spectral=True) is None
    wn = dn._netE(nz=128)
    for i in (0, 2, 4):
        wn.ebm[i] = nn.utils.weight_norm(wn.ebm[i])
    assert training._ebm_layers(wn, spectral=True) is None


def test_layer_table_eligibility_host_only():
    """_specnorm_spec: host tensors, mixed modes, other dtypes and more than 8 layers are not taken (the stock modules
    then run); a generator with another reparametrisation is handed back before any plan is built."""
    from damc import plans, training
    from src import diffusion_net as dn

    G = dn._netG_cifar10(nz=16, ngf=4, use_spc_norm=True)
    sn = plans.sn_layers([m for m in G.gen if isinstance(m, nn.ConvTranspose2d)])
    assert len(sn) == 4
    assert training._specnorm_spec(sn) is None          # CPU tensors
    assert training._specnorm_spec([]) is None
    assert training._specnorm_spec(sn * 3) is None      # 12 layers
    assert not training._foreign_reparam(G)
    G.gen[0] = nn.utils.weight_norm(nn.ConvTranspose2d(16, 32, 8, 1, 0))
    assert training._foreign_reparam(G)
    assert training.generator_apply(G, torch.zeros(2, 16)) is None
