"""CPU: the host-side shape logic of the toy amortizer's training calls -- damc_mlp_train_* (the fused MLP's forward
keeping activations, and its backward) and damc_denoiser_train_* at an even nz that is no multiple of 4.  No device
work: every pointer in a descriptor is a placeholder that the size functions never dereference."""
import ctypes

import pytest

from test_toyq_cpu import _toy_desc

ENCODER = ([2, 128, 128, 128, 128], "relu")      # _netQ_U_toy.encoder (toy_example/src/diffusion_net.py:166-174)
PRIOR_EMB = ([2, 128, 128], "lrelu")             # _netQ_U_toy.prior_emb (:180-184), LeakyReLU's default slope


def _mlp_desc(widths, act="relu", slope=0.01):
    """damc_mlp_t of nn.Linear widths with `act` after every layer but the last, placeholder pointers."""
    from damc import _lib

    d = _lib.Mlp()
    d.n_layers = len(widths) - 1
    for i in range(min(d.n_layers, _lib.MLP_MAX_LAYERS)):
        e = d.layers[i]
        e.din, e.dout, e.w, e.bias = widths[i], widths[i + 1], 256, 256
        if i + 1 < d.n_layers:
            e.act, e.slope = (_lib.ACT_RELU, 0.0) if act == "relu" else (_lib.ACT_LRELU, slope)
    return d


def _sizes(d, B):
    from damc import _lib

    L = _lib.lib()
    return (int(L.damc_mlp_train_saved_floats(ctypes.byref(d), B)),
            int(L.damc_mlp_train_workspace_bytes(ctypes.byref(d), B)))


def test_mlp_train_symbols_exist():
    from damc import _lib

    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("damc_mlp_train_saved_floats", "damc_mlp_train_workspace_bytes", "damc_mlp_train_forward",
                 "damc_mlp_train_backward"):
        assert hasattr(so, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.lib().damc_abi_version() == 3


@pytest.mark.parametrize("B", [1, 21, 500])
@pytest.mark.parametrize("widths,act", [ENCODER, PRIOR_EMB])
def test_mlp_train_sizes_of_the_toy_modules(widths, act, B):
    saved, ws = _sizes(_mlp_desc(widths, act), B)
    assert saved > 0 and ws > 0
    # every hidden layer's (B, dout) block, in `saved` and in the backward's dY scratch
    hidden = B * sum(widths[1:-1])
    assert saved >= hidden and ws >= 4 * hidden


def test_mlp_train_sizes_refuse_bad_descriptors():
    from damc import _lib

    assert _sizes(_mlp_desc([2, 257, 128]), 21) == (0, 0)               # a width over 256
    assert _sizes(_mlp_desc([2, 128, 128], "lrelu", slope=-0.1), 21) == (0, 0)  # act' is read from the sign of y
    d = _mlp_desc([2, 128, 128, 128])
    d.layers[1].din = 96                                                 # does not chain
    assert _sizes(d, 21) == (0, 0)
    assert _sizes(_mlp_desc([2] + [8] * 9), 21) == (0, 0)               # 9 layers
    assert _sizes(_mlp_desc(*ENCODER), 0) == (0, 0)
    # the descriptors next to them are taken
    assert all(_sizes(_mlp_desc([2, 256, 128]), 21))
    assert all(_sizes(_mlp_desc([2, 128, 128], "lrelu", slope=0.0), 21))
    assert all(_sizes(_mlp_desc([2] + [8] * 8), 21))


def test_toy_denoiser_trains_on_the_library():
    """The training workspace takes an even nz that is no multiple of 4 (out2 padded to the next multiple inside it),
    nz = 128 keeps a stable nonzero size, and the drop-in's predicate sends the toy's denoiser there."""
    import torch

    from damc import _lib, training
    from toyq_util import build_toy_case

    L = _lib.lib()
    ws = lambda d, B=21: int(L.damc_denoiser_train_workspace_bytes(ctypes.byref(d), B))  # noqa: E731
    assert ws(_toy_desc(2)) > 0
    assert ws(_toy_desc(6)) > 0
    assert ws(_toy_desc(3)) == 0  # an odd nz has no Fourier embedding
    n128 = ws(_toy_desc(128))
    assert n128 > 0
    assert ws(_toy_desc(128)) == n128
    Q = build_toy_case("q_toy")["Q"]
    assert Q.p.nz == 2
    assert training.denoiser_train_supported(Q.p)
    # on the host there is nothing to run on: the caller keeps its stock layers
    assert training.mlp_apply(Q.encoder, torch.zeros(3, 2)) is None
