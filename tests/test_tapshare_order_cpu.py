"""CPU (host-only calls): the K order of the generator's k4 s2 limb weights (gemm.h x3_up2_walk) and the rule for the
tap-shared A staging (gemm.h x3_tapshare_ok), through damc_x3_layer_walk / damc_x3_walk_ktile /
damc_x3_layer_tapshare / damc_x3_layer_sign_block.

For every k4 s2 layer of the five generator topologies at their default widths: the walk visits every (tap, 32-channel
slice) K tile exactly once, groups of four consecutive K tiles share a slice (and, in the input gradient, the taps'
parity class), and every sign block -- which is also the split-K granule -- starts at a multiple of 4 K tiles, so no
workgroup ever starts inside a group."""
import ctypes

import pytest

# (cin, cout, hin) of the k4 s2 p1 layers, diffusion_net._G_TOPOLOGY at the default ngf
TOPOLOGIES = {
    "cifar10": [(1024, 512, 8), (512, 256, 16)],
    "svhn": [(512, 256, 4), (256, 128, 8)],
    "celeba64": [(1024, 512, 4), (512, 256, 8), (256, 128, 16)],
    "celebaHQ": [(2048, 1024, 4), (1024, 512, 8), (512, 512, 16), (512, 256, 32), (256, 128, 64)],
    "mnist": [(1024, 512, 7), (512, 256, 14)],
}
CASES = [(n, i) for n, ls in TOPOLOGIES.items() for i in range(len(ls))]


def _up2(cin, cout, hin):
    from damc import _lib

    d = _lib.Layer()
    d.kind, d.cin, d.cout, d.k, d.stride, d.pad = _lib.LAYER_UP2, cin, cout, 4, 2, 1
    d.hin = d.win = hin
    d.hout = d.wout = 2 * hin
    return d


def _tile(L, input_grad, kt):
    c0, tap = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.damc_x3_walk_ktile(input_grad, kt, ctypes.byref(c0), ctypes.byref(tap)) == 0
    return c0.value, tap.value


@pytest.mark.parametrize("name,idx", CASES)
def test_walk_is_a_bijection_in_groups_of_four(name, idx):
    from damc import _lib

    L = _lib.lib()
    cin, cout, hin = TOPOLOGIES[name][idx]
    d = _up2(cin, cout, hin)
    for input_grad, cg, taps in ((0, cin, 4), (1, cout, 16)):
        assert L.damc_x3_layer_walk(ctypes.byref(d), input_grad) == 1
        nkt = taps * cg // 32
        tiles = [_tile(L, input_grad, kt) for kt in range(nkt)]
        assert sorted(tiles) == sorted((c0, t) for c0 in range(0, cg, 32) for t in range(taps))
        for g0 in range(0, nkt, 4):
            grp = tiles[g0:g0 + 4]
            assert len({c0 for c0, _ in grp}) == 1
            if input_grad:
                # one parity class of (ky, kx); its four taps are the 2 x 2 displacements (ky // 2, kx // 2)
                assert len({((t >> 2) & 1, t & 1) for _, t in grp}) == 1
                assert sorted(((t >> 2) >> 1, (t & 3) >> 1) for _, t in grp) == [(0, 0), (0, 1), (1, 0), (1, 1)]
            else:
                assert [t for _, t in grp] == [0, 1, 2, 3]
        # sign blocks = MFMA accumulation blocks = split-K slices: whole groups
        negk = L.damc_x3_layer_sign_block(ctypes.byref(d), input_grad)
        assert negk in (256, 512, 1024)
        assert (negk // 32) % 4 == 0 and (taps * cg) % negk == 0


@pytest.mark.parametrize("rule", ["256", "512", "1024"])
def test_pinned_sign_blocks_keep_whole_groups(monkeypatch, rule):
    from damc import _lib

    L = _lib.lib()
    monkeypatch.setenv("DAMC_X3_NEGK_RULE", rule)
    for name, idx in CASES:
        d = _up2(*TOPOLOGIES[name][idx])
        for input_grad in (0, 1):
            assert (L.damc_x3_layer_sign_block(ctypes.byref(d), input_grad) // 32) % 4 == 0


def test_tapshare_rule_is_by_grid_alone():
    """Shared staging needs whole images in a 256-row tile: the 4^2, 8^2 and 16^2 grids of the CIFAR-10, SVHN and
    CelebA-64 generators qualify, CelebA-HQ's 32^2 and 64^2 grids and MNIST's 7^2 / 14^2 fall back; layers without limb
    weights report neither the walk nor the staging."""
    from damc import _lib

    L = _lib.lib()
    for name, idx in CASES:
        cin, cout, hin = TOPOLOGIES[name][idx]
        d = _up2(cin, cout, hin)
        want = 1 if hin in (4, 8, 16) else 0
        assert L.damc_x3_layer_tapshare(ctypes.byref(d), 0) == want, (name, idx)
        assert L.damc_x3_layer_tapshare(ctypes.byref(d), 1) == want, (name, idx)
    out = _up2(128, 3, 32)  # a k4 s2 output layer: 3 channels, no limb copies
    assert L.damc_x3_layer_walk(ctypes.byref(out), 0) == 0 and L.damc_x3_layer_walk(ctypes.byref(out), 1) == 0
    assert L.damc_x3_layer_tapshare(ctypes.byref(out), 0) == 0 and L.damc_x3_layer_tapshare(ctypes.byref(out), 1) == 0
    d = _lib.Layer()
    d.kind = _lib.LAYER_SMALLC
    assert L.damc_x3_layer_walk(ctypes.byref(d), 0) == 0 and L.damc_x3_layer_tapshare(ctypes.byref(d), 1) == 0
