"""CPU: the case tables of tests/encoder_ops_util.py reach the paths they name.  libdamc.so's host-only size functions
say "supported" / "unsupported" as the tables claim (tests/test_gpu_encoder_ops.py relies on it: a workspace of size 0
would skip the split-K path or turn a parity case into a refusal), and the fp64 reference of every norm case keeps all
its pre-activations clear of the LeakyReLU kink, so the backward tests need no exclusion logic (cap: zero elements)."""
import pytest

import encoder_ops_util as U


def _L():
    from damc import _lib

    return _lib.lib()


@pytest.mark.parametrize("case,split", U.CONV_CASES, ids=[U.case_id(c) for c, _ in U.CONV_CASES])
def test_conv2d_split_k_workspace_as_claimed(case, split):
    B, hin, win, cin, cout, k, s, p = case
    n = int(_L().damc_conv2d_workspace_floats(*case))
    assert (n > 0) == split, (case, n)
    if split:  # S slabs of the (M, cout) output, S >= 2, only on the K-major engine
        ho, wo = U.conv_out_hw(case)
        M = B * ho * wo
        assert cin % 32 == 0 and n % (M * cout) == 0 and n // (M * cout) >= 2


@pytest.mark.parametrize("case", U.X3_CASES, ids=U.case_id)
def test_x3_cases_are_supported(case):
    B, hin, win, cin, cout, k, s, p = case
    L = _L()
    assert int(L.damc_conv2d_x3_bytes(cout, cin, k)) == cout * k * k * cin * 6
    assert int(L.damc_conv2d_x3_workspace_bytes(*case)) > 0


def test_x3_partial_sign_blocks_are_in_the_table():
    nk = int(_L().damc_x3_sign_block())
    Ks = [c[3] * c[5] * c[5] for c in U.X3_CASES]
    assert any(K % nk for K in Ks) and any(K % nk == 0 and K // nk >= 8 for K in Ks)


@pytest.mark.parametrize("case", U.X3_UNSUPPORTED, ids=U.case_id)
def test_x3_unsupported_cases_report_zero(case):
    B, hin, win, cin, cout, k, s, p = case
    L = _L()
    assert int(L.damc_conv2d_x3_bytes(cout, cin, k)) == 0
    assert int(L.damc_conv2d_x3_workspace_bytes(*case)) == 0


@pytest.mark.parametrize("case,dx", U.CONV_BWD_CASES, ids=[U.case_id(c) for c, _ in U.CONV_BWD_CASES])
def test_conv2d_backward_cases_are_supported(case, dx):
    assert int(_L().damc_conv2d_backward_workspace_bytes(*case)) > 0


@pytest.mark.parametrize("case", U.NORM_CASES, ids=U.case_id)
def test_norm_workspaces_follow_the_partition(case):
    B, hw, c = case
    L = _L()
    S = U.in_splits(hw)
    if case in U.NORM_SPLITS:
        assert (S, U.apply_splits(hw)) == U.NORM_SPLITS[case]
    assert int(L.damc_instnorm_workspace_floats(B, hw, c)) == B * c * S * 3 + B * c  # S partials and the pivot
    assert int(L.damc_instnorm_bwd_workspace_floats(B, hw, c)) >= B * c * S * 2 + B * c * 2


@pytest.mark.parametrize("case", U.NORM_CASES, ids=U.case_id)
def test_norm_reference_stays_clear_of_the_kink(case):
    assert U.kink_margin(case) > U.KINK_REL, (case, U.kink_margin(case))


def test_norm_const_channel_reference():
    """The constant-channel variant: variance exactly 0 in that channel, the others clear of the kink."""
    import numpy as np

    case, ch = U.NORM_CONST_CASE, U.NORM_CONST_CHANNEL
    y = U.norm_inputs(case, const_channel=ch)[0].numpy()
    assert np.all(y[:, :, ch] == y[0, 0, ch])
    assert U.kink_margin(case, const_channel=ch) > U.KINK_REL
    r64 = U.norm_refs(case, const_channel=ch)[1]
    beta = U.norm_inputs(case, const_channel=ch)[2].double().numpy()
    want = beta[ch] if beta[ch] > 0 else U.SLOPE * beta[ch]
    assert np.all(r64["h"][:, :, ch] == want)


def test_guards_notice_a_stray_word():
    """The guard helper itself, on host memory: one word in front of or behind a payload, or in a strided gap."""
    import torch

    U.reset_guards()
    try:
        c = U.guarded((3, 7), "cpu")
        ws = U.guarded(10, "cpu")  # 10 bytes: the payload ends inside a word
        assert c.shape == (3, 7) and c.dtype == torch.float32 and ws.shape == (10,) and ws.dtype == torch.uint8
        assert U.is_pattern(c)
        c[:, :5] = 1.0
        ws[:] = 0
        U.assert_guards_intact()
        assert U.is_pattern(c[:, 5:]) and not U.is_pattern(c[:, 4:])
        for buf, lead, words in list(U._GUARDED):
            for at in (lead - 1, lead + words):
                keep = int(buf[at])
                buf[at] = 0
                with pytest.raises(AssertionError):
                    U.assert_guards_intact()
                buf[at] = keep
        U.assert_guards_intact()
    finally:
        U.reset_guards()
