"""GPU: the amortizer's per-op entry points of include/damc.h called directly, at the smallest shapes that reach each
launcher path (tests/encoder_ops_util.py holds the tables and says what each case reaches): damc_gemm,
damc_conv2d_nhwc (+ damc_pack_conv2d, damc_conv2d_workspace_floats), damc_conv2d_x3_nhwc (+ damc_pack_conv2d_x3),
damc_instnorm_lrelu_nhwc / _train_nhwc / _backward_nhwc, damc_conv2d_backward_nhwc and damc_nchw_to_nhwc
(Encoder_*, workspace/src/diffusion_net.py:227-413).

Rule: |hip - fp64| <= 3 |torch fp32 - fp64| + 1e-6 in rel-L2 against PyTorch-CPU evaluations of the same operation on
the same fp32 inputs, for the whole output and for its last row / column / pixel row / channel / pixel, small slices
floored at 1e-3 x the output's RMS (encoder_ops_util.check).  Every output and workspace sits in a guarded buffer
(a NaN pattern in front, behind and in every strided gap; workspaces at exactly the size their size function reports)
and the guards are compared after every library call; input padding (lda / ldb gaps) is NaN, so a read of it shows.
Run with -s to see the per-case distances (profiles/r13/encoder_ops_parity.txt is one such run).
"""
import numpy as np
import pytest
import torch

import encoder_ops_util as U
from encoder_ops_util import assert_guards_intact, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_guards():
    U.reset_guards()
    yield
    U.reset_guards()


def _api(gpu_device):
    from damc import _lib

    return _lib, _lib.lib(), _lib.stream_ptr(gpu_device)


def _np(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------- damc_gemm
def _padded(t, ld, offset, device):
    """t (rows, cols) on the device with leading dimension ld, NaN in the gaps, `offset` floats past an aligned base."""
    rows, cols = t.shape
    flat = torch.full((offset + rows * ld,), float("nan"), device=device)
    v = flat[offset:].view(rows, ld)
    v[:, :cols] = t.to(device)
    assert v.data_ptr() % 16 == (4 * offset) % 16
    return v


def _gemm(gpu_device, M, N, K, act, with_bias=True, lda=None, ldb=None, ldc=None, off_a=0, off_b=0, off_c=0):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    a, b, bias = U.gemm_inputs(M, N, K)
    lda, ldb, ldc = lda or K, ldb or N, ldc or N
    ad, bd = _padded(a, lda, off_a, gpu_device), _padded(b, ldb, off_b, gpu_device)
    biasd = bias.to(gpu_device) if with_bias else None
    c = guarded((M, ldc), gpu_device, lead=256 + 4 * off_c)
    assert c.data_ptr() % 256 == 4 * off_c
    _lib.check(L.damc_gemm(ptr(ad), lda, ptr(bd), ldb, ptr(biasd), ptr(c), ldc, M, N, K, act, U.SLOPE, stream), "gemm")
    assert_guards_intact()
    if ldc > N:
        assert U.is_pattern(c[:, N:]), "the ldc gap was written"
    r32, r64 = U.gemm_refs(M, N, K, act, with_bias)
    name = "gemm %s act%d%s" % (U.case_id((M, N, K)), act, "" if with_bias else " nobias")
    if (lda, ldb, ldc) != (K, N, N):
        name += " ld(%d,%d,%d)" % (lda, ldb, ldc)
    if off_a or off_b or off_c:
        name += " off(%d,%d,%d)" % (off_a, off_b, off_c)
    U.check(name, _np(c[:, :N]), r32, r64, U.GEMM_SLICES)


@pytest.mark.parametrize("M,N,K", U.GEMM_CASES, ids=[U.case_id(c) for c in U.GEMM_CASES])
def test_gemm_matches_fp64(gpu_device, M, N, K):
    _gemm(gpu_device, M, N, K, U.ACT_NONE)
    _gemm(gpu_device, M, N, K, U.ACT_NONE, with_bias=False)


@pytest.mark.parametrize("act", [U.ACT_NONE, U.ACT_LRELU, U.ACT_TANH, U.ACT_SILU, U.ACT_RELU])
def test_gemm_activations(gpu_device, act):
    _gemm(gpu_device, *U.GEMM_ACT_CASE, act)


def test_gemm_strided_operands_keep_the_gaps(gpu_device):
    M, N, K = U.GEMM_STRIDED
    _gemm(gpu_device, M, N, K, U.ACT_NONE, lda=K + 4, ldb=N + 4, ldc=N + 3)


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_gemm_misaligned_operand(gpu_device, which):
    M, N, K = U.GEMM_MISALIGNED
    _gemm(gpu_device, M, N, K, U.ACT_NONE, **{"off_" + which: 1})


def test_gemm_refuses_bad_arguments(gpu_device):
    """An unknown activation, a NULL operand, a leading dimension below the row length: DAMC_ERR_ARG, no store."""
    _lib, L, stream = _api(gpu_device)
    a, b, _ = (t.to(gpu_device) for t in U.gemm_inputs(3, 5, 2))
    c = guarded((3, 5), gpu_device)
    pa, pb, pc = _lib.ptr(a), _lib.ptr(b), _lib.ptr(c)
    M, N, K = 3, 5, 2
    for args in [(pa, K, pb, N, None, pc, N, M, N, K, 5, 0.0), (pa, K, pb, N, None, pc, N, M, N, K, -1, 0.0),
                 (None, K, pb, N, None, pc, N, M, N, K, 0, 0.0), (pa, K, None, N, None, pc, N, M, N, K, 0, 0.0),
                 (pa, K, pb, N, None, None, N, M, N, K, 0, 0.0), (pa, K - 1, pb, N, None, pc, N, M, N, K, 0, 0.0),
                 (pa, K, pb, N - 1, None, pc, N, M, N, K, 0, 0.0), (pa, K, pb, N, None, pc, N - 1, M, N, K, 0, 0.0)]:
        assert L.damc_gemm(*args, stream) == _lib.DAMC_ERR_ARG, args[1:]
    assert_guards_intact()
    assert U.is_pattern(c)


# ------------------------------------------------------------------------------------------------ damc_conv2d_nhwc
def _pack_conv(gpu_device, case):
    _lib, L, stream = _api(gpu_device)
    B, hin, win, cin, cout, k, s, p = case
    w = U.conv_inputs(case)[1].to(gpu_device)
    wp = guarded((cout * cin * k * k,), gpu_device)
    _lib.check(L.damc_pack_conv2d(_lib.ptr(w), cout, cin, k, _lib.ptr(wp), stream), "pack conv2d")
    assert_guards_intact()
    return wp


@pytest.mark.parametrize("case,split", U.CONV_CASES, ids=[U.case_id(c) for c, _ in U.CONV_CASES])
def test_conv2d_matches_fp64(gpu_device, case, split):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, hin, win, cin, cout, k, s, p = case
    ho, wo = U.conv_out_hw(case)
    x, w, bias, _ = U.conv_inputs(case)
    xd, bd = U.nhwc(x).to(gpu_device), bias.to(gpu_device)
    wp = _pack_conv(gpu_device, case)
    r32, r64 = U.conv_refs(case)
    nws = int(L.damc_conv2d_workspace_floats(*case))
    assert (nws > 0) == split
    runs = [("unsplit", None, 0)]
    if nws:
        runs.append(("splitk", guarded((nws,), gpu_device), nws))
    for label, ws, n in runs:
        y = guarded((B, ho, wo, cout), gpu_device)
        _lib.check(L.damc_conv2d_nhwc(ptr(xd), B, hin, win, cin, ptr(wp), ptr(bd), cout, k, s, p, ptr(y), ptr(ws), n,
                                      stream), "conv2d")
        assert_guards_intact()
        U.check("conv2d %s %s" % (U.case_id(case), label), _np(y), r32, r64, U.CONV_SLICES)
    # bias = NULL
    y = guarded((B, ho, wo, cout), gpu_device)
    _lib.check(L.damc_conv2d_nhwc(ptr(xd), B, hin, win, cin, ptr(wp), None, cout, k, s, p, ptr(y), None, 0, stream),
               "conv2d")
    assert_guards_intact()
    U.check("conv2d %s nobias" % U.case_id(case), _np(y), *U.conv_refs(case, False), U.CONV_SLICES)


def test_conv2d_refuses_more_taps_than_the_k_major_engine_takes(gpu_device):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    case = U.CONV_TOO_MANY_TAPS
    B, hin, win, cin, cout, k, s, p = case
    ho, wo = U.conv_out_hw(case)
    x, w, bias, _ = U.conv_inputs(case)
    xd, bd = U.nhwc(x).to(gpu_device), bias.to(gpu_device)
    wp = _pack_conv(gpu_device, case)
    y = guarded((B, ho, wo, cout), gpu_device)
    rc = L.damc_conv2d_nhwc(ptr(xd), B, hin, win, cin, ptr(wp), ptr(bd), cout, k, s, p, ptr(y), None, 0, stream)
    assert rc != 0
    assert_guards_intact()
    assert U.is_pattern(y), "a refused call wrote its output"


# --------------------------------------------------------------------------------------------- damc_conv2d_x3_nhwc
def _conv_x3(gpu_device, case, xd, bd, w3):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, hin, win, cin, cout, k, s, p = case
    ho, wo = U.conv_out_hw(case)
    nb = int(L.damc_conv2d_x3_workspace_bytes(*case))
    assert nb > 0
    ws = guarded(nb, gpu_device)
    y = guarded((B, ho, wo, cout), gpu_device)
    _lib.check(L.damc_conv2d_x3_nhwc(ptr(xd), B, hin, win, cin, ptr(w3), ptr(bd), cout, k, s, p, ptr(y), ptr(ws), nb,
                                     stream), "conv2d_x3")
    assert_guards_intact()
    return y


@pytest.mark.parametrize("case", U.X3_CASES, ids=U.case_id)
def test_conv2d_x3_matches_fp64(gpu_device, monkeypatch, case):
    _lib, L, stream = _api(gpu_device)
    B, hin, win, cin, cout, k, s, p = case
    x, w, bias, _ = U.conv_inputs(case)
    xd, wd, bd = U.nhwc(x).to(gpu_device), w.to(gpu_device), bias.to(gpu_device)
    nw = int(L.damc_conv2d_x3_bytes(cout, cin, k))
    assert nw > 0
    w3 = guarded(nw, gpu_device)
    _lib.check(L.damc_pack_conv2d_x3(_lib.ptr(wd), cout, cin, k, _lib.ptr(w3), stream), "pack x3")
    assert_guards_intact()
    monkeypatch.delenv("DAMC_X3_KSPLIT", raising=False)
    y = _conv_x3(gpu_device, case, xd, bd, w3)
    r32, r64 = U.conv_refs(case)
    U.check("conv2d_x3 %s" % U.case_id(case), _np(y), r32, r64, U.CONV_SLICES)
    # the sign-block split-K sums its slabs in the unsplit launch's order: bitwise the same output (gemm_x3.hip x3_ksplit)
    monkeypatch.setenv("DAMC_X3_KSPLIT", "0")
    y0 = _conv_x3(gpu_device, case, xd, bd, w3)
    assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), "DAMC_X3_KSPLIT=0 changes the bits"
    # bias = NULL
    monkeypatch.delenv("DAMC_X3_KSPLIT", raising=False)
    yn = _conv_x3(gpu_device, case, xd, None, w3)
    U.check("conv2d_x3 %s nobias" % U.case_id(case), _np(yn), *U.conv_refs(case, False), U.CONV_SLICES)


@pytest.mark.parametrize("case", U.X3_UNSUPPORTED, ids=U.case_id)
def test_conv2d_x3_refuses_what_its_size_functions_refuse(gpu_device, case):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, hin, win, cin, cout, k, s, p = case
    ho, wo = U.conv_out_hw(case)
    assert int(L.damc_conv2d_x3_bytes(cout, cin, k)) == 0 and int(L.damc_conv2d_x3_workspace_bytes(*case)) == 0
    x, w, bias, _ = U.conv_inputs(case)
    xd, wd, bd = U.nhwc(x).to(gpu_device), w.to(gpu_device), bias.to(gpu_device)
    w3 = guarded(cout * k * k * cin * 6, gpu_device)
    ws = guarded(1 << 16, gpu_device)
    y = guarded((B, ho, wo, cout), gpu_device)
    assert L.damc_pack_conv2d_x3(ptr(wd), cout, cin, k, ptr(w3), stream) == _lib.DAMC_ERR_ARG
    assert L.damc_conv2d_x3_nhwc(ptr(xd), B, hin, win, cin, ptr(w3), ptr(bd), cout, k, s, p, ptr(y), ptr(ws), 1 << 16,
                                 stream) == _lib.DAMC_ERR_ARG
    assert_guards_intact()
    assert U.is_pattern(y) and U.is_pattern(w3.view(torch.float32))


# ---------------------------------------------------------------------------------------------- InstanceNorm + LReLU
STAT_SLICES = (("mean", (Ellipsis, 0)), ("rstd", (Ellipsis, 1)))
# The per-channel vectors (dgamma, dbeta, db: at most 300 elements) are checked whole.  Each element is one long
# cancelling sum, so a one-element slice would compare two single rounding-error draws: over the eight channels of
# dgamma at (2, 63, 8) torch's own fp32 error spans 1.4e-8 .. 6.4e-6, a factor of 450, by luck alone.  A wrong last
# channel moves the whole vector's rel-L2 by about 1 / sqrt(c), five orders above the bound.


def _norm_inference(gpu_device, case, y, gamma, beta):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, hw, c = case
    yb = guarded((B, hw, c), gpu_device)
    yb.copy_(y.to(gpu_device))
    ws = guarded((int(L.damc_instnorm_workspace_floats(B, hw, c)),), gpu_device)
    gd, bd = gamma.to(gpu_device), beta.to(gpu_device)
    _lib.check(L.damc_instnorm_lrelu_nhwc(ptr(yb), B, hw, c, ptr(gd), ptr(bd), U.EPS, U.SLOPE, ptr(ws), stream),
               "instnorm")
    assert_guards_intact()
    return yb


def _norm_train(gpu_device, case, y, gamma, beta):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, hw, c = case
    yd, gd, bd = y.to(gpu_device), gamma.to(gpu_device), beta.to(gpu_device)
    h = guarded((B, hw, c), gpu_device)
    stats = guarded((B, c, 2), gpu_device)
    ws = guarded((int(L.damc_instnorm_workspace_floats(B, hw, c)),), gpu_device)
    _lib.check(L.damc_instnorm_lrelu_train_nhwc(ptr(yd), B, hw, c, ptr(gd), ptr(bd), U.EPS, U.SLOPE, ptr(h), ptr(stats),
                                                ptr(ws), stream), "instnorm train")
    assert_guards_intact()
    return h, stats


def _norm_backward(gpu_device, case, y, gamma, beta, dh, stats, want_dgamma=True, want_dbeta=True):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, hw, c = case
    yd, gd, bd, dhd = (t.to(gpu_device) for t in (y, gamma, beta, dh))
    dy = guarded((B, hw, c), gpu_device)
    dgamma = guarded((c,), gpu_device)
    dbeta = guarded((c,), gpu_device)
    ws = guarded((int(L.damc_instnorm_bwd_workspace_floats(B, hw, c)),), gpu_device)
    _lib.check(L.damc_instnorm_lrelu_backward_nhwc(ptr(yd), ptr(stats), ptr(dhd), B, hw, c, ptr(gd), ptr(bd), U.SLOPE,
                                                   ptr(dy), ptr(dgamma) if want_dgamma else None,
                                                   ptr(dbeta) if want_dbeta else None, ptr(ws), stream),
               "instnorm backward")
    assert_guards_intact()
    return dy, dgamma, dbeta


@pytest.mark.parametrize("case", U.NORM_CASES, ids=U.case_id)
def test_instnorm_calls_match_fp64(gpu_device, case):
    y, gamma, beta, dh = U.norm_inputs(case)
    r32, r64 = U.norm_refs(case)
    name = "instnorm %s " % U.case_id(case)
    out = _norm_inference(gpu_device, case, y, gamma, beta)
    U.check(name + "inference", _np(out), r32["h"], r64["h"], U.NORM_SLICES)
    h, stats = _norm_train(gpu_device, case, y, gamma, beta)
    U.check(name + "train h", _np(h), r32["h"], r64["h"], U.NORM_SLICES)
    U.check(name + "train stats", _np(stats), r32["stats"], r64["stats"], STAT_SLICES)
    assert torch.equal(out.view(torch.int32), h.view(torch.int32)), "the two apply kernels share one operation order"
    dy, dgamma, dbeta = _norm_backward(gpu_device, case, y, gamma, beta, dh, stats)
    U.check(name + "backward dy", _np(dy), r32["dy"], r64["dy"], U.NORM_SLICES)
    U.check(name + "backward dgamma", _np(dgamma), r32["dgamma"], r64["dgamma"])
    U.check(name + "backward dbeta", _np(dbeta), r32["dbeta"], r64["dbeta"])


@pytest.mark.parametrize("skip", ["dgamma", "dbeta"])
def test_instnorm_backward_with_a_null_gradient(gpu_device, skip):
    case = U.NORM_NULL_GRADS_CASE
    y, gamma, beta, dh = U.norm_inputs(case)
    r32, r64 = U.norm_refs(case)
    _, stats = _norm_train(gpu_device, case, y, gamma, beta)
    dy, dgamma, dbeta = _norm_backward(gpu_device, case, y, gamma, beta, dh, stats, want_dgamma=skip != "dgamma",
                                       want_dbeta=skip != "dbeta")
    name = "instnorm %s no %s " % (U.case_id(case), skip)
    U.check(name + "dy", _np(dy), r32["dy"], r64["dy"], U.NORM_SLICES)
    kept, left = (dbeta, dgamma) if skip == "dgamma" else (dgamma, dbeta)
    key = "dbeta" if skip == "dgamma" else "dgamma"
    U.check(name + key, _np(kept), r32[key], r64[key])
    assert U.is_pattern(left), "a NULL gradient was written somewhere else"


def test_instnorm_constant_channel(gpu_device):
    """Variance 0 in one channel: finite, and lrelu(beta_c) there."""
    case, ch = U.NORM_CONST_CASE, U.NORM_CONST_CHANNEL
    y, gamma, beta, dh = U.norm_inputs(case, const_channel=ch)
    r32, r64 = U.norm_refs(case, const_channel=ch)
    sl = U.NORM_SLICES + (("const", (Ellipsis, ch)),)
    name = "instnorm %s const-channel " % U.case_id(case)
    out = _norm_inference(gpu_device, case, y, gamma, beta)
    U.check(name + "inference", _np(out), r32["h"], r64["h"], sl)
    h, stats = _norm_train(gpu_device, case, y, gamma, beta)
    U.check(name + "train h", _np(h), r32["h"], r64["h"], sl)
    U.check(name + "train stats", _np(stats), r32["stats"], r64["stats"], STAT_SLICES)
    # torch's fp32 mean of a constant channel is not the constant, and rstd = 316 there: its own distance (9e-4) makes
    # the rule loose on that slice, so the channel is also held to lrelu(beta_c) itself, within 4 ulp
    b = beta.double().numpy()[ch]
    want = b if b > 0 else U.SLOPE * b
    assert np.all(r64["h"][:, :, ch] == want)
    for got in (_np(out), _np(h)):
        assert np.abs(got[:, :, ch].astype(np.float64) - want).max() <= 4 * np.spacing(np.float32(abs(want)))
    st = _np(stats)
    rstd0 = np.float32(1.0) / np.sqrt(np.float32(U.EPS))
    assert np.all(st[:, ch, 0] == y.numpy()[0, 0, ch]) and np.abs(st[:, ch, 1] - rstd0).max() <= 4 * np.spacing(rstd0)


def test_instnorm_large_offset(gpu_device):
    """|mean| = 1000 std: neither the statistics (partials taken relative to a per-channel pivot) nor the apply kernels
    may lose the low bits of y - mean.  No backward here: the fp32 inputs alone put a 3.5e-5 from fp64 at this offset,
    in PyTorch as in the library, which is above the kink margin any draw of 67584 elements offers (9e-6 here), so the
    sign LeakyReLU' reads near the kink is a coin toss that says nothing about the kernels."""
    case = U.NORM_OFFSET_CASE
    y, gamma, beta, dh = U.norm_inputs(case, off_mul=1000.0)
    r32, r64 = U.norm_refs(case, off_mul=1000.0)
    name = "instnorm %s off1000 " % U.case_id(case)
    out = _norm_inference(gpu_device, case, y, gamma, beta)
    U.check(name + "inference", _np(out), r32["h"], r64["h"], U.NORM_SLICES)
    h, stats = _norm_train(gpu_device, case, y, gamma, beta)
    U.check(name + "train h", _np(h), r32["h"], r64["h"], U.NORM_SLICES)
    U.check(name + "train stats", _np(stats), r32["stats"], r64["stats"], STAT_SLICES)
    assert torch.equal(out.view(torch.int32), h.view(torch.int32))


# ---------------------------------------------------------------------------------------- damc_conv2d_backward_nhwc
@pytest.mark.parametrize("case,want_dx", U.CONV_BWD_CASES, ids=[U.case_id(c) for c, _ in U.CONV_BWD_CASES])
def test_conv2d_backward_matches_fp64(gpu_device, case, want_dx):
    _lib, L, stream = _api(gpu_device)
    ptr = _lib.ptr
    B, hin, win, cin, cout, k, s, p = case
    x, w, bias, dy = U.conv_inputs(case)
    xd, wd, dyd = U.nhwc(x).to(gpu_device), w.to(gpu_device), U.nhwc(dy).to(gpu_device)
    nb = int(L.damc_conv2d_backward_workspace_bytes(*case))
    assert nb > 0
    ws = guarded(nb, gpu_device)
    dx = guarded((B, hin, win, cin), gpu_device)
    dw = guarded((cout, cin, k, k), gpu_device)
    db = guarded((cout,), gpu_device)
    _lib.check(L.damc_conv2d_backward_nhwc(ptr(xd), ptr(dyd), ptr(wd), B, hin, win, cin, cout, k, s, p,
                                           ptr(dx) if want_dx else None, ptr(dw), ptr(db), ptr(ws), nb, stream),
               "conv2d backward")
    assert_guards_intact()
    r32, r64 = U.conv_bwd_refs(case)
    name = "conv2d_bwd %s " % U.case_id(case)
    if want_dx:
        U.check(name + "dx", _np(dx), r32["dx"], r64["dx"], U.CONV_SLICES)
    else:
        assert U.is_pattern(dx)
    U.check(name + "dw", _np(dw), r32["dw"], r64["dw"], (("lastcout", (-1,)), ("lastcin", (slice(None), -1))))
    U.check(name + "db", _np(db), r32["db"], r64["db"])
    # db = NULL: the other gradients as before, db untouched
    U.reset_guards()
    ws = guarded(nb, gpu_device)
    dw2 = guarded((cout, cin, k, k), gpu_device)
    db2 = guarded((cout,), gpu_device)
    _lib.check(L.damc_conv2d_backward_nhwc(ptr(xd), ptr(dyd), ptr(wd), B, hin, win, cin, cout, k, s, p, None, ptr(dw2),
                                           None, ptr(ws), nb, stream), "conv2d backward")
    assert_guards_intact()
    assert U.is_pattern(db2)
    U.check(name + "dw (dx, db NULL)", _np(dw2), r32["dw"], r64["dw"])


# ------------------------------------------------------------------------------------------------ damc_nchw_to_nhwc
@pytest.mark.parametrize("B,C,HW", U.NCHW_CASES, ids=[U.case_id(c) for c in U.NCHW_CASES])
def test_nchw_to_nhwc_is_exact(gpu_device, B, C, HW):
    _lib, L, stream = _api(gpu_device)
    g = torch.Generator().manual_seed(B * 100 + C * 10 + HW)
    x = torch.randn(B, C, HW, generator=g)
    y = guarded((B, HW, C), gpu_device)
    xd = x.to(gpu_device)
    _lib.check(L.damc_nchw_to_nhwc(_lib.ptr(xd), B, C, HW, _lib.ptr(y), stream), "nchw_to_nhwc")
    assert_guards_intact()
    assert torch.equal(y.cpu(), x.permute(0, 2, 1).contiguous())
