"""Shared by tests/test_encoder_ops_cases_cpu.py and tests/test_gpu_encoder_ops.py: the case tables of the per-op
encoder entry points of include/damc.h (damc_gemm, damc_conv2d_nhwc, damc_conv2d_x3_nhwc, the three InstanceNorm calls,
damc_conv2d_backward_nhwc, damc_nchw_to_nhwc), their fp32 / fp64 PyTorch-CPU references, the accuracy rule and the
guarded device buffers.

Accuracy rule (tests/test_gpu_training.py, test_gpu_configs._check): the same operation on the same fp32 inputs with
PyTorch on the CPU in fp32 and in fp64; |hip - fp64| <= 3 |torch fp32 - fp64| + 1e-6 in rel-L2, for the whole output and
for the slices a tail bug would hit.  A slice whose fp64 norm is below 1e-3 x the output's RMS x sqrt(slice size) takes
that value as its denominator (gtrain_check's floor).

Guards: every output, workspace and strided-output gap sits inside a buffer filled with one NaN bit pattern, with 256
bytes of it in front and behind; assert_guards_intact() compares those regions as int32 after every library call.
"""
import functools

import numpy as np

# ------------------------------------------------------------------------------------------------ case tables
# conv tuples: (B, hin, win, cin, cout, k, stride, pad)

ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SILU, ACT_RELU = 0, 1, 2, 3, 4  # include/damc.h DAMC_ACT_*
SLOPE = 0.2
EPS = 1e-5

# damc_gemm: (M, N, K), dense leading dimensions, 256-B aligned operands
GEMM_CASES = [(1, 1, 4), (1, 8, 1), (3, 5, 2),  # K = 1 and 2: the scalar A path
              (128, 128, 32),                    # exact tile
              (129, 130, 36),                    # every tail at once; N % 4 != 0: the scalar B path
              (130, 257, 100)]                   # three N tiles, nz = 100
GEMM_ACT_CASE = (129, 130, 36)
GEMM_STRIDED = (37, 64, 128)                     # lda = K + 4, ldb = N + 4, ldc = N + 3
GEMM_MISALIGNED = (16, 12, 64)                   # A, B or C offset by one float

# damc_conv2d_nhwc; split: damc_conv2d_workspace_floats is non-zero (K-major with K >= 512 and few output tiles)
CONV_CASES = [
    ((2, 9, 7, 3, 5, 3, 1, 1), False),     # scalar gather, non-square
    ((3, 8, 8, 1, 8, 3, 1, 1), False),     # scalar gather, cin = 1
    ((2, 8, 6, 4, 6, 4, 2, 1), False),     # float4 gather
    ((1, 5, 5, 20, 7, 3, 2, 0), False),    # K = 180, K tiles straddle taps
    ((2, 8, 8, 32, 12, 4, 2, 1), True),    # K-major; cout % 8 != 0 (the limb engine declines)
    ((2, 4, 4, 64, 300, 4, 1, 0), True),   # three N tiles, M = 2
    ((2, 9, 7, 32, 16, 5, 2, 2), True),    # 25 taps, pad 2, non-square
    ((2, 6, 6, 64, 16, 1, 1, 0), False),   # k = 1
]
CONV_TOO_MANY_TAPS = (2, 8, 8, 32, 8, 6, 2, 2)  # 36 taps on the K-major engine (at most 32): must be refused

# damc_conv2d_x3_nhwc
X3_F32A_CASES = [
    (1, 8, 8, 32, 8, 4, 2, 1),       # one sign block, M = 16
    (3, 7, 7, 32, 24, 4, 2, 1),      # odd map
    (2, 6, 10, 96, 72, 4, 2, 1),     # non-square, 3 sign blocks
    (5, 8, 8, 160, 136, 4, 2, 1),    # K = 2560 = 5 sign blocks, N crosses the 128 tile
    (2, 16, 16, 64, 64, 4, 2, 1),    # M = 128
    (3, 16, 16, 64, 64, 4, 2, 1),    # M = 192, a partial 256-row tile
    (5, 16, 16, 32, 16, 4, 2, 1),    # M = 320, two M tiles
]
X3_LIMB_CASES = [
    (3, 5, 5, 32, 8, 3, 1, 1),       # K = 288, partial sign block
    (2, 9, 7, 32, 16, 5, 2, 2),      # K = 800
    (2, 6, 6, 64, 16, 1, 1, 0),      # K = 64
    (2, 4, 4, 256, 64, 4, 1, 0),     # K = 4096 = 8 sign blocks, M = 2: the narrow split
    (33, 4, 4, 256, 64, 4, 1, 0),    # the same head at M = 33
    (3, 3, 3, 512, 40, 3, 1, 0),     # K = 4608, nine sign blocks: the MNIST head
]
X3_CASES = X3_F32A_CASES + X3_LIMB_CASES
X3_UNSUPPORTED = [(2, 8, 8, 32, 12, 4, 2, 1), (2, 8, 8, 32, 8, 6, 2, 2)]  # cout % 8 != 0; 36 taps

# the norm calls: (B, hw, c); S = clamp(hw / 64, 1, 64) statistics splits, P = clamp(hw / 256, 1, 64) apply splits
NORM_CASES = [(1, 1, 1), (3, 9, 63), (2, 49, 65), (2, 63, 8), (2, 64, 64), (2, 65, 130),
              (1, 200, 64),     # S = 3, uneven
              (2, 1024, 33),    # S = 16, P = 4
              (1, 4097, 5)]     # S capped at 64, P = 16, both uneven
NORM_SPLITS = {(1, 200, 64): (3, 1), (2, 1024, 33): (16, 4), (1, 4097, 5): (64, 16)}
NORM_NULL_GRADS_CASE = (2, 65, 130)
NORM_CONST_CASE = (2, 65, 130)       # channel NORM_CONST_CHANNEL held constant (variance 0)
NORM_CONST_CHANNEL = 129
NORM_OFFSET_CASE = (2, 1024, 33)     # off_c = 1000 s_c
KINK_REL = 1e-6                      # no fp64 pre-activation within KINK_REL x its RMS of the LeakyReLU kink

# damc_conv2d_backward_nhwc: (case, dx requested)
CONV_BWD_CASES = [
    ((2, 6, 10, 96, 72, 4, 2, 1), True),     # non-square k4 s2 p1
    ((2, 8, 6, 4, 6, 4, 2, 1), True),        # cin = 4
    ((5, 8, 8, 160, 136, 4, 2, 1), True),    # batch not a multiple of 32
    ((2, 9, 7, 3, 5, 3, 1, 1), False),       # first conv, dx = NULL
    ((3, 8, 8, 1, 8, 3, 1, 1), False),
    ((2, 4, 4, 256, 64, 4, 1, 0), True),     # last conv covering its whole input
    ((3, 3, 3, 512, 40, 3, 1, 0), True),
    ((2, 4, 4, 64, 300, 4, 1, 0), True),
]

NCHW_CASES = [(1, 1, 1), (2, 3, 35), (3, 5, 64)]  # (B, C, HW)


def case_id(t):
    return "-".join(str(v) for v in t)


def conv_out_hw(case):
    B, hin, win, cin, cout, k, s, p = case
    return (hin + 2 * p - k) // s + 1, (win + 2 * p - k) // s + 1


def in_splits(hw):
    return max(1, min(64, hw // 64))


def apply_splits(hw):
    return max(1, min(64, hw // 256))


def _seed(tag, t):
    """A fixed seed per (table, case): the CPU kink check and the GPU tests draw the same inputs."""
    h = sum((i + 1) * 7919 * int(v) for i, v in enumerate(t))
    return (sum(ord(ch) for ch in tag) * 1000003 + h) % (2 ** 31 - 1)


# ------------------------------------------------------------------------------------------------ references
def _act(v, act):
    import torch
    import torch.nn.functional as F

    if act == ACT_LRELU:
        return F.leaky_relu(v, SLOPE)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SILU:
        return F.silu(v)
    if act == ACT_RELU:
        return F.relu(v)
    return v


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K):
    import torch

    g = torch.Generator().manual_seed(_seed("gemm", (M, N, K)))
    return (torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(N, generator=g))


@functools.lru_cache(maxsize=None)
def gemm_refs(M, N, K, act, with_bias=True):
    """(torch fp32, fp64) of act(A B + bias) on the fp32 inputs of gemm_inputs."""
    a, b, bias = gemm_inputs(M, N, K)
    out = []
    for dt in (a.dtype, a.double().dtype):
        v = a.to(dt) @ b.to(dt)
        if with_bias:
            v = v + bias.to(dt)
        out.append(_act(v, act).numpy())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def conv_inputs(case):
    """x (B, cin, hin, win) NCHW, w (cout, cin, k, k), bias (cout), dy (B, cout, ho, wo): fp32, fan-in scaled weight."""
    import torch

    B, hin, win, cin, cout, k, s, p = case
    ho, wo = conv_out_hw(case)
    g = torch.Generator().manual_seed(_seed("conv", case))
    x = torch.randn(B, cin, hin, win, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / float(np.sqrt(cin * k * k))
    bias = torch.randn(cout, generator=g)
    dy = torch.randn(B, cout, ho, wo, generator=g)
    return x, w, bias, dy


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv_refs(case, with_bias=True):
    """(torch fp32, fp64) of conv2d(x, w, bias), NHWC."""
    import torch.nn.functional as F

    B, hin, win, cin, cout, k, s, p = case
    x, w, bias, _ = conv_inputs(case)
    return tuple(nhwc(F.conv2d(x.to(dt), w.to(dt), bias.to(dt) if with_bias else None, stride=s, padding=p)).numpy()
                 for dt in (x.dtype, x.double().dtype))


@functools.lru_cache(maxsize=None)
def conv_bwd_refs(case):
    """(torch fp32, fp64) of {dx NHWC, dw (cout, cin, k, k), db (cout)} for the output gradient dy of conv_inputs."""
    import torch.nn.functional as F

    B, hin, win, cin, cout, k, s, p = case
    x, w, bias, dy = conv_inputs(case)
    out = []
    for dt in (x.dtype, x.double().dtype):
        xs, wt, bs = (t.to(dt).clone().requires_grad_(True) for t in (x, w, bias))
        F.conv2d(xs, wt, bs, stride=s, padding=p).backward(dy.to(dt))
        out.append(dict(dx=nhwc(xs.grad).numpy(), dw=wt.grad.numpy(), db=bs.grad.numpy()))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def norm_inputs(case, off_mul=8.0, const_channel=-1):
    """y (B, hw, c) = off_c + s_c N(0, 1) with s_c in [0.5, 2], off_c = off_mul s_c; gamma, beta (c); dh (B, hw, c)."""
    import torch

    B, hw, c = case
    g = torch.Generator().manual_seed(_seed("norm", case) + int(off_mul) + 31 * (const_channel + 1))
    sc = 0.5 + 1.5 * torch.rand(c, generator=g)
    y = sc * off_mul + sc * torch.randn(B, hw, c, generator=g)
    gamma = torch.randn(c, generator=g)
    beta = torch.randn(c, generator=g)
    dh = torch.randn(B, hw, c, generator=g)
    if const_channel >= 0:
        y[:, :, const_channel] = y[0, 0, const_channel]
    return y.contiguous(), gamma, beta, dh


def _norm_eval(y, gamma, beta, dh, dt):
    """InstanceNorm2d(affine, eps, biased variance) + LeakyReLU on (B, hw, c) and its backward, in dtype dt."""
    import torch
    import torch.nn.functional as F

    ys, gs, bs = (t.to(dt).clone().requires_grad_(True) for t in (y, gamma, beta))
    mean = ys.mean(dim=1, keepdim=True)
    var = ((ys - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    a = (ys - mean) * rstd * gs + bs
    h = F.leaky_relu(a, SLOPE)
    h.backward(dh.to(dt))
    stats = torch.stack([mean[:, 0], rstd[:, 0]], dim=-1)  # (B, c, 2)
    return dict(a=a.detach().numpy(), h=h.detach().numpy(), stats=stats.detach().numpy(), dy=ys.grad.numpy(),
                dgamma=gs.grad.numpy(), dbeta=bs.grad.numpy())


@functools.lru_cache(maxsize=None)
def norm_refs(case, off_mul=8.0, const_channel=-1):
    """(torch fp32, fp64) dicts {a, h, stats (B, c, 2) = {mean, rstd}, dy, dgamma, dbeta}."""
    import torch

    y, gamma, beta, dh = norm_inputs(case, off_mul, const_channel)
    return _norm_eval(y, gamma, beta, dh, torch.float32), _norm_eval(y, gamma, beta, dh, torch.float64)


def kink_margin(case, off_mul=8.0, const_channel=-1):
    """min |a| / rms(a) of the fp64 pre-activation."""
    a = norm_refs(case, off_mul, const_channel)[1]["a"]
    if const_channel >= 0:
        a = np.delete(a, const_channel, axis=2)
    return float(np.abs(a).min() / max(np.sqrt(np.mean(a * a)), 1e-300))


# ------------------------------------------------------------------------------------------------ the bound
def distances(got, ref32, ref64, slices=()):
    """[(label, |hip - fp64|, |torch32 - fp64|)] in rel-L2 for the whole output and each (label, index) slice."""
    got = np.asarray(got, dtype=np.float64)
    ref32 = np.asarray(ref32, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref32.shape, ref64.shape)
    rms = float(np.sqrt(np.mean(ref64 * ref64))) if ref64.size else 0.0
    rows = []
    for label, idx in (("all", Ellipsis),) + tuple(slices):
        r = ref64[idx]
        den = max(float(np.linalg.norm(r)), 1e-3 * rms * np.sqrt(max(r.size, 1)), 1e-30)
        rows.append((label, float(np.linalg.norm(got[idx] - r)) / den, float(np.linalg.norm(ref32[idx] - r)) / den))
    return rows


def report(name, got, ref32, ref64, slices=()):
    """Print both distances per slice; returns the rows."""
    assert np.isfinite(np.asarray(got)).all(), name + ": non-finite output"
    rows = distances(got, ref32, ref64, slices)
    for label, e, e32 in rows:
        print("%-58s %-10s hip-fp64 %.3e  torch32-fp64 %.3e" % (name, label, e, e32))
    return rows


def check(name, got, ref32, ref64, slices=()):
    """Print both distances per slice, then assert |hip - fp64| <= 3 |torch32 - fp64| + 1e-6 for each."""
    for label, e, e32 in report(name, got, ref32, ref64, slices):
        assert e <= 3.0 * e32 + 1e-6, (name, label, e, e32)


GEMM_SLICES = (("lastrow", (-1,)), ("lastcol", (Ellipsis, -1)))           # (M, N)
CONV_SLICES = (("lastpixrow", (-1, -1)), ("lastchan", (Ellipsis, -1)))     # NHWC (B, ho, wo, cout)
NORM_SLICES = (("lastchan", (Ellipsis, -1)), ("lastpix", (slice(None), -1)))  # (B, hw, c)

# ------------------------------------------------------------------------------------------------ guarded buffers
GUARD_WORD = 0x7FC5A5A5  # a quiet NaN: compared as int32
_GUARDED = []


def reset_guards():
    del _GUARDED[:]


def guarded(nbytes_or_shape, device, lead=256, tail=256):
    """A device buffer of nbytes (int: a uint8 payload view) or of a float32 shape (tuple), with `lead` bytes in front
    and `tail` bytes behind, the whole buffer filled with GUARD_WORD.  lead = 256 keeps the payload 256-B aligned;
    lead = 260 offsets it by one float."""
    import torch

    assert lead % 4 == 0 and tail % 4 == 0
    if isinstance(nbytes_or_shape, (tuple, list)):
        shape = tuple(int(v) for v in nbytes_or_shape)
        nbytes = 4 * int(np.prod(shape)) if shape else 4
    else:
        shape, nbytes = None, int(nbytes_or_shape)
    words = (nbytes + 3) // 4
    buf = torch.full((lead // 4 + words + tail // 4,), GUARD_WORD, dtype=torch.int32, device=device)
    assert not buf.is_cuda or buf.data_ptr() % 256 == 0
    _GUARDED.append((buf, lead // 4, words))
    mid = buf[lead // 4:lead // 4 + words]
    if shape is None:
        return mid.view(torch.uint8)[:nbytes]
    return mid.view(torch.float32).reshape(shape)


def is_pattern(t):
    """True when every 32-bit word of the float32 tensor t still holds GUARD_WORD."""
    import torch

    return bool((t.contiguous().view(torch.int32) == GUARD_WORD).all().item())


def assert_guards_intact():
    """Synchronise and compare the lead and tail region of every guarded buffer made since reset_guards()."""
    import torch

    if any(buf.is_cuda for buf, _, _ in _GUARDED):
        torch.cuda.synchronize()
    for i, (buf, lead, words) in enumerate(_GUARDED):
        front = int((buf[:lead] != GUARD_WORD).sum().item())
        back = int((buf[lead + words:] != GUARD_WORD).sum().item())
        assert front == 0 and back == 0, ("guarded buffer %d (%d payload words): %d words overwritten in front, "
                                          "%d behind" % (i, words, front, back))


# ------------------------------------------------------------------------------------------------ the whole forward
# Shared by tests/test_encoder_forms_cases_cpu.py and tests/test_gpu_encoder_forms.py: the cases that run
# damc_q_encoder_fwd on Encoder_* modules under every switch setting that changes which kernel runs, and the dispatch
# predicates of csrc/encoder.hip (enc_shapes, damc_q_encoder_fwd), csrc/enc_first.hip (launch_first_layer) and
# csrc/enc_head.hip (launch_dense_head_x3) restated in Python.
FWD_B, FWD_NEMB = 2, 128

# (Encoder_* name, image side, nc, nif, {DAMC_ENC_<switch>: value}, engine)
FWD_CASES = [
    ("cifar10", 32, 3, 64, {}, "limb"),                                                 # conv3_in_fused<3>
    ("cifar10", 32, 3, 64, {"FIRST_ONEPASS": "0"}, "limb"),                             # conv3_mfma<3, 4, *>
    ("cifar10", 32, 3, 64, {"FIRST_ONEPASS": "0", "FIRST_MFMA": "0"}, "limb"),          # conv3_stats<3, 4>, apply<3, 1>
    ("cifar10", 32, 3, 64, {"FIRST_ONEPASS": "0", "FIRST_MFMA": "0", "FIRST_PX": "1"}, "limb"),  # conv3_stats<3, 1>
    ("cifar10", 32, 3, 64, {"F32A": "0"}, "limb"),                                      # one-pass kernels' limb stores
    ("cifar10", 32, 3, 64, {"IN_ONEPASS": "0"}, "limb"),                                # in_strip_stats, in_stats
    ("cifar10", 32, 3, 64, {"IN_ONEPASS": "0", "IN_STRIP": "0"}, "limb"),               # in_stats at hw = 256 (S = 4)
    ("cifar10", 32, 3, 64, {"IN_ONEPASS": "0", "F32A": "0"}, "limb"),                   # in_apply_x3 throughout
    ("cifar10", 32, 3, 64, {"IN_ONEPASS": "0", "IN_STRIP": "0", "F32A": "0"}, "limb"),
    ("cifar10", 32, 3, 64, {"HEAD": "0"}, "limb"),                                      # the last conv on the limb GEMM
    ("cifar10", 32, 3, 64, {"HEAD": "1"}, "limb"),
    ("cifar10", 32, 3, 64, {"HEAD_PD": "1"}, "limb"),                                   # enc_head_x3<1>
    ("cifar10", 32, 3, 64, {}, "fp32"),                                                 # in_stats_pivot, in_apply
    ("cifar10", 32, 4, 64, {}, "limb"),                                                 # conv3_in_fused<4>
    ("cifar10", 32, 4, 64, {"FIRST_ONEPASS": "0"}, "limb"),                             # conv3_stats<4, 4>: no MFMA
    ("cifar10", 32, 4, 64, {"FIRST_ONEPASS": "0", "FIRST_PX": "1"}, "limb"),            # conv3_stats<4, 1>
    ("mnist", 28, 1, 64, {}, "limb"),                                                   # conv3_in_fused<1>, 3 x 3 head
    ("mnist", 28, 1, 64, {"FIRST_ONEPASS": "0"}, "limb"),                               # conv3_stats<1, 4>: W % 16 != 0
    ("mnist", 28, 1, 64, {"FIRST_ONEPASS": "0", "FIRST_PX": "1"}, "limb"),              # conv3_stats<1, 1>
    ("celeba64", 64, 3, 64, {}, "limb"),                   # conv3_mfma<3, 4, *>, the strip norm at 1024 pixels
    ("celeba64", 64, 3, 64, {"FIRST_MFMA": "0"}, "limb"),  # conv3_stats<3, 4> over 8 strips
    ("celeba64", 64, 3, 64, {"IN_STRIP": "0"}, "limb"),    # in_stats at 1024 pixels (S = 16)
    ("celeba64", 64, 3, 64, {"IN_ONEPASS": "0"}, "limb"),
    ("celeba64", 64, 1, 64, {}, "limb"),                   # conv3_mfma<1, 4, *>
    ("celeba64", 64, 3, 128, {}, "limb"),                  # conv3_mfma<3, 8, *>
    ("celeba64", 64, 1, 128, {}, "limb"),                  # conv3_mfma<1, 8, *>
]

# the kernel instantiations of csrc/enc_norm.hip, csrc/enc_first.hip and csrc/enc_head.hip
FWD_KERNELS = (
    ["in_stats_kernel", "in_stats_pivot_kernel", "in_apply_kernel", "in_merge_kernel", "in_strip_stats_kernel",
     "in_apply_f32_kernel", "in_apply_x3_kernel", "in_fused_x3_kernel<1>", "in_fused_x3_kernel<2>",
     "in_fused_x3_kernel<4>", "in_apply_train_kernel", "in_bwd_sums_kernel", "in_bwd_apply_kernel"]
    + ["conv3_in_fused_kernel<%d>" % c for c in (1, 3, 4)]
    + ["conv3_stats_kernel<%d, %d>" % (c, p) for c in (1, 3, 4) for p in (1, 4)]
    + ["conv3_apply_x3_kernel<%d, 1>" % c for c in (1, 3, 4)]
    + ["conv3_mfma_kernel<%d, %d, %s>" % (c, t, s) for c in (1, 3) for t in (4, 8) for s in ("true", "false")]
    + ["enc_head_x3_kernel<1>", "enc_head_x3_kernel<4>", "enc_head_reduce_kernel"])

_ENC_TOPOLOGY = {  # src/diffusion_net.py: (hidden channel multipliers of nif, the last conv's kernel)
    "cifar10": ((1, 2, 4, 8), 4), "celeba64": ((1, 2, 4, 8, 8), 4), "celebaHQ": ((1, 2, 4, 4, 8, 8, 8), 4),
    "mnist": ((1, 2, 4, 8), 3)}


def fwd_case_id(case):
    name, hw, nc, nif, sw, engine = case
    tag = "-".join("%s=%s" % kv for kv in sorted(sw.items())) or "default"
    return "%s-%d-nc%d-nif%d-%s-%s" % (name, hw, nc, nif, engine, tag)


def enc_layers(name, nc, nif, nemb=FWD_NEMB):
    """[(cin, cout, k, stride, pad, has_norm)] of Encoder_<name>(nc, nemb, nif)."""
    mults, k_last = _ENC_TOPOLOGY[name]
    out, cin = [], nc
    for i, m in enumerate(mults):
        out.append((cin, nif * m) + ((3, 1, 1) if i == 0 else (4, 2, 1)) + (True,))
        cin = nif * m
    return out + [(cin, nemb, k_last, 1, 0, False)]


def module_layers(enc):
    """The same list read from an Encoder_* module."""
    import torch

    mods, out = list(enc.net), []
    for i, m in enumerate(mods):
        if isinstance(m, torch.nn.Conv2d):
            norm = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.InstanceNorm2d)
            out.append((m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], norm))
    return out


def x3_ksplit(M, N, K, bm=256, bn=128, negk=512):
    """csrc/gemm_x3.hip x3_ksplit's default rule (zdim = 1): the slices a limb conv's K is split into."""
    wgs = ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
    if K % negk or K // negk < 2:
        return 1
    ks = K // negk
    return ks if (wgs < 128 or (wgs < 256 and ks <= 16)) else 1


def forward_kernels(layers, H, W, B, sw=None, engine="limb", slope=0.2):
    """The kernel instantiations of enc_norm.hip, enc_first.hip and enc_head.hip that one damc_q_encoder_fwd call
    launches, in launch order, for the layer list of enc_layers / module_layers as damc.amortizer.EncoderPlan describes
    it (limb layers hand over their PyTorch weight, 16-byte aligned; xemb 16-byte aligned).  sw: DAMC_ENC_<key> values.
    The convolutions, the weight packing and the limb splits (gemm*.hip, x3_pack.hip) are not listed."""
    sw = sw or {}
    off = lambda key: sw.get(key) == "0"  # noqa: E731
    n = len(layers)
    kmajor = lambda c: c > 0 and c % 32 == 0  # noqa: E731
    limb = [engine == "limb" and kmajor(cin) and cout % 8 == 0 and k * k <= 32 for cin, cout, k, s, p, nm in layers]
    h, w = [H], [W]
    for cin, cout, k, s, p, nm in layers:
        h.append((h[-1] + 2 * p - k) // s + 1)
        w.append((w[-1] + 2 * p - k) // s + 1)
    assert h[n] == 1 and w[n] == 1
    cin0, C0, k0, s0, p0, nm0 = layers[0]
    first_fused = (n > 1 and limb[1] and (k0, s0, p0) == (3, 1, 1) and cin0 in (1, 3, 4) and C0 % 64 == 0 and
                   C0 <= 512 and nm0 and not kmajor(cin0) and W <= 1024)
    nl = n - 1
    cinh, couth, kh, sh_, ph, _ = layers[nl]
    head_geom = (nl >= 2 and limb[nl] and sh_ == 1 and ph == 0 and h[nl] == kh and w[nl] == kh and couth % 64 == 0 and
                 (cinh * kh * kh) % 512 == 0 and layers[nl - 1][5] and layers[nl - 1][1] % 32 == 0)
    head = head_geom and not off("HEAD") and not off("IN_ONEPASS")

    def f32a_layer(i):
        return not off("F32A") and i < n and limb[i] and layers[i][2:5] == (4, 2, 1)

    out, i0 = [], 0
    if first_fused:
        want = max(1, min(64, H * W // 512))
        R = max((H + want - 1) // want, (128 + W - 1) // W)
        assert ((R + 2) * (W + 2) * cin0 + 9 * cin0 * C0 + C0) * 4 <= 65536
        sm1 = ((H + 2) * (W + 2) * cin0 + 9 * cin0 * 16 + 8 * 8 + 32) * 4
        one = not off("FIRST_ONEPASS") and H * W <= 1024 and W % 4 == 0 and C0 % 16 == 0 and sm1 <= 65536
        smw = 3 * (R + 2) * (W + 2) * cin0 * 2
        mf = (not one and not off("FIRST_MFMA") and cin0 in (1, 3) and C0 in (64, 128) and W % 16 == 0 and
              smw <= 49152 and 0.0 <= slope <= 1.0)
        px = 4 if (W % 4 == 0 and sw.get("FIRST_PX") != "1") else 1
        if one:
            out.append("conv3_in_fused_kernel<%d>" % cin0)
        elif mf:
            out += ["conv3_mfma_kernel<%d, %d, true>" % (cin0, C0 // 16), "in_merge_kernel",
                    "conv3_mfma_kernel<%d, %d, false>" % (cin0, C0 // 16)]
        else:
            out += ["conv3_stats_kernel<%d, %d>" % (cin0, px), "in_merge_kernel",
                    "conv3_apply_x3_kernel<%d, 1>" % cin0]
        i0 = 1
    for i in range(i0, n):
        cin, cout, k, s, p, nm = layers[i]
        hw = h[i + 1] * w[i + 1]
        if head and i == n - 1:
            out += ["enc_head_x3_kernel<%d>" % (1 if sw.get("HEAD_PD") == "1" else 4), "enc_head_reduce_kernel"]
            continue
        nxt = i + 1 < n and limb[i + 1]
        in1 = nm and nxt and cout % 32 == 0 and hw <= 256 and not off("IN_ONEPASS")
        strip = (nm and not in1 and nxt and cout % 8 == 0 and limb[i] and hw % 256 == 0 and hw // 256 <= 64 and
                 not off("IN_STRIP"))
        if not nm:
            continue
        if in1:
            out.append("in_fused_x3_kernel<%d>" % (1 if hw <= 64 else 2 if hw <= 128 else 4))
        elif nxt and cout % 8 == 0:
            if not strip:
                out.append("in_stats_kernel")
            elif x3_ksplit(B * hw, cout, k * k * cin) > 1:  # else the conv's epilogue took them (its unsplit tile)
                out.append("in_strip_stats_kernel")
            out += ["in_merge_kernel", "in_apply_f32_kernel" if f32a_layer(i + 1) else "in_apply_x3_kernel"]
        else:
            out += ["in_stats_pivot_kernel", "in_apply_kernel"]
    return out
