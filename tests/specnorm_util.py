"""Shared by tests/test_specnorm_cpu.py and tests/test_gpu_specnorm.py: a plain-torch restatement, in a given dtype, of
one forward of torch.nn.utils.spectral_norm's SpectralNorm.compute_weight on the in-place 3-d view [A][R][K] of a
weight_orig (matrix row = the middle index, column = a * K + k: include/damc.h damc_specnorm_forward) and of the gradient
formula damc_specnorm_backward implements, plus the case table of the per-op GPU tests.
"""
import functools

# (A, R, K).  The tile of csrc/specnorm.hip is 256 lanes = slab lanes x row lanes x column lanes over 16-byte (K % 4 == 0)
# or scalar column groups, 8 rows per row lane, 4 slabs per slab lane; the elementwise kernels take 4096 elements a block.
CASES = [
    (1, 3, 5),         # Linear, scalar path, one partial tile
    (1, 1, 200),       # one row: u = +-1
    (1, 200, 128),     # _netE layer 1: 32 column lanes x 8 row lanes, 4 row chunks of 64 (tail 8)
    (1, 200, 200),     # _netE layer 2: 64 column lanes (50 used) x 4 row lanes, 7 row chunks of 32 (tail 8)
    (4, 3, 9),         # ConvTranspose2d k3 output layer, scalar path
    (33, 7, 16),       # k4: 4 column lanes x 8 row lanes x 8 slab lanes, 2 slab chunks of 32 (tail 1)
    (128, 128, 64),    # projection-layer shape: 16 x 16 x 1 lanes, 32 slab chunks, 256 elementwise blocks
    # at least two blocks along both reduced axes, a tail on each.  Scalar path, K = 9 -> 16 column lanes x 16 row lanes:
    # rows (reduced by W^T u) in 2 chunks of 128 with a tail of 2, slabs (reduced by W v) in 2 chunks of 4 with a tail of
    # 2; 7020 elements = 2 elementwise blocks with a tail
    (6, 130, 9),
    # 16-byte path past the 256 column lanes: 275 column groups in 2 column chunks (tail 19), 1 row lane -> 3 row chunks
    # of 8 (tail 4)
    (1, 20, 1100),
]
EPS = 1e-12  # nn.utils.spectral_norm's default


def case_id(c):
    return "-".join(str(v) for v in c)


def seed_of(case):
    a, r, k = case
    return (a * 1000003 + r * 7919 + k * 31 + 17) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """w (A, R, K), u (R), v (A K) unit vectors as the wrapper initialises them, g (A, R, K) = dL/dW_hat: fp32."""
    import torch
    import torch.nn.functional as F

    a, r, k = case
    gen = torch.Generator().manual_seed(seed_of(case))
    w = torch.randn(a, r, k, generator=gen) / float((a * k) ** 0.5)
    u = F.normalize(torch.randn(r, generator=gen), dim=0, eps=EPS)
    v = F.normalize(torch.randn(a * k, generator=gen), dim=0, eps=EPS)
    g = torch.randn(a, r, k, generator=gen)
    return w, u, v, g


def matrix(w3):
    """The hook's weight matrix of the [A][R][K] view: (R, A K)."""
    a, r, k = w3.shape
    return w3.permute(1, 0, 2).reshape(r, a * k)


def forward_ref(w3, u, v, power_iterations, eps, dt):
    """(u, v, sigma, w_hat) after one compute_weight with this many power iterations, in dtype dt."""
    import torch
    import torch.nn.functional as F

    w3 = w3.to(dt)
    m = matrix(w3)
    u, v = u.to(dt).clone(), v.to(dt).clone()
    for _ in range(power_iterations):
        v = F.normalize(torch.mv(m.t(), u), dim=0, eps=eps)
        u = F.normalize(torch.mv(m, v), dim=0, eps=eps)
    sigma = torch.dot(u, torch.mv(m, v))
    return u, v, sigma, w3 / sigma


def backward_ref(g3, w_hat3, sigma, u, v):
    """dL/dW_orig = (G - <G, W_hat> u v^T) / sigma on the [A][R][K] view (u, v constants of the graph)."""
    a, r, k = g3.shape
    d = (g3 * w_hat3).sum()
    outer = u.reshape(1, r, 1) * v.reshape(a, 1, k)
    return (g3 - d * outer) / sigma


@functools.lru_cache(maxsize=None)
def refs(case, power_iterations):
    """(torch fp32, fp64) dicts {u, v, sigma, w_hat, dw} on the fp32 inputs of inputs(case); computed once, read-only."""
    import torch

    w, u, v, g = inputs(case)
    out = []
    for dt in (torch.float32, torch.float64):
        uu, vv, sigma, what = forward_ref(w, u, v, power_iterations, EPS, dt)
        dw = backward_ref(g.to(dt), what, sigma, uu, vv)
        out.append({k: t.numpy() for k, t in dict(u=uu, v=vv, sigma=sigma.reshape(1), w_hat=what, dw=dw).items()})
    return tuple(out)
