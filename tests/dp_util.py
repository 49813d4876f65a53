"""Shared by tests/test_dp_cpu.py and tests/test_gpu_dp.py: a numpy Philox4x32-10 with the key / counter packing of
csrc/common.h's philox_normal4, guarded device buffers, and the layout arithmetic of a gradient bucket."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
PACK_SIZES = [1, 3, 4, 5, 8191, 8192, 8193]
GUARD = 64  # floats on either side of a guarded buffer (256 B: the slice in the middle keeps 16-byte alignment)
SENTINEL = 12345.0


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds over uint64 arrays holding 32-bit words; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & MASK), np.asarray(k1, dtype=np.uint64) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def philox_block(seed, chain, step, quad, stream_id):
    """The block of (seed, chain, step, quad, stream_id) as philox_normal4 packs it: counter = (quad, step lo, chain lo,
    stream_id ^ chain hi * 0x9E3779B9), key = (seed lo, seed hi ^ step hi).  chain / step: Python ints or int arrays
    (object dtype for values past 2^63)."""
    chain = np.asarray(chain, dtype=object)
    step = np.asarray(step, dtype=object)
    lo = lambda a: np.asarray(a & MASK, dtype=np.uint64)  # noqa: E731
    hi = lambda a: np.asarray((a >> 32) & MASK, dtype=np.uint64)  # noqa: E731
    c3 = np.uint64(stream_id) ^ ((hi(chain) * np.uint64(W0)) & MASK)
    k1 = np.uint64((seed >> 32) & MASK) ^ hi(step)
    return philox4x32_10(np.uint64(quad), lo(step), lo(chain), c3, seed & MASK, k1)


def philox_uniform(n_steps, batch, seed, step_offset, chain_base, stream_id):
    """damc_philox_uniform's contract: (n_steps, batch) fp32, (word 0 >> 8) * 2^-24."""
    st, r = np.meshgrid(np.arange(n_steps), np.arange(batch), indexing="ij")
    chain = np.array([int(chain_base) + int(v) for v in r.reshape(-1)], dtype=object)
    step = np.array([int(step_offset) + int(v) for v in st.reshape(-1)], dtype=object)
    w0 = philox_block(int(seed), chain, step, 0, stream_id)[0]
    return ((w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(n_steps, batch)


def guarded(n, device, fill=SENTINEL):
    """(whole, view): a tensor of n floats between two GUARD-float zones holding SENTINEL; the view starts filled with
    `fill`."""
    import torch

    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
    view = whole[GUARD:GUARD + n]
    view.fill_(fill)
    return whole, view


def guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def many_sizes(n=200):
    """A > 96-tensor size list: mostly small odd sizes, a few past one chunk."""
    return [(37 * i) % 61 + 1 if i % 50 else 8192 + i for i in range(n)]
