"""CPU: the host side of the data-parallel update -- argument checks of the new entry points, the gradient bucket's
layout arithmetic, iteration_seed, GradBucket.verify over gloo (world 2), and the no-fallback rule of the seeded
Q.calculate_loss."""
import ctypes
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from dp_util import PACK_SIZES, many_sizes

ERR_ARG = 1001


def test_new_entry_points_refuse_bad_arguments_on_the_host():
    from damc import _lib

    L = _lib.lib()
    assert L.damc_abi_version() == 3
    ll = (ctypes.c_longlong * 2)(0, 4)
    neg = (ctypes.c_longlong * 2)(0, -4)
    ptrs = (ctypes.c_void_p * 2)(8, 8)
    # damc_grad_pack: NULL table / pointer array / offsets / bucket, too many tensors, a negative offset
    assert L.damc_grad_pack(None, 1, ptrs, ll, 2, 1.0, 8, None) == ERR_ARG
    assert L.damc_grad_pack(8, 1, None, ll, 2, 1.0, 8, None) == ERR_ARG
    assert L.damc_grad_pack(8, 1, ptrs, None, 2, 1.0, 8, None) == ERR_ARG
    assert L.damc_grad_pack(8, 1, ptrs, ll, 2, 1.0, None, None) == ERR_ARG
    assert L.damc_grad_pack(8, -1, ptrs, ll, 2, 1.0, 8, None) == ERR_ARG
    assert L.damc_grad_pack(8, 1, ptrs, ll, _lib.ADAM_MAX_TENSORS + 1, 1.0, 8, None) == ERR_ARG
    assert L.damc_grad_pack(8, 1, ptrs, neg, 2, 1.0, 8, None) == ERR_ARG
    # damc_philox_uniform
    assert L.damc_philox_uniform(None, 1, 4, 1, 0, 0, _lib.STREAM_QU, None) == ERR_ARG
    assert L.damc_philox_uniform(8, 0, 4, 1, 0, 0, _lib.STREAM_QU, None) == ERR_ARG
    assert L.damc_philox_uniform(8, 1, 0, 1, 0, 0, _lib.STREAM_QU, None) == ERR_ARG
    # damc_q_noise_glue_seeded: the code damc_q_noise_glue returns for NULL pointers
    assert L.damc_q_noise_glue(None, None, None, 4, 8, -5.1, 9.8, None, 128, None, None, None, None) == ERR_ARG
    good = dict(z=8, B=4, nz=8, freqs=8, ntemb=128, eps=8, zt=8, temb=8)

    def seeded(**kw):
        a = dict(good, **kw)
        return L.damc_q_noise_glue_seeded(a["z"], a["B"], a["nz"], -5.1, 9.8, a["freqs"], a["ntemb"], 1, 0, 0, None,
                                          a["eps"], None, a["zt"], a["temb"], None)

    for bad in (dict(z=None), dict(freqs=None), dict(eps=None), dict(zt=None), dict(temb=None), dict(B=0), dict(nz=0),
                dict(ntemb=127), dict(ntemb=0)):
        assert seeded(**bad) == ERR_ARG, bad


def test_numpy_philox_known_answers():
    """The tests' Philox4x32-10 against Random123's published vectors (kat_vectors: zeros, and all ones)."""
    import dp_util

    got = [int(v) for v in dp_util.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    got = [int(v) for v in dp_util.philox4x32_10(f, f, f, f, f, f)]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    u = dp_util.philox_uniform(2, 3, 42, 2 ** 32 + 1, 2 ** 32 + 3, 0x55)
    assert u.shape == (2, 3) and u.dtype.name == "float32" and (u >= 0).all() and (u < 1).all()


def _check_layout(sizes):
    from damc import dist

    offs, total = dist.bucket_layout(sizes)
    assert len(offs) == len(sizes)
    assert all(o % 4 == 0 for o in offs) and total % 4 == 0
    end = 0
    for o, n in zip(offs, sizes):
        assert o >= end  # in order, no overlap
        assert o - end < 4  # and no more padding than the rounding needs
        end = o + n
    assert end <= total < end + 4
    return offs, total


def test_bucket_layout_is_aligned_ordered_and_disjoint():
    from damc import _lib, optim

    offs, total = _check_layout(PACK_SIZES)
    assert offs == [0, 4, 8, 12, 20, 8212, 16404] and total == 24600
    sizes = many_sizes(200)
    _check_layout(sizes)
    # more than DAMC_ADAM_MAX_TENSORS tensors go in slices of <= 96 whose chunk counts add up
    chunks = optim._Chunks.of(sizes, torch.device("cpu"))
    assert [(t0, t1) for t0, t1, *_ in chunks.slices] == [(0, 96), (96, 192), (192, 200)]
    want = [sum(-(-n // _lib.ADAM_CHUNK) for n in sizes[t0:t1]) for t0, t1, *_ in chunks.slices]
    assert [n for _, _, _, n, _ in chunks.slices] == want
    assert [b for *_, b in chunks.slices] == [0, want[0], want[0] + want[1]]
    assert chunks.nchunks == sum(want) == sum(-(-n // _lib.ADAM_CHUNK) for n in sizes)


def test_iteration_seed_is_a_pure_hash_below_2_62():
    from damc import dist

    seen = set()
    for it in range(16):
        for purpose in range(6):
            s = dist.iteration_seed(1234, it, purpose)
            assert s == dist.iteration_seed(1234, it, purpose)
            assert 0 <= s < 2 ** 62
            seen.add(s)
    assert len(seen) == 16 * 6
    assert dist.iteration_seed(1235, 0, 0) not in seen
    assert dist.iteration_seed(2 ** 62 - 1, 2 ** 40, 3) < 2 ** 62


def test_seeded_calculate_loss_refuses_cpu_tensors():
    from damc import _lib
    from src import diffusion_net as dn

    Q = dn._netQ_U_toy(nz=2, nxemb=16, ntemb=16, nf=1)
    x, z = torch.zeros(4, 2), torch.zeros(4, 2)
    with pytest.raises(_lib.DamcError):
        Q.calculate_loss(x=x, z=z, seed=1)
    with pytest.raises(_lib.DamcError):
        Q.calculate_loss(z=z, seed=1, draw_index=3, chain_base=8)
    assert Q.calculate_loss(x=x, z=z).shape == (4,)  # the unseeded call is untouched


def test_grad_bucket_refuses_cpu_gradients():
    from damc import _lib, dist

    p = torch.nn.Parameter(torch.zeros(5))
    p.grad = torch.ones(5)
    with pytest.raises(_lib.DamcError):
        dist.GradBucket([p]).pack(1.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _verify_worker(rank, world, port, q):
    import datetime

    import torch.distributed as d

    from damc import dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    d.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    params = [torch.nn.Parameter(torch.zeros(n)) for n in (3, 8, 5)]
    for p in params:
        p.grad = torch.ones_like(p)
    bucket = dist.GradBucket(params)
    out = []
    bucket.verify()  # the ranks agree
    out.append("ok")
    if rank == 1:
        params[1].grad = None
    try:
        bucket.verify()
        out.append("ok")
    except RuntimeError as e:
        out.append("raised: %s" % e)
    q.put((rank, out))
    d.destroy_process_group()


def test_verify_raises_on_every_rank_when_one_lacks_a_gradient():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_verify_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=120) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    for rank in range(world):
        first, second = res[rank]
        assert first == "ok"
        assert second.startswith("raised: GradBucket.verify"), (rank, second)
