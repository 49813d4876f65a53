"""CPU: the host side of the iteration glue (csrc/schedule.hip, damc.schedule, damc.loop); no kernel is launched.

The three calls are exported and bound and the ABI version stays 3; every bad argument is refused on the host with
-DAMC_ERR_ARG before any launch (the pointers handed over are not device memory and this test has no device: a launch
would fail with a HIP error instead); the Python wrappers refuse CPU tensors, mismatched pairs and a non-capturable
optimiser; the per-consumer draw offsets that damc.loop documents equal a hand count over three iterations."""
import ctypes

import pytest
import torch

SYMBOLS = ("damc_iteration_advance", "damc_ema_update", "damc_lr_decay")
FAKE = ctypes.c_void_p(0x1000)


def test_symbols_are_exported_and_bound():
    from damc import _lib

    so = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(so, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.damc_abi_version() == _lib.ABI_VERSION == 3  # additive: the ABI version stays


def test_bad_arguments_are_refused_on_the_host():
    from damc import _lib

    L = _lib.lib()
    bad = -_lib.DAMC_ERR_ARG
    assert L.damc_iteration_advance(None, 1, None) == bad

    def ptrs(n):
        return (ctypes.c_void_p * max(n, 1))(*([0x2000] * max(n, 1)))

    def ema(chunks=FAKE, target="ok", source="ok", n=2, period=10):
        t = ptrs(n) if target == "ok" else target
        s = ptrs(n) if source == "ok" else source
        return L.damc_ema_update(chunks, 1, t, s, n, 0.005, 0.995, None, period, 1, None)

    assert ema(chunks=None) == bad          # null table
    assert ema(target=None) == bad          # null pointer arrays
    assert ema(source=None) == bad
    assert ema(n=0) == bad                  # ntensors outside 1..96
    assert ema(n=_lib.ADAM_MAX_TENSORS + 1) == bad
    assert ema(period=0) == bad
    hole = ptrs(2)
    hole[1] = None
    assert ema(target=hole) == bad          # a null entry
    assert ema(source=hole) == bad

    def decay(lr64=FAKE, lr32=FAKE, n=3, period=1000):
        return L.damc_lr_decay(lr64, lr32, n, 0.99, 1e-5, None, period, 1, None)

    assert _lib.LR_DECAY_MAX == 8
    assert decay(lr64=None) == bad
    assert decay(lr32=None) == bad
    assert decay(n=0) == bad
    assert decay(n=9) == bad                # n above 8
    assert decay(period=0) == bad


def test_clock_lives_on_the_device():
    from damc import _lib, schedule

    with pytest.raises(_lib.DamcError, match="device memory"):
        schedule.TrainClock("cpu")
    with pytest.raises(_lib.DamcError, match="device memory"):
        schedule.TrainClock(torch.device("cpu"), iteration=5)


def test_ema_target_refuses_what_the_kernel_does_not_take():
    from damc import _lib, schedule

    a, b = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(_lib.DamcError, match="shape"):
        schedule.EmaTarget([a, torch.zeros(12)], [b, torch.zeros(3, 4)])
    with pytest.raises(_lib.DamcError, match="float32"):
        schedule.EmaTarget([a.double()], [b.double()])
    with pytest.raises(_lib.DamcError, match="float32"):
        schedule.EmaTarget([a], [b.half()])
    with pytest.raises(_lib.DamcError, match="float32"):
        schedule.EmaTarget([torch.zeros(4, 6)[:, ::2]], [b])  # not contiguous
    with pytest.raises(_lib.DamcError, match="as many"):
        schedule.EmaTarget([a, a], [b])
    with pytest.raises(_lib.DamcError, match="HIP kernels only"):
        schedule.EmaTarget([a], [b])  # well-formed, but CPU tensors: no fallback


def test_lr_decay_needs_a_capturable_optimiser():
    from damc import _lib, optim, schedule

    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(_lib.DamcError, match="capturable"):
        schedule.LrDecay(optim.Adam([p], lr=2e-4))
    with pytest.raises(_lib.DamcError, match="capturable"):
        schedule.LrDecay([optim.Adam([p], lr=2e-4, capturable=True), optim.AdamW([p], lr=2e-4)])
    with pytest.raises(_lib.DamcError, match="capturable"):
        schedule.LrDecay(optim.Adam([p], lr=2e-4).param_groups[0])
    with pytest.raises(_lib.DamcError, match="ROCm device"):
        schedule.LrDecay(optim.Adam([p], lr=2e-4, capturable=True))  # capturable, but CPU parameters


def test_documented_draw_offsets_against_a_hand_count():
    """damc.loop's table: each consumer moves its counter by a fixed stride per iteration.  The hand count walks three
    iterations of the body's calls in order and adds what each documented call advances its DrawState by: the per-op
    hooks' explicit advance(1), the sweep's n_interval, the chains' n_steps, calculate_loss's 1 per update."""
    from damc import loop

    n, gl, el, nq = 7, 3, 4, 6
    count = dict.fromkeys(loop.CONSUMERS, 0)
    for it in range(3):
        assert loop.offsets(it, n, gl, el, nq) == count, it
        count["mask"] += 1          # philox_uniform + advance(1)
        count["zt_target"] += 1     # philox_normal + advance(1)
        count["sweep_target"] += n  # reverse_sweep(draws=)
        count["pe_prior"] += 1
        count["zt_prior"] += 1
        count["sweep_prior"] += n
        count["posterior"] += gl    # posterior_langevin(draws=), n_steps
        count["fresh"] += 1
        count["prior"] += el        # prior_langevin(draws=), n_steps
        for _ in range(nq):
            count["q"] += 1         # calculate_loss(draws=)
    assert loop.offsets(3, n, gl, el, nq) == count
    assert count == {"mask": 3, "zt_target": 3, "sweep_target": 21, "pe_prior": 3, "zt_prior": 3, "sweep_prior": 21,
                     "posterior": 9, "fresh": 3, "prior": 12, "q": 18}
    assert loop.strides(n, gl, el) == loop.offsets(1, n, gl, el, 6)
    sd = loop.seeds(2 ** 64 - 2)
    assert [sd[c] for c in loop.CONSUMERS[:4]] == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]  # one seed each, mod 2^64
    assert len(set(loop.seeds(11).values())) == len(loop.CONSUMERS)
    from damc import _lib

    with pytest.raises(_lib.DamcError, match="device memory"):
        loop.make_draws(1, "cpu")
