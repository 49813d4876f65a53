"""GPU: the iteration glue (csrc/schedule.hip through damc.schedule) against the reference driver's own expressions,
bit for bit.

The comparators are the lines of train_gen_recon.py:247-261 themselves: `rho * p + (1 - rho) * t` evaluated by torch on
the same device, `max(lr * 0.99, 1e-5)` evaluated by Python on doubles, and a host `if (it + 1) % period == 0`.  Every
comparison is torch.equal / == on the exact values: the kernels round where those expressions round, so there is no
tolerance to choose."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 8192
SENTINEL = -7.5e30
GUARD = 8  # sentinel elements before, between and after the carved tensors


def _carve(specs, device, gen):
    """Tensors carved from two guarded flat buffers (targets, sources).  specs: (numel, target_mis, source_mis), the
    misalignments in elements off a 16-byte boundary.  Values: normal draws with +0 and -0 planted.  Returns (targets,
    sources, (tbuf, tmask), (sbuf, smask)); mask marks the elements that belong to a tensor."""
    def layout(which):
        o, spans = GUARD, []
        for spec in specs:
            start = o + spec[which]
            spans.append((start, spec[0]))
            o = (start + spec[0] + 3) // 4 * 4 + GUARD
        return spans, o

    out = []
    for which in (1, 2):
        spans, total = layout(which)
        host = torch.full((total,), SENTINEL, dtype=torch.float32)
        mask = torch.zeros(total, dtype=torch.bool)
        for start, n in spans:
            v = torch.randn(n, generator=gen)
            v[::5] = 0.0
            v[2::7] = -0.0
            host[start:start + n] = v
            mask[start:start + n] = True
        buf = host.to(device)
        assert buf.data_ptr() % 16 == 0
        views = [buf[start:start + n] for start, n in spans]
        for v, spec in zip(views, specs):
            assert (v.data_ptr() % 16 == 0) == (spec[which] == 0)
        out.append((views, buf, mask.to(device)))
    (tv, tbuf, tmask), (sv, sbuf, smask) = out
    return tv, sv, (tbuf, tmask), (sbuf, smask)


def _bits(t):
    return t.view(torch.int32)


EMA_SPECS = ([(n, 0, 0) for n in (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)] +
             [(CHUNK + 5, 1, 1),     # both at a storage offset of 1 element: the scalar path over a whole chunk
              (CHUNK + 5, 0, 1)] +   # only the source misaligned
             [(2, 0, 0)] * 100)      # 110 tensors: two slices of at most 96


@pytest.mark.parametrize("rho", [0.005, 0.5, 0.0, 1.0])
def test_ema_is_the_reference_expression_bit_for_bit(gpu_device, rho):
    from damc import schedule

    gen = torch.Generator().manual_seed(1234)
    tv, sv, (tbuf, tmask), (sbuf, smask) = _carve(EMA_SPECS, gpu_device, gen)
    assert len(tv) == 110
    want = [rho * p + (1 - rho) * t for p, t in zip(sv, tv)]  # train_gen_recon.py:261, torch on the device
    sbuf0, tbuf0 = sbuf.clone(), tbuf.clone()
    ema = schedule.EmaTarget(sv, tv, rho=rho)
    assert len(ema._chunks.slices) == 2
    ema.update()  # no clock: always
    torch.cuda.synchronize()
    for i, (t, w) in enumerate(zip(tv, want)):
        assert torch.equal(_bits(t), _bits(w)), "pair %d (numel %d) differs from rho * p + (1 - rho) * t" % (i, t.numel())
    assert torch.equal(_bits(sbuf), _bits(sbuf0)), "a source or its guard was written"
    assert torch.equal(_bits(tbuf)[~tmask], _bits(tbuf0)[~tmask]), "a sentinel around a target was written"
    if rho != 0.0:
        assert not torch.equal(tbuf[tmask], tbuf0[tmask]), "the update changed nothing"


def test_ema_gate_fires_on_the_due_iterations_only(gpu_device):
    from damc import schedule

    gen = torch.Generator().manual_seed(99)
    specs = [(5, 0, 0), (2 * CHUNK + 7, 0, 0), (CHUNK + 5, 1, 1)]
    tv, sv, (tbuf, tmask), (sbuf, _) = _carve(specs, gpu_device, gen)
    rho = 0.005
    ema = schedule.EmaTarget(sv, tv, rho=rho, period=10, phase=1)
    clock = schedule.TrainClock(gpu_device)
    sbuf0 = sbuf.clone()
    fired = []
    for it in range(22):
        before = tbuf.clone()
        want = [rho * p + (1 - rho) * t for p, t in zip(sv, tv)]
        ema.update(clock)
        torch.cuda.synchronize()
        if torch.equal(_bits(tbuf), _bits(before)):
            pass  # bitwise untouched, guards included
        else:
            fired.append(it)
            for t, w in zip(tv, want):
                assert torch.equal(_bits(t), _bits(w))
            assert torch.equal(_bits(tbuf)[~tmask], _bits(before)[~tmask])
        assert clock.read() == it
        clock.advance()
    assert fired == [9, 19]
    assert clock.read() == 22
    assert torch.equal(_bits(sbuf), _bits(sbuf0))


LR_START = [2e-4, 1.02e-5, 1e-5]  # decays; reaches the floor; already there


def _lr_optimizer(device, lrs):
    from damc import optim as dopt

    groups = [dict(params=[torch.nn.Parameter(torch.zeros(4, device=device))], lr=lr) for lr in lrs]
    return dopt.Adam(groups, betas=(0.5, 0.999), capturable=True)


def _assert_lrs(decay, opt, py):
    assert decay.values() == py  # the doubles, exactly
    for g, v in zip(opt.param_groups, py):
        lr = g["lr"]
        assert lr.dim() == 0 and lr.dtype == torch.float32 and lr.is_cuda
        assert torch.equal(_bits(lr.cpu()), _bits(torch.tensor(v, dtype=torch.float32)))


def test_lr_decay_is_the_python_chain(gpu_device):
    from damc import schedule

    opt = _lr_optimizer(gpu_device, LR_START)
    decay = schedule.LrDecay(opt, factor=0.99, floor=1e-5, period=3, phase=1)
    clock = schedule.TrainClock(gpu_device)
    py = list(LR_START)
    _assert_lrs(decay, opt, py)
    for it in range(40):
        decay.step(clock)
        clock.advance()
        if (it + 1) % 3 == 0:
            py = [max(v * 0.99, 1e-5) for v in py]
        _assert_lrs(decay, opt, py)
    assert py[0] < 2e-4 * 0.99 ** 12 and py[0] > 1e-5 and py[1] == 1e-5 and py[2] == 1e-5
    # the state round-trips through plain Python values, into the same tensors
    sd = decay.state_dict()
    ptrs = [g["lr"].data_ptr() for g in opt.param_groups]
    decay.load_state_dict({**sd, "lr": LR_START})
    _assert_lrs(decay, opt, LR_START)
    decay.load_state_dict(sd)
    _assert_lrs(decay, opt, py)
    assert ptrs == [g["lr"].data_ptr() for g in opt.param_groups]


def test_lr_decay_over_more_than_eight_groups(gpu_device):
    from damc import schedule

    lrs = [1e-4 * (i + 1) for i in range(10)]  # two launches: 8 + 2
    opt = _lr_optimizer(gpu_device, lrs)
    decay = schedule.LrDecay(opt, factor=0.99, floor=1e-5, period=1, phase=0)
    decay.step(None)  # no clock: always
    decay.step(schedule.TrainClock(gpu_device, iteration=7))
    _assert_lrs(decay, opt, [max(max(v * 0.99, 1e-5) * 0.99, 1e-5) for v in lrs])


def test_clock_set_is_eager_only_and_wraps(gpu_device, monkeypatch):
    from damc import _lib, schedule

    clock = schedule.TrainClock(gpu_device, iteration=2 ** 64 - 1)
    assert clock.read() == 2 ** 64 - 1
    clock.advance(3)
    assert clock.read() == 2
    clock.set(41)
    clock.advance()
    assert clock.read() == 42
    # set() writes a host value, which a capture would fix: refused while the stream is capturing (the flag it reads
    # is patched; no capture is started for a call that must not be recorded)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.DamcError, match="capture"):
        clock.set(3)
    opt = _lr_optimizer(gpu_device, LR_START)
    decay = schedule.LrDecay(opt)
    with pytest.raises(_lib.DamcError, match="capture"):
        decay.state_dict()
    with pytest.raises(_lib.DamcError, match="capture"):
        decay.load_state_dict({})
    monkeypatch.undo()
    assert clock.read() == 42


def test_glue_replays_from_one_graph(gpu_device):
    """EmaTarget.update(clock), LrDecay.step(clock), clock.advance() recorded once; the source is rewritten in place
    before every replay.  25 replays equal the host-gated loop (the torch expression, the Python chain) bitwise."""
    from damc import graphs, schedule

    N, rho = 25, 0.005
    gen = torch.Generator().manual_seed(7)
    specs = [(5, 0, 0), (2 * CHUNK + 7, 0, 0), (CHUNK + 5, 1, 1), (3, 0, 1)]
    tv, sv, (tbuf, tmask), (sbuf, smask) = _carve(specs, gpu_device, gen)
    feeds = [[torch.randn(n, generator=gen).to(gpu_device) for n, _, _ in specs] for _ in range(N)]
    tbuf0 = tbuf.clone()

    # the host-gated loop, on copies
    t_ref = [t.clone() for t in tv]
    py = list(LR_START)
    for it in range(N):
        p_now = feeds[it]
        if (it + 1) % 3 == 0:
            py = [max(v * 0.99, 1e-5) for v in py]
        if (it + 1) % 10 == 0:
            t_ref = [rho * p + (1 - rho) * t for p, t in zip(p_now, t_ref)]

    opt = _lr_optimizer(gpu_device, LR_START)
    ema = schedule.EmaTarget(sv, tv, rho=rho, period=10, phase=1)
    decay = schedule.LrDecay(opt, factor=0.99, floor=1e-5, period=3, phase=1)
    clock = schedule.TrainClock(gpu_device)
    start = decay.state_dict()

    def body():
        ema.update(clock)
        decay.step(clock)
        clock.advance()

    graph = graphs.capture(body)  # the warm-up ran the body once for real: put the state back, in place
    clock.set(0)
    tbuf.copy_(tbuf0)
    decay.load_state_dict(start)
    for it in range(N):
        for s, new in zip(sv, feeds[it]):
            s.copy_(new)
        graph.replay()
    torch.cuda.synchronize()
    assert clock.read() == N
    for i, (t, w) in enumerate(zip(tv, t_ref)):
        assert torch.equal(_bits(t), _bits(w)), "target %d" % i
    assert torch.equal(_bits(tbuf)[~tmask], _bits(tbuf0)[~tmask])
    assert not torch.equal(_bits(tbuf)[tmask], _bits(tbuf0)[tmask])
    _assert_lrs(decay, opt, py)
