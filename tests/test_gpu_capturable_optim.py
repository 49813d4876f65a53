"""GPU: damc.optim.Adam / AdamW(capturable=True) -- the step count on the device, read by damc_adam_step_capturable.

Shapes, hyper-parameter sets and tolerances are tests/test_gpu_optim.py's: STEP_TOL = 5e-7 (max abs difference over the
reference's max abs) for parameters and moments against torch.optim.Adam/AdamW(capturable=True) and against the
non-capturable damc.optim; the clip norm and clipped gradients within 1e-6.  Bitwise equality with the non-capturable
form is not asked: the bias corrections come from the device's pow there and from the host's here.  The captured step IS
asked to be bitwise: a graph of clip_and_step replayed 5 times equals the same optimiser stepped eagerly 5 times."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 512, 4, 4), (512,), (3,), (5, 7), (8193,), (256, 3, 3, 3)]
STEP_TOL = 5e-7
KINDS = [
    ("adam", dict(lr=2e-4, betas=(0.5, 0.999))),                       # G / E optimiser
    ("adamw", dict(lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-4)),   # Q optimiser
    ("adam", dict(lr=1e-3, weight_decay=1e-2)),                         # L2 form, default betas (lerp w < 0.5)
]
_GRADS = {}


def _params(device, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(device)) for s in SHAPES]


def _grads(device, step, scale=1.0):
    """The gradient set of a step, drawn once and shared by every test."""
    key = (step, scale)
    if key not in _GRADS:
        g = torch.Generator().manual_seed(100 + step)
        _GRADS[key] = [(torch.randn(s, generator=g) * scale).to(device) for s in SHAPES]
    return _GRADS[key]


def _set_grads(params, step, scale=1.0):
    for p, g in zip(params, _grads(params[0].device, step, scale)):
        p.grad = g.clone()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _classes(kind):
    from damc import optim as dopt

    return (torch.optim.Adam, dopt.Adam) if kind == "adam" else (torch.optim.AdamW, dopt.AdamW)


def _check_against(mine, do, ref, to, tol=STEP_TOL, steps=6.0):
    torch.cuda.synchronize()
    for a, b in zip(mine, ref):
        sa, sb = do.state[a], to.state[b]
        ra, rm, rv = _rel(a.detach(), b.detach()), _rel(sa["exp_avg"], sb["exp_avg"]), _rel(sa["exp_avg_sq"],
                                                                                           sb["exp_avg_sq"])
        print("capturable step: param %.2e exp_avg %.2e exp_avg_sq %.2e (tol %.0e)" % (ra, rm, rv, tol))
        assert ra < tol and rm < tol and rv < tol
        assert float(sa["step"]) == float(sb["step"]) == steps


@pytest.mark.parametrize("kind,kw", KINDS)
def test_capturable_step_matches_torch_and_the_host_form(gpu_device, kind, kw):
    tcls, dcls = _classes(kind)
    ref = _params(gpu_device)
    host = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    to, ho, do = tcls(ref, capturable=True, **kw), dcls(host, **kw), dcls(mine, capturable=True, **kw)
    for step in range(6):
        for ps in (ref, host, mine):
            _set_grads(ps, step)
        to.step()
        ho.step()
        do.step()
    _check_against(mine, do, ref, to)
    _check_against(mine, do, host, ho)
    # torch's capturable state format: a 0-d fp32 tensor on the parameter's device, one shared by the group here
    steps = [do.state[p]["step"] for p in mine]
    assert all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float32 for t in steps)
    assert all(t is steps[0] for t in steps)


def test_tensor_lr_is_read_by_the_kernel(gpu_device):
    """lr as a 0-d device tensor against torch's capturable AdamW with the same tensor lr; changing the tensor in
    place changes the next step, with nothing rebuilt."""
    from damc import optim as dopt

    kw = dict(betas=(0.5, 0.999), weight_decay=1e-4, capturable=True)
    ref = _params(gpu_device)
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    lr_t, lr_d = torch.tensor(3e-4, device=gpu_device), torch.tensor(3e-4, device=gpu_device)
    to, do = torch.optim.AdamW(ref, lr=lr_t, **kw), dopt.AdamW(mine, lr=lr_d, **kw)
    for step in range(6):
        if step == 3:  # the reference driver's decay, as an in-place write
            lr_t.fill_(1e-4)
            lr_d.fill_(1e-4)
        _set_grads(ref, step)
        _set_grads(mine, step)
        to.step()
        do.step()
    _check_against(mine, do, ref, to)
    # and it is the float-lr optimiser that switched lr at the same step
    flt = [torch.nn.Parameter(p.detach().clone()) for p in _params(gpu_device)]
    fo = dopt.AdamW(flt, lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-4, capturable=True)
    for step in range(6):
        if step == 3:
            fo.param_groups[0]["lr"] = 1e-4
        _set_grads(flt, step)
        fo.step()
    _check_against(mine, do, flt, fo)


def test_capturable_clip_and_step_matches_torch_sequence(gpu_device):
    from damc import optim as dopt

    ref = _params(gpu_device, seed=3)
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    to = torch.optim.Adam(ref, lr=2e-4, betas=(0.5, 0.999), capturable=True)
    do = dopt.Adam(mine, lr=2e-4, betas=(0.5, 0.999), capturable=True)
    for step in range(5):
        _set_grads(ref, step, scale=0.5)
        _set_grads(mine, step, scale=0.5)
        tn = torch.nn.utils.clip_grad_norm_(ref, 10.0)
        to.step()
        dn = do.clip_and_step(10.0)
        assert dn.is_cuda and dn.dim() == 0
        torch.cuda.synchronize()
        assert abs(float(dn) - float(tn)) / float(tn) < 1e-6
        for a, b in zip(mine, ref):
            assert _rel(a.grad, b.grad) < 1e-6  # gradients left scaled, as clip_grad_norm_ leaves them
    for a, b in zip(mine, ref):
        assert _rel(a.detach(), b.detach()) < 2e-6


def test_state_dict_round_trips_in_both_directions(gpu_device):
    """torch capturable -> damc capturable -> torch capturable, and non-capturable (CPU step) <-> capturable (device
    step): every hop continues as the optimiser that never stopped."""
    from damc import optim as dopt

    kw = dict(lr=2e-4, betas=(0.5, 0.999))
    ref = _params(gpu_device, seed=5)
    to = torch.optim.Adam(ref, capturable=True, **kw)
    for step in range(3):
        _set_grads(ref, step)
        to.step()
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    do = dopt.Adam(mine, capturable=True, **kw)
    do.load_state_dict(copy.deepcopy(to.state_dict()))
    # a non-capturable damc optimiser loads the same capturable state: step lands on the CPU, the flag stays its own
    host = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    ho = dopt.Adam(host, **kw)
    ho.load_state_dict(copy.deepcopy(to.state_dict()))
    assert ho.param_groups[0]["capturable"] is False
    assert all(ho.state[p]["step"].device.type == "cpu" for p in host)
    # ... and a capturable one loads a non-capturable state: step moves to the device
    back = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    bo = dopt.Adam(back, capturable=True, **kw)
    bo.load_state_dict(copy.deepcopy(ho.state_dict()))  # load_state_dict may alias the tensors it is given
    assert bo.param_groups[0]["capturable"] is True
    assert all(bo.state[p]["step"].is_cuda and float(bo.state[p]["step"]) == 3.0 for p in back)
    assert len({id(bo.state[p]["step"]) for p in back}) == 1  # equal counts: one shared device counter
    for step in range(3, 5):
        for ps in (ref, mine, host, back):
            _set_grads(ps, step)
        to.step()
        do.step()
        ho.step()
        bo.step()
    _check_against(mine, do, ref, to, steps=5.0)
    _check_against(back, bo, ref, to, steps=5.0)
    _check_against(host, ho, ref, to, steps=5.0)
    # back into torch's capturable optimiser: private per-parameter device counters, and it keeps stepping
    t2p = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    t2 = torch.optim.Adam(t2p, capturable=True, **kw)
    t2.load_state_dict(copy.deepcopy(do.state_dict()))
    assert [float(t2.state[p]["step"]) for p in t2p] == [5.0] * len(t2p)
    _set_grads(ref, 5)
    _set_grads(t2p, 5)
    to.step()
    t2.step()
    torch.cuda.synchronize()
    assert [float(t2.state[p]["step"]) for p in t2p] == [6.0] * len(t2p)
    for a, b in zip(t2p, ref):
        assert _rel(a.detach(), b.detach()) < STEP_TOL


def test_partial_gradients_keep_per_parameter_counts(gpu_device):
    """A step in which every other parameter has no gradient: the idle ones keep their count (their shared counter is
    cloned for the ones that step), as torch's capturable AdamW counts."""
    from damc import optim as dopt

    kw = dict(lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-4, capturable=True)
    ref = _params(gpu_device)
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    to, do = torch.optim.AdamW(ref, **kw), dopt.AdamW(mine, **kw)
    for step in range(5):
        _set_grads(ref, step)
        _set_grads(mine, step)
        if step == 2:
            for i in range(0, len(ref), 2):
                ref[i].grad = None
                mine[i].grad = None
        to.step()
        do.step()
    torch.cuda.synchronize()
    for a, b in zip(mine, ref):
        assert float(do.state[a]["step"]) == float(to.state[b]["step"])
        assert _rel(a.detach(), b.detach()) < STEP_TOL


def test_more_tensors_than_one_launch_advance_the_count_once(gpu_device):
    """130 parameters (two <= 96-tensor slices per step): the shared count advances once per step, not per slice."""
    from damc import optim as dopt

    g = torch.Generator().manual_seed(11)
    sizes = [int(n) for n in torch.randint(1, 3000, (130,), generator=g)]
    ref = [torch.nn.Parameter(torch.randn(n, generator=g).to(gpu_device)) for n in sizes]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    kw = dict(lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-4, capturable=True)
    to, do = torch.optim.AdamW(ref, **kw), dopt.AdamW(mine, **kw)
    for step in range(3):
        gs = torch.Generator().manual_seed(100 + step)
        for a, b in zip(ref, mine):
            a.grad = torch.randn(a.shape, generator=gs).to(gpu_device)
            b.grad = a.grad.clone()
        to.step()
        do.clip_and_step(1e9)  # clip factor 1: the step alone
    torch.cuda.synchronize()
    assert float(do.state[mine[0]]["step"]) == float(do.state[mine[-1]]["step"]) == 3.0
    for a, b in zip(mine, ref):
        assert _rel(a.detach(), b.detach()) < 2e-6


def test_captured_clip_and_step_replays_bitwise(gpu_device):
    """clip_and_step recorded once and replayed 5 times, the gradients rewritten in place between replays, against the
    same optimiser stepped eagerly 5 times: parameters, moments, step and the returned norm, bit for bit."""
    from damc import graphs
    from damc import optim as dopt

    kw = dict(lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-4, capturable=True)
    eager = _params(gpu_device, seed=9)
    eo = dopt.AdamW(eager, **kw)
    norms = []
    for step in range(5):
        _set_grads(eager, step, scale=0.5)
        norms.append(eo.clip_and_step(1.0).clone())
    torch.cuda.synchronize()

    cap = _params(gpu_device, seed=9)
    co = dopt.AdamW(cap, **kw)
    _set_grads(cap, 0, scale=0.5)
    out = {}

    def body():
        out["norm"] = co.clip_and_step(1.0)

    start = [p.detach().clone() for p in cap]
    graph = graphs.capture(body)
    # the warm-up stepped once for real: parameters, moments and the count go back, in place
    with torch.no_grad():
        for p, s in zip(cap, start):
            p.copy_(s)
            co.state[p]["exp_avg"].zero_()
            co.state[p]["exp_avg_sq"].zero_()
        co.state[cap[0]]["step"].zero_()
    for step in range(5):
        with torch.no_grad():
            for p, g in zip(cap, _grads(gpu_device, step, 0.5)):
                p.grad.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["norm"], norms[step])
    for a, b in zip(cap, eager):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(co.state[a]["exp_avg"], eo.state[b]["exp_avg"])
        assert torch.equal(co.state[a]["exp_avg_sq"], eo.state[b]["exp_avg_sq"])
        assert torch.equal(a.grad, b.grad)  # left clipped, as the eager call leaves them
    assert float(co.state[cap[0]]["step"]) == float(eo.state[eager[0]]["step"]) == 5.0


def test_sharded_step_takes_a_capturable_optimiser(gpu_device):
    """dist.sharded_step (world of 1: pack, attach, clip_and_step) with a capturable optimiser, eager, against the
    non-capturable one."""
    from damc import dist
    from damc import optim as dopt

    kw = dict(lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-4)
    a = _params(gpu_device, seed=4)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ao, bo = dopt.AdamW(a, **kw), dopt.AdamW(b, capturable=True, **kw)
    for step in range(3):
        _set_grads(a, step)
        _set_grads(b, step)
        na = dist.sharded_step(ao, 8, 8, max_norm=1.0)
        nb = dist.sharded_step(bo, 8, 8, max_norm=1.0)
        assert torch.equal(na, nb)
    torch.cuda.synchronize()
    for p, q in zip(b, a):
        assert _rel(p.detach(), q.detach()) < STEP_TOL
    assert float(bo.state[b[0]]["step"]) == 3.0
