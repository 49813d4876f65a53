"""GPU: data-parallel training pieces -- the seeded Q update's Philox draws (damc_philox_uniform,
damc_q_noise_glue_seeded, Q.calculate_loss(seed=...)), the gradient bucket (damc_grad_pack, damc.dist.GradBucket) and
damc.dist.sharded_step, on one GPU: shards of a batch in one process, and two real ranks over gloo."""
import copy
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dp_util
from conftest import REPO, build_q_case
from dp_util import PACK_SIZES, guarded, guards_intact
from toyq_util import build_toy_case

pytestmark = pytest.mark.gpu

KEYS = [(1, 0, 0), (0x0123456789ABCDEF, 5, 7), (42, 2 ** 32 + 3, 1), (42, 3, 2 ** 32 + 1),
        (2 ** 62 - 1, 2 ** 40 + 17, 2 ** 33 + 5)]  # (seed, chain_base, step_offset): high words of each mixed in


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------- 1. uniform stream
@pytest.mark.parametrize("seed,chain_base,step_offset", KEYS)
def test_philox_uniform_is_the_numpy_philox(gpu_device, seed, chain_base, step_offset):
    from damc import _lib, langevin

    n_steps, B = 3, 37
    for sid in (_lib.STREAM_QU, _lib.STREAM_POSTERIOR):
        got = _np(langevin.philox_uniform(n_steps, B, seed, gpu_device, step_offset=step_offset,
                                          chain_base=chain_base, stream_id=sid))
        want = dp_util.philox_uniform(n_steps, B, seed, step_offset, chain_base, sid)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert (got >= 0).all() and (got < 1).all()
        assert np.array_equal(got * 2.0 ** 24, np.floor(got * 2.0 ** 24))  # on the 2^-24 grid
    # rows [a, a + c) drawn with chain_base + a are the slice of the whole draw
    a, c = 11, 9
    whole = langevin.philox_uniform(n_steps, B, seed, gpu_device, step_offset=step_offset, chain_base=chain_base)
    part = langevin.philox_uniform(n_steps, c, seed, gpu_device, step_offset=step_offset, chain_base=chain_base + a)
    assert torch.equal(part, whole[:, a:a + c])


# ------------------------------------------------------------------------------------------- 2. seeded glue
def _fake_q(ntemb, lmin=-5.1, lmax=9.8):
    return types.SimpleNamespace(logsnr_min=lmin, logsnr_max=lmax, p=types.SimpleNamespace(ntemb=ntemb))


def _seeded_glue_guarded(z, ntemb, seed, draw_index, chain_base, lmin=-5.1, lmax=9.8):
    """damc_q_noise_glue_seeded into guarded buffers: (u, eps, logsnr, zt, temb) views and the whole buffers."""
    from damc import _lib, training

    B, nz = z.shape
    dev = z.device
    bufs = [guarded(n, dev) for n in (B, B * nz, B, B * nz, B * ntemb)]
    u, eps, lg, zt, se = (v for _, v in bufs)
    p = _lib.ptr
    _lib.check(_lib.lib().damc_q_noise_glue_seeded(p(z), B, nz, lmin, lmax, p(training._freqs(ntemb // 2, dev)), ntemb,
                                                   seed, draw_index, chain_base, p(u), p(eps), p(lg), p(zt), p(se),
                                                   _lib.stream_ptr(dev)), "damc_q_noise_glue_seeded")
    torch.cuda.synchronize()
    return (u, eps.view(B, nz), lg, zt.view(B, nz), se.view(B, ntemb)), [w for w, _ in bufs]


@pytest.mark.parametrize("B,nz,ntemb", [(1, 2, 128), (5, 6, 128), (21, 128, 128), (16, 100, 64)])
def test_seeded_glue_is_the_injected_glue(gpu_device, B, nz, ntemb):
    from damc import _lib, langevin, synth, training

    seed, k, base = 0x1F2E3D4C5B6A7988, 2 ** 32 + 9, 2 ** 32 + 1000
    z = torch.from_numpy(synth.normal_f32(71, B, (B, nz))).to(gpu_device)
    (u, eps, lg, zt, se), wholes = _seeded_glue_guarded(z, ntemb, seed, k, base)
    assert all(guards_intact(w) for w in wholes)
    # the draws are the library's own streams on the same key
    assert torch.equal(u, langevin.philox_uniform(1, B, seed, gpu_device, step_offset=k, chain_base=base)[0])
    assert torch.equal(eps, langevin.philox_normal(1, B, nz, seed, gpu_device, step_offset=k, chain_base=base,
                                                   stream_id=_lib.STREAM_QEPS)[0])
    # and everything after them is damc_q_noise_glue fed those draws
    lg_ref = torch.empty(B, device=gpu_device)
    zt_ref, se_ref = training.q_noise_glue(_fake_q(ntemb), u.clone(), z, eps.clone(), logsnr_out=lg_ref)
    assert torch.equal(zt, zt_ref) and torch.equal(se, se_ref) and torch.equal(lg, lg_ref)
    assert torch.isfinite(zt).all() and torch.isfinite(se).all()
    # the Python entry point gives the same tensors, with u and logsnr left out (NULL)
    zt2, se2, eps2 = training.q_noise_glue_seeded(_fake_q(ntemb), z, seed, k, base)
    assert torch.equal(zt2, zt) and torch.equal(se2, se) and torch.equal(eps2, eps)


def test_seeded_glue_shards_are_the_whole_batch_rows(gpu_device):
    from damc import synth

    B, nz, ntemb, seed, k = 21, 128, 128, 77, 3
    z = torch.from_numpy(synth.normal_f32(71, 0, (B, nz))).to(gpu_device)
    whole, _ = _seeded_glue_guarded(z, ntemb, seed, k, 0)
    for lo, hi in ((0, 5), (5, 21)):
        part, guards = _seeded_glue_guarded(z[lo:hi].contiguous(), ntemb, seed, k, lo)
        assert all(guards_intact(w) for w in guards)
        for a, b in zip(part, whole):
            assert torch.equal(a, b[lo:hi])


# ------------------------------------------------------------------------------------- 3. seeded calculate_loss
class _materialised:
    """torch.randn / rand / randn_like return the given device tensors, in calculate_loss's order (as
    conftest.qtrain_run patches them); `dtype` converts (the fp64 evaluation)."""

    def __init__(self, pe, u, eps, dtype=torch.float32, device=None):
        self.pe, self.u, self.eps, self.dtype, self.device = pe, u, eps, dtype, device

    def __enter__(self):
        self.orig = torch.randn, torch.rand, torch.randn_like
        dev = self.device
        torch.randn = lambda *a, **k: self.pe.clone().to(device=dev or k.get("device") or "cpu", dtype=self.dtype)
        torch.rand = lambda *a, **k: self.u.clone().to(device="cpu", dtype=self.dtype)
        torch.randn_like = lambda t, **k: self.eps.clone().to(device=t.device, dtype=self.dtype)

    def __exit__(self, *exc):
        torch.randn, torch.rand, torch.randn_like = self.orig


def _q_streams(Q, B, seed, k, base, device):
    from damc import _lib, langevin

    pe = langevin.philox_normal(1, B, Q.nz, seed, device, step_offset=k, chain_base=base, stream_id=_lib.STREAM_QPE)[0]
    u = langevin.philox_uniform(1, B, seed, device, step_offset=k, chain_base=base)[0]
    eps = langevin.philox_normal(1, B, Q.nz, seed, device, step_offset=k, chain_base=base,
                                 stream_id=_lib.STREAM_QEPS)[0]
    return pe, u, eps


def _mixed_mask(B, device):
    mask = torch.ones(B, 1, device=device)
    mask[1::3] = 0.0
    return mask


def _loss_and_grads(Q, **kw):
    for p in Q.parameters():
        p.grad = None
    loss = Q.calculate_loss(**kw)
    loss.mean().backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in Q.parameters()]


@pytest.mark.parametrize("which", ["q_cifar10_s", "q_toy"])
def test_seeded_calculate_loss_is_the_unseeded_one_on_the_materialised_streams(gpu_device, which):
    from damc import synth

    c = build_q_case(which, gpu_device) if which != "q_toy" else build_toy_case(which, gpu_device)
    Q, x = c["Q"].train(), c["x"]
    B = x.shape[0]
    z = torch.from_numpy(synth.normal_f32(2, 0, (B, Q.nz))).to(gpu_device)
    mask = _mixed_mask(B, gpu_device)
    seed, k, base = 0x2545F4914F6CDD1D, 6, 40
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(gpu_device)
    loss_s, grads_s = _loss_and_grads(Q, x=x, z=z, mask=mask, seed=seed, draw_index=k, chain_base=base)
    assert torch.equal(torch.get_rng_state(), cpu_state)
    assert torch.equal(torch.cuda.get_rng_state(gpu_device), dev_state)
    pe, u, eps = _q_streams(Q, B, seed, k, base, gpu_device)
    with _materialised(pe, u, eps):
        loss_u, grads_u = _loss_and_grads(Q, x=x, z=z, mask=mask)
    assert torch.isfinite(loss_s).all() and torch.equal(loss_s, loss_u)
    assert sum(g is not None for g in grads_s) > 10
    for (n, _), a, b in zip(Q.named_parameters(), grads_s, grads_u):
        assert (a is None) == (b is None), n
        assert a is None or torch.equal(a, b), n
    # another draw_index is another draw; the same one repeats
    loss_k1, _ = _loss_and_grads(Q, x=x, z=z, mask=mask, seed=seed, draw_index=k + 1, chain_base=base)
    loss_again, _ = _loss_and_grads(Q, x=x, z=z, mask=mask, seed=seed, draw_index=k, chain_base=base)
    assert not torch.equal(loss_k1, loss_s) and torch.equal(loss_again, loss_s)
    # x None: every row takes the prior embedding
    loss_p, _ = _loss_and_grads(Q, z=z, seed=seed, draw_index=k, chain_base=base)
    with _materialised(pe, u, eps):
        loss_pu, _ = _loss_and_grads(Q, z=z)
    assert torch.equal(loss_p, loss_pu)


def test_seeded_calculate_loss_has_no_fallback(gpu_device):
    from damc import _lib, training

    c = build_toy_case("q_toy", gpu_device)
    Q, x = c["Q"].train(), c["x"]
    z = torch.zeros(x.shape[0], Q.nz, device=gpu_device)
    with training.stock_pytorch(), pytest.raises(_lib.DamcError):
        Q.calculate_loss(x=x, z=z, seed=1)
    prev, training.Q_GLUE = training.Q_GLUE, False
    try:
        with pytest.raises(_lib.DamcError):
            Q.calculate_loss(x=x, z=z, seed=1)
    finally:
        training.Q_GLUE = prev
    supported = training.denoiser_train_supported
    training.denoiser_train_supported = lambda p: False
    try:
        with pytest.raises(_lib.DamcError):
            Q.calculate_loss(x=x, z=z, seed=1)
    finally:
        training.denoiser_train_supported = supported


# ------------------------------------------------------------------------------------------------ 4. pack
def _pack_inputs(sizes, device, null_at, misaligned_at):
    from damc import synth

    grads = []
    for t, n in enumerate(sizes):
        if t == null_at:
            grads.append(None)
            continue
        lead = 1 if t == misaligned_at else 0
        g = torch.from_numpy(synth.normal_f32(61, t, (n + lead,))).to(device)[lead:]
        assert g.is_contiguous() and (g.data_ptr() % 16 == 4) == bool(lead)
        grads.append(g)
    return grads


@pytest.mark.parametrize("scale", [1.0, 5.0 / 21.0])
def test_grad_pack_is_bitwise_g_times_scale(gpu_device, scale):
    from damc import dist

    sizes = PACK_SIZES + [40000]
    grads = _pack_inputs(sizes, gpu_device, null_at=2, misaligned_at=5)  # sizes 4 (NULL) and 8192 (scalar path)
    offs, total = dist.bucket_layout(sizes)
    whole, bucket = guarded(total, gpu_device, fill=0.0)
    bucket[offs[2]:offs[2] + sizes[2]] = 7.0  # the NULL tensor's slice must be overwritten with zeros
    dist.grad_pack(grads, sizes, offs, bucket, scale)
    torch.cuda.synchronize()
    first = bucket.clone()
    assert guards_intact(whole)
    covered = torch.zeros(total, dtype=torch.bool, device=gpu_device)
    for g, o, n in zip(grads, offs, sizes):
        want = torch.zeros(n, device=gpu_device) if g is None else g * scale
        assert torch.equal(bucket[o:o + n], want), n
        covered[o:o + n] = True
    assert bool((bucket[~covered] == 0).all()) and int((~covered).sum()) == total - sum(sizes)
    dist.grad_pack(grads, sizes, offs, bucket, scale)
    assert torch.equal(bucket, first) and guards_intact(whole)
    with pytest.raises(Exception):
        dist.grad_pack(grads, sizes, [o + 4 for o in offs], bucket, scale)  # the last slice would leave the bucket


def test_grad_bucket_packs_200_tensors_in_slices(gpu_device):
    from damc import dist, synth

    sizes = dp_util.many_sizes(200)
    params = [torch.nn.Parameter(torch.zeros(n, device=gpu_device)) for n in sizes]
    no_grad = {3, 150}
    for t, p in enumerate(params):
        if t not in no_grad:
            p.grad = torch.from_numpy(synth.normal_f32(62, t, (sizes[t],))).to(gpu_device)
    grads = [None if p.grad is None else p.grad.clone() for p in params]
    bucket = dist.GradBucket(params)
    scale = 16.0 / 21.0
    buf = bucket.pack(scale)
    lay = bucket.layout
    assert lay.index == tuple(t for t in range(200) if t not in no_grad)
    assert list(lay.offsets) == dist.bucket_layout([sizes[t] for t in lay.index])[0]
    covered = torch.zeros_like(buf, dtype=torch.bool)
    for t, o, n in zip(lay.index, lay.offsets, lay.numels):
        assert torch.equal(buf[o:o + n], grads[t] * scale), t
        covered[o:o + n] = True
    assert bool((buf[~covered] == 0).all())
    bucket.attach()
    for t, p in enumerate(params):
        if t in no_grad:
            assert p.grad is None
        else:
            assert p.grad.data_ptr() % 16 == 0 and p.grad.shape == p.shape
            assert p.grad.data_ptr() == buf.data_ptr() + 4 * lay.offsets[lay.index.index(t)]
            assert torch.equal(p.grad, grads[t] * scale)
    assert bucket.pack(1.0).data_ptr() == buf.data_ptr()  # the same set of gradients: the cached buffer, in place


# ------------------------------------------------------------------- 5. simulated two-rank update, one process
B_DP, SHARDS, MAX_NORM = 21, ((0, 5), (5, 21)), 1.0


class _ECase:
    """E update (train_gen_recon.py:233-241): e_pos.mean() - e_neg.mean() over B positive and 2B negative latents."""
    name = "E"

    def __init__(self):
        from damc import synth

        self.zp = torch.from_numpy(synth.normal_f32(81, 0, (B_DP, 128)))
        self.zn = torch.from_numpy(synth.normal_f32(81, 1, (2 * B_DP, 128)))

    def net(self):
        from damc import synth
        from src import diffusion_net as dn

        return synth.load_into(dn._netE(nz=128), 10).train()

    def opt(self, net):
        from damc import optim

        return optim.Adam(net.parameters(), lr=2e-4, betas=(0.5, 0.999))

    def loss(self, net, lo, hi, it, like):
        zp, zn = self.zp[lo:hi].to(like), self.zn[2 * lo:2 * hi].to(like)
        return net(zp).mean() - net(zn).mean()

    loss64 = loss


class _GCase(_ECase):
    """G update (train_gen_recon.py:222-231): sum((G(z) - x)^2, [1, 2, 3]).mean() on cifar10_w16's generator."""
    name = "G"

    def __init__(self):
        from damc import synth

        self.z = torch.from_numpy(synth.normal_f32(2, 3, (B_DP, 128)))
        self.x = torch.from_numpy(synth.uniform_f32(1, 3, (B_DP, 3, 32, 32)))

    def net(self):
        from damc import synth
        from src import diffusion_net as dn

        return synth.load_into(dn._netG_cifar10(nz=128, ngf=16, nc=3), 0).train()

    def loss(self, net, lo, hi, it, like):
        z, x = self.z[lo:hi].to(like), self.x[lo:hi].to(like)
        return torch.sum((net(z) - x) ** 2, dim=[1, 2, 3]).mean()

    loss64 = loss


class _QCase(_ECase):
    """Seeded Q update (train_gen_recon.py:211-220) on q_cifar10_s with a mixed mask: every replica passes the same
    seed and draw_index = the iteration, and chain_base = its first row."""
    name = "Q"

    def __init__(self):
        from damc import dist, synth

        self.x = torch.from_numpy(synth.uniform_f32(1, 5, (B_DP, 3, 32, 32)))
        self.z = torch.from_numpy(synth.normal_f32(2, 5, (B_DP, 128)))
        self.mask = _mixed_mask(B_DP, "cpu")
        self.seeds = [dist.iteration_seed(1234, it, 3) for it in range(2)]

    def net(self):
        return copy.deepcopy(build_q_case("q_cifar10_s", "cpu")["Q"]).train()

    def opt(self, net):
        from damc import optim

        return optim.AdamW(net.parameters(), lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-4)

    def loss(self, net, lo, hi, it, like):
        x, z, mask = (t[lo:hi].to(like) for t in (self.x, self.z, self.mask))
        return net.calculate_loss(x=x, z=z, mask=mask, seed=self.seeds[it], draw_index=it, chain_base=lo).mean()

    def loss64(self, net, lo, hi, it, like):
        """The stock modules on the same draws: the materialised streams of rows [lo, hi), as fp64."""
        dev = torch.device("cuda:0")
        pe, u, eps = _q_streams(net, hi - lo, self.seeds[it], it, lo, dev)
        x, z, mask = (t[lo:hi].to(like) for t in (self.x, self.z, self.mask))
        with _materialised(pe.cpu(), u.cpu(), eps.cpu(), dtype=like.dtype, device=like.device):
            return net.calculate_loss(x=x, z=z, mask=mask).mean()


def _grads_of(net):
    return [None if p.grad is None else p.grad.detach().clone() for p in net.parameters()]


@pytest.mark.parametrize("case_cls", [_ECase, _GCase, _QCase], ids=lambda c: c.name)
def test_two_shards_update_like_two_ranks(gpu_device, case_cls):
    """Replicas 0 and 1 take rows [0, 5) and [5, 21) of a B = 21 batch and reduce through their buckets (pack, torch.add
    of the two buffers, the sum copied into both, attach, clip_and_step); replica 2 takes the whole batch.

    The gradient criterion is the project's 3 x rule: per tensor, |sharded - fp64| <= 3 |whole batch - fp64|, fp64 on
    the stock modules, both distances relative to the fp64 gradient's norm floored at 1e-3 x the net's largest gradient
    norm (conftest.gtrain_check's floor, for gradients that are analytically zero).  Measured: the worst ratio is 0.80
    (E), 1.17 (G, gen.2.bias: 6.1e-8 against 5.3e-8) and 1.25 (Q, encoder.net.1.weight)."""
    from damc import dist, training

    case = case_cls()
    base = case.net()
    nets = [copy.deepcopy(base).to(gpu_device) for _ in range(3)]
    opts = [case.opt(n) for n in nets]
    like = torch.zeros((), device=gpu_device)
    buckets = [dist.GradBucket(list(n.parameters())) for n in nets[:2]]
    first = {}
    for it in range(2):
        raw, packed = [], []
        for r, (lo, hi) in enumerate(SHARDS):
            opts[r].zero_grad()
            case.loss(nets[r], lo, hi, it, like).backward()
            raw.append(_grads_of(nets[r]))
            packed.append(buckets[r].pack((hi - lo) / B_DP).clone())
        total = torch.add(packed[0], packed[1])
        lay = buckets[0].layout
        assert buckets[1].layout.index == lay.index and buckets[1].layout.offsets == lay.offsets
        # 1. the reduced bucket is g0 * s0 + g1 * s1 with every operation rounded on its own
        for t, o, n in zip(lay.index, lay.offsets, lay.numels):
            want = raw[0][t] * (5 / B_DP) + raw[1][t] * (16 / B_DP)
            assert torch.equal(total[o:o + n].view_as(want), want), (it, t)
        norms = []
        for r in range(2):
            buckets[r].buffer.copy_(total)
            buckets[r].attach()
            if it == 0 and r == 0:
                first["sharded"] = _grads_of(nets[0])
            norms.append(opts[r].clip_and_step(MAX_NORM))
        # 2. both replicas hold the same norm, parameters and optimiser state, bit for bit
        assert torch.equal(norms[0], norms[1]) and bool(torch.isfinite(norms[0]))
        for (n, p0), p1 in zip(nets[0].named_parameters(), nets[1].parameters()):
            assert torch.equal(p0, p1), (it, n)
            s0, s1 = opts[0].state.get(p0, {}), opts[1].state.get(p1, {})
            assert s0.keys() == s1.keys()
            for k in s0:
                assert torch.equal(s0[k], s1[k]), (it, n, k)
        opts[2].zero_grad()
        case.loss(nets[2], 0, B_DP, it, like).backward()
        if it == 0:
            first["whole"] = _grads_of(nets[2])
        opts[2].clip_and_step(MAX_NORM)
    # 3. the first iteration's reduced gradients against the whole batch's, both measured from fp64 on the stock modules
    net64 = copy.deepcopy(base).double()
    with training.stock_pytorch():
        case.loss64(net64, 0, B_DP, 0, torch.zeros((), dtype=torch.float64)).backward()
    g64 = [None if p.grad is None else p.grad.detach() for p in net64.parameters()]
    names = [n for n, _ in base.named_parameters()]
    assert [g is None for g in g64] == [g is None for g in first["whole"]] == [g is None for g in first["sharded"]]
    floor = 1e-3 * max(float(g.norm()) for g in g64 if g is not None)
    worst = (0.0, None)
    for n, r64, gw, gs in zip(names, g64, first["whole"], first["sharded"]):
        if r64 is None:
            continue
        den = max(float(r64.norm()), floor)
        e_w = float((gw.double().cpu() - r64).norm()) / den
        e_s = float((gs.double().cpu() - r64).norm()) / den
        print("%s %-34s |sharded - fp64| %.2e  |whole - fp64| %.2e" % (case.name, n, e_s, e_w))
        worst = max(worst, (e_s / max(e_w, 1e-30), n))
        assert e_s <= 3 * e_w, (n, e_s, e_w)
    print("%s worst ratio %.2f (%s)" % (case.name, worst[0], worst[1]))


# ---------------------------------------------------------------------- 6. two real ranks on one GPU over gloo
def test_two_ranks_on_one_gpu_over_gloo(gpu_device, tmp_path):
    """tests/dp_rank_worker.py twice, as fresh child processes: each rank's reduced bucket is the sum of the two
    pre-reduce buckets, and both ranks end with the same bucket and the same parameters."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = os.path.join(REPO, "tests", "dp_rank_worker.py")
    outs = [str(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), outs[r]], env=env, cwd=REPO,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        for r, p in enumerate(procs):  # a failed or overdue rank ends the test: the other one is not waited for
            try:
                log, _ = p.communicate(timeout=150)
            except subprocess.TimeoutExpired:
                pytest.fail("rank %d did not finish in 150 s" % r)
            assert p.returncode == 0, "rank %d exited %s:\n%s" % (r, p.returncode, log[-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    d = [np.load(o) for o in outs]
    assert [int(x["count"]) for x in d] == [3, 5]
    for it in range(2):
        b0, b1 = d[0]["before%d" % it], d[1]["before%d" % it]
        assert np.abs(b0).sum() > 0 and not np.array_equal(b0, b1)
        for x in d:
            assert np.array_equal(x["after%d" % it], b0 + b1), it  # fp32 add, each rank
        assert np.array_equal(d[0]["after%d" % it], d[1]["after%d" % it])
    assert np.array_equal(d[0]["norms"], d[1]["norms"]) and np.isfinite(d[0]["norms"]).all()
    keys = sorted(k for k in d[0].files if k.startswith("param"))
    assert len(keys) == 6
    for k in keys:
        assert np.array_equal(d[0][k], d[1][k]), k


# ------------------------------------------------------------------------------------------ 7. graph replay
def test_seeded_q_update_replays_from_a_captured_graph(gpu_device):
    """calculate_loss(seed=...).mean().backward() + GradBucket.pack at the toy driver's B = 500, recorded into a graph
    with (seed, draw_index) fixed: the replay's loss and bucket are bitwise the eager ones.  Nothing in the seeded
    update reads the host's generator, so no draw has to be handed over as a device tensor."""
    from damc import dist, synth

    seed, k, base, B = 0x51ED270B7F4A7C15, 4, 1000, 500

    def fresh():
        Q = build_toy_case("q_toy_driver", gpu_device)["Q"].train()
        x = torch.from_numpy(synth.uniform_f32(51, 0, (B, 2))).to(gpu_device)
        z = torch.from_numpy(synth.normal_f32(52, 0, (B, Q.nz))).to(gpu_device)
        mask = (torch.from_numpy(synth.uniform_f32(53, 0, (B, 1), 0.0, 1.0)) >= 0.1).float().to(gpu_device)
        return Q, dist.GradBucket(list(Q.parameters())), x, z, mask

    def update(Q, bucket, x, z, mask):
        for p in Q.parameters():
            p.grad = None
        loss = Q.calculate_loss(x=x, z=z, mask=mask, seed=seed, draw_index=k, chain_base=base).mean()
        loss.backward()
        return loss.detach(), bucket.pack(0.5)

    loss_e, buf_e = update(*fresh())
    torch.cuda.synchronize()
    loss_e, buf_e = loss_e.clone(), buf_e.clone()
    assert bool(torch.isfinite(loss_e)) and float(buf_e.abs().sum()) > 0

    args = fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            update(*args)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, buf_g = update(*args)
    for _ in range(2):
        buf_g.zero_()
        loss_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e), "loss differs between graph replay and eager"
        assert torch.equal(buf_g, buf_e), "bucket differs between graph replay and eager"
