"""Multi-GPU: one process per GPU (torchrun), chains sharded by GLOBAL index, RCCL only at the end.

The Langevin / reverse-sweep updates of different chains never interact (every term of U is a sum
over chains; InstanceNorm is per sample — SURVEY.md §8e), so a batch is split into contiguous
per-rank slices and each rank runs the HIP kernels on its slice with ``chain_base`` = the slice
start: Philox noise is keyed by the global chain index, so the union of the shards is bitwise the
1-GPU result.  The only collectives are the final reductions below (``all_reduce(SUM)`` over
RCCL/xGMI for backend "nccl", or gloo in the CPU tests):
  * reconstruction MSE (eval_gen_recon.py:177-212): [sum of per-sample MSE, count];
  * FID sufficient statistics (MCMC.py:130-176 feed pfw.fid): [sum f, sum f f^T, n] in fp64;
and, for the anomaly score, which is not a sum, one ``all_gather`` of fixed-size slices (``all_gather_shards``).

Data-parallel updates: each rank runs the G / Q / E update's forward and backward on its shard of the
batch (the seeded ``Q.calculate_loss`` keys its draws by the global row), ``GradBucket`` packs the net's gradients into
one flat buffer scaled by local / global batch, one ``all_reduce(SUM)`` sums the ranks' buffers, the gradients become
views of the buffer and the usual clip + Adam kernels run on those views (``sharded_step``).
"""
import ctypes

import torch


def shard(global_batch, rank, world):
    """Contiguous balanced slice of [0, global_batch): returns (start, count)."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError("bad rank/world %d/%d" % (rank, world))
    base, rem = divmod(int(global_batch), int(world))
    start = rank * base + min(rank, rem)
    return start, base + (1 if rank < rem else 0)


def block_plan(global_batch, rank, world, scaling="weak"):
    """Which chains one rank runs in a Langevin block (bench.py; train_gen_recon.py:203-209: posterior on B
    chains, prior on 2B = cat(z0, N(0, I)) chains), and the global index of its first chain of each kind.

    weak:   every rank runs a full batch of its own (B posterior + 2B prior chains); rank r's chains are
            global chains [r B, (r+1) B) and [2 r B, 2 (r+1) B) -> noise streams never collide.
    strong: the global batch is split: posterior rows shard(B) and prior rows shard(2B) of the global
            arrays; chain_base = the slice start, so the union over ranks is the 1-GPU block bit for bit.
    Returns dict(post_start, post_count, prior_start, prior_count, post_global, prior_global) — *_start are the
    chain_base values (and, for strong, the slice offsets into the global inputs); *_global the chain count of the
    block a rank's slice belongs to (what a shape-dependent engine choice must key on: langevin.prior_langevin's
    global_batch)."""
    B = int(global_batch)
    if scaling == "weak":
        return dict(post_start=rank * B, post_count=B, prior_start=rank * 2 * B, prior_count=2 * B,
                    post_global=B, prior_global=2 * B)
    if scaling == "strong":
        ps, pc = shard(B, rank, world)
        qs, qc = shard(2 * B, rank, world)
        return dict(post_start=ps, post_count=pc, prior_start=qs, prior_count=qc, post_global=B, prior_global=2 * B)
    raise ValueError("scaling must be 'weak' or 'strong', got %r" % (scaling,))


def _dist():
    import torch.distributed as d

    return d if d.is_available() and d.is_initialized() else None


def all_reduce_sum_(t, group=None):
    d = _dist()
    if d is not None and d.get_world_size(group) > 1:
        d.all_reduce(t, op=d.ReduceOp.SUM, group=group)
    return t


class ReconMSE:
    """Running sum of per-sample mean squared reconstruction errors (eval_gen_recon.py:192-211)."""

    def __init__(self, device):
        self.acc = torch.zeros(2, dtype=torch.float64, device=device)

    def update(self, x_hat, x):
        per_sample = torch.mean((x_hat - x) ** 2, dim=list(range(1, x.dim())))
        self.acc[0] += per_sample.double().sum()
        self.acc[1] += per_sample.numel()

    def compute(self):
        tot = all_reduce_sum_(self.acc.clone())
        return float(tot[0] / tot[1])


class FidStats:
    """Sufficient statistics of feature vectors for the Frechet distance: sum f, sum f f^T, n (fp64).

    The feature extractor (Inception, third-party, unavailable offline) is outside the hot path;
    this class only shards and reduces its outputs, and the plain fp64 GEMM goes to the vendor BLAS.
    """

    def __init__(self, dim, device):
        self.s1 = torch.zeros(dim, dtype=torch.float64, device=device)
        self.s2 = torch.zeros(dim, dim, dtype=torch.float64, device=device)
        self.n = torch.zeros(1, dtype=torch.float64, device=device)

    def update(self, feats):
        f = feats.double().reshape(feats.shape[0], -1)
        self.s1 += f.sum(0)
        self.s2 += f.t() @ f
        self.n += f.shape[0]

    def compute(self):
        flat = torch.cat([self.s1, self.s2.reshape(-1), self.n])
        all_reduce_sum_(flat)
        d = self.s1.numel()
        s1, s2, n = flat[:d], flat[d:d + d * d].reshape(d, d), float(flat[-1])
        mu = s1 / n
        sigma = (s2 - n * torch.outer(mu, mu)) / (n - 1)
        return mu, sigma


def sharded_recon_mse(Q, G, E, batches, g_l_steps=10, g_llhd_sigma=0.1, g_l_step_size=0.1):
    """Eval reconstruction MSE over global batches, each split across ranks (eval_gen_recon.py:177-212).

    batches: iterable of global x batches (identical on every rank); rank r processes its slice.
    Every rank draws the same global initial latents and sweep key from its (identically seeded) torch
    generator and runs its slice with chain_base = the slice start, so the Q sweep and the posterior
    chains of the union of the shards are bitwise the 1-GPU run's.
    """
    from . import amortizer, langevin

    d = _dist()
    rank, world = (d.get_rank(), d.get_world_size()) if d is not None else (0, 1)
    meter = None
    for x in batches:
        s, c = shard(x.shape[0], rank, world)
        # global draws, identical on every rank (host generator), in q_forward's order: zt, then the sweep key
        zt = torch.randn(x.shape[0], Q.nz)
        seed = langevin.new_seed() if Q.with_noise else 0
        if c == 0:
            continue
        xs = x[s:s + c].contiguous()
        meter = meter or ReconMSE(xs.device)
        with torch.no_grad():
            z = amortizer.q_forward(Q, x=xs, zt=zt[s:s + c], seed=seed, chain_base=s)
        langevin.posterior_langevin(z, xs, G, E, g_l_steps, g_llhd_sigma, g_l_step_size, False, chain_base=s)
        meter.update(langevin.generator_forward(z, G), xs)
    if meter is None:
        meter = ReconMSE(torch.device("cuda"))
    return meter.compute()


def all_gather_shards(local, batch_sizes, group=None):
    """Per-rank values of sharded global batches -> the global vector, in global order, on every rank.

    local: this rank's values, its shard() slice of every batch in batch order (1-D).  Scores are not a sum, so the
    one collective is an all_gather of fixed-size slices: every rank sends [count, values padded to the largest
    rank's count] in fp64 (fp32 values travel exactly), and the counts that arrive are checked against shard()'s.
    World size 1 needs no process group."""
    d = _dist()
    rank, world = (d.get_rank(group), d.get_world_size(group)) if d is not None else (0, 1)
    local = local.reshape(-1).to(torch.float64)
    sizes = [int(n) for n in batch_sizes]
    per_rank = [sum(shard(n, r, world)[1] for n in sizes) for r in range(world)]
    if local.numel() != per_rank[rank]:
        raise ValueError("rank %d holds %d values, its shards hold %d" % (rank, local.numel(), per_rank[rank]))
    if world == 1:
        return local
    buf = torch.zeros(1 + max(per_rank), dtype=torch.float64, device=local.device)
    buf[0] = local.numel()
    buf[1:1 + local.numel()] = local
    got = [torch.empty_like(buf) for _ in range(world)]
    d.all_gather(got, buf, group=group)
    counts = [int(g[0].item()) for g in got]
    if counts != per_rank:
        raise RuntimeError("gathered shard counts %s, expected %s" % (counts, per_rank))
    offs, parts = [1] * world, []
    for n in sizes:  # global order: batch by batch, each batch's slices in rank order
        for r in range(world):
            c = shard(n, r, world)[1]
            parts.append(got[r][offs[r]:offs[r] + c])
            offs[r] += c
    return torch.cat(parts) if parts else local


def sharded_pr_auc(Q, G, E, batches, labels, g_l_steps=5, g_l_step_size=0.1, g_llhd_sigma=1.0, recon_weight=1.0,
                   scorer=None):
    """PR-AUC of the anomaly score over global batches, each split across ranks (eval_anomaly_det.py:100-126).

    batches: iterable of global x batches (identical on every rank); labels: the global labels in the batches' order
    (one vector, or one per batch), 1 = anomalous.  As in sharded_recon_mse, every rank draws the same global initial
    latents and sweep key in q_forward's order and scores its slice with chain_base = the slice start
    (anomaly.score), so the scores of the union of the shards are bitwise the 1-GPU run's; one all_gather at the end
    (all_gather_shards), then every rank computes anomaly.pr_auc of the gathered vector.
    scorer(xs, zt, seed, chain_base) -> (count,) scores replaces anomaly.score (tests of the gather)."""
    from . import anomaly, langevin

    if scorer is None:
        def scorer(xs, zt, seed, chain_base):
            return anomaly.score(Q, G, E, xs, g_l_steps=g_l_steps, g_l_step_size=g_l_step_size,
                                 g_llhd_sigma=g_llhd_sigma, recon_weight=recon_weight, zt=zt, seed=seed,
                                 chain_base=chain_base)[0]

    d = _dist()
    rank, world = (d.get_rank(), d.get_world_size()) if d is not None else (0, 1)
    sizes, mine, device = [], [], None
    for x in batches:
        sizes.append(int(x.shape[0]))
        s, c = shard(x.shape[0], rank, world)
        # global draws, identical on every rank (host generator), in q_forward's order: zt, then the sweep key
        zt = torch.randn(x.shape[0], Q.nz)
        seed = langevin.new_seed() if Q.with_noise else 0
        device = device or x.device
        if c == 0:
            continue
        mine.append(scorer(x[s:s + c].contiguous(), zt[s:s + c], seed, s).reshape(-1))
    local = torch.cat(mine) if mine else torch.zeros(0, dtype=torch.float32, device=device or "cpu")
    scores = all_gather_shards(local, sizes).cpu().numpy()
    parts = labels if isinstance(labels, (list, tuple)) else [labels]
    y = torch.cat([torch.as_tensor(v).reshape(-1).cpu() for v in parts]).numpy()
    return anomaly.pr_auc(y, scores)


# ------------------------------------------------------------------------------------- data-parallel updates
def bucket_layout(numels):
    """(offsets, total) of a gradient bucket: prefix sums of the sizes rounded up to 4 elements, so every slice of a
    16-byte aligned buffer is 16-byte aligned and the clip norm over the slices takes grad_sumsq_kernel's vector path,
    in the same order as over separately allocated gradients."""
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off += (int(n) + 3) // 4 * 4
    return offs, off


def iteration_seed(base_seed, iteration, purpose=0):
    """A 62-bit Philox seed for (base_seed, iteration, purpose): a pure host hash (splitmix64's finaliser over the
    three words), equal on every rank without a collective.  purpose separates the seeds one iteration needs (the Q
    sweep, the posterior chains, the prior chains, the Q update, ...)."""
    m = (1 << 64) - 1
    h = 0
    for w in (int(base_seed), int(iteration), int(purpose)):
        h = (h + (w & m) + 0x9E3779B97F4A7C15) & m
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & m
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & m
        h ^= h >> 31
    return h >> 2


def grad_pack(grads, numels, offsets, bucket, scale):
    """bucket[offsets[t] : offsets[t] + numels[t]] = grads[t] * scale (damc_grad_pack), one launch per 96 tensors; a
    None gradient writes zeros.  The elements between the slices are left as they are."""
    from . import _lib, optim

    f32, strided = torch.float32, torch.strided
    for t in (*grads, bucket):
        # optim._require_fp32_cuda, as one expression on the common case (optim.Adam._collect does the same)
        if t is not None and not (t.dtype is f32 and t.is_cuda and t.layout is strided and t.is_contiguous()):
            optim._require_fp32_cuda(t, "grad_pack")
    if len(grads) != len(numels) or len(grads) != len(offsets) or any(
            g is not None and g.numel() != n for g, n in zip(grads, numels)):
        raise _lib.DamcError("grad_pack: gradients, sizes and offsets disagree")
    if any(o < 0 or o + n > bucket.numel() for o, n in zip(offsets, numels)):
        raise _lib.DamcError("grad_pack: a slice lies outside the bucket")
    chunks = optim._Chunks.of(list(numels), bucket.device)
    L, s = _lib.lib(), optim._stream()
    for t0, t1, dev, n, _ in chunks.slices:
        ptrs = (ctypes.c_void_p * (t1 - t0))(*[g.data_ptr() if g is not None else None for g in grads[t0:t1]])
        offs = (ctypes.c_longlong * (t1 - t0))(*offsets[t0:t1])
        optim._check(L.damc_grad_pack(ctypes.c_void_p(dev.data_ptr()), n, ptrs, offs, t1 - t0, float(scale),
                                      ctypes.c_void_p(bucket.data_ptr()), s), "damc_grad_pack")
    return bucket


class _Layout:
    def __init__(self, index, numels, device):
        self.index, self.numels = index, numels
        self.offsets, self.total = bucket_layout(numels)
        self.buffer = torch.empty(max(self.total, 4), dtype=torch.float32, device=device)
        self.buffer.zero_()  # the padding between slices stays zero: pack never writes it
        self.host = None     # pinned staging buffer of the gloo route
        self.views = None    # the slices as the parameters' shapes, made on the first attach


class GradBucket:
    """One flat fp32 buffer for the gradients of ``params``, for a single all_reduce per update.

    The layout covers the parameters whose ``.grad`` is not None, in order (``optim.Adam._collect``'s rule); the slice
    offsets are ``bucket_layout``'s.  The layout and its buffer are cached per (device, index / size tuple), so an
    update whose set of gradients repeats allocates nothing.  ``pack`` -> ``all_reduce`` -> ``attach`` leaves every
    covered ``p.grad`` a view of the reduced buffer: there is no unpack pass, the clip norm and the Adam step read the
    slices through their pointer tables as they read any gradient."""

    def __init__(self, params):
        self.params = [p for p in params]
        self._layouts = {}
        self.layout = None

    def _current(self):
        from . import _lib

        index = tuple(i for i, p in enumerate(self.params) if p.grad is not None)
        if not index:
            raise _lib.DamcError("GradBucket: no parameter has a gradient")
        grads = [self.params[i].grad for i in index]
        dev = grads[0].device
        if dev.type != "cuda":
            raise _lib.DamcError("GradBucket: the gradients must be on a ROCm device (got %s); the pack kernel has no "
                                 "CPU fallback" % dev)
        numels = tuple(g.numel() for g in grads)
        key = (str(dev), index, numels)
        lay = self._layouts.get(key)
        if lay is None:
            if len(self._layouts) > 16:
                self._layouts.clear()
            lay = self._layouts[key] = _Layout(index, numels, dev)
        self.layout = lay
        return lay, grads

    @property
    def buffer(self):
        return self.layout.buffer if self.layout is not None else None

    @torch.no_grad()
    def pack(self, scale=1.0):
        """buffer slice t = grad t * scale, for the parameters that have a gradient now; returns the buffer."""
        lay, grads = self._current()
        return grad_pack(grads, lay.numels, lay.offsets, lay.buffer, scale)

    def all_reduce(self, group=None):
        """One SUM all_reduce of the flat buffer.  RCCL reduces in place; under a gloo group a device buffer is staged
        through a pinned host tensor (ranks that share one GPU in the tests; bench.py reduces on the CPU under gloo)."""
        d = _dist()
        lay = self.layout
        if lay is None:
            raise RuntimeError("GradBucket.all_reduce before pack")
        if d is None or d.get_world_size(group) == 1:
            return lay.buffer
        if d.get_backend(group) == "gloo" and lay.buffer.is_cuda:
            if lay.host is None:
                lay.host = torch.empty(lay.buffer.shape, dtype=torch.float32).pin_memory()
            lay.host.copy_(lay.buffer)  # a blocking device-to-host copy: ordered after pack on the current stream
            d.all_reduce(lay.host, op=d.ReduceOp.SUM, group=group)
            lay.buffer.copy_(lay.host, non_blocking=True)
        else:
            d.all_reduce(lay.buffer, op=d.ReduceOp.SUM, group=group)
        return lay.buffer

    def attach(self):
        """p.grad = the buffer's slice, viewed as p, for every covered parameter."""
        lay = self.layout
        if lay is None:
            raise RuntimeError("GradBucket.attach before pack")
        if lay.views is None:  # the same view objects every update: ~100 slices + reshapes are host time otherwise
            lay.views = [lay.buffer[off:off + n].view_as(self.params[i])
                         for i, off, n in zip(lay.index, lay.offsets, lay.numels)]
        for i, v in zip(lay.index, lay.views):
            self.params[i].grad = v

    def verify(self, group=None):
        """Debug check, not on the step's path: every rank must hold gradients for the same parameters (one
        all_gather_object of the (index, numel) tuples); raises RuntimeError on every rank if they disagree."""
        index = tuple(i for i, p in enumerate(self.params) if p.grad is not None)
        mine = (index, tuple(self.params[i].grad.numel() for i in index))
        d = _dist()
        if d is None or d.get_world_size(group) == 1:
            return
        got = [None] * d.get_world_size(group)
        d.all_gather_object(got, mine, group=group)
        if any(g != got[0] for g in got):
            bad = [r for r, g in enumerate(got) if g != got[0]]
            raise RuntimeError("GradBucket.verify: ranks %s hold gradients for other parameters than rank 0 (%s)"
                               % (bad, [len(g[0]) for g in got]))


def sharded_step(optimizer, local_batch, global_batch, max_norm=None, group=None, verify=False):
    """The data-parallel form of clip + step, after this rank's backward over its ``local_batch`` rows of the
    ``global_batch``: pack the gradients scaled by local / global (every loss of the drivers is a mean over the local
    rows, so the sum over ranks is the global mean's gradient), one all_reduce, gradients re-pointed at the reduced
    buffer, then ``optimizer.clip_and_step(max_norm)`` (damc.optim) -- ``step()`` when max_norm is None; a stock
    optimiser gets clip_grad_norm_ followed by step().  Returns the total norm, or None.  A world of 1 takes the same
    path (pack and attach, no collective)."""
    bucket = getattr(optimizer, "_damc_grad_bucket", None)
    params = [p for g in optimizer.param_groups for p in g["params"]]
    if bucket is None or len(bucket.params) != len(params) or any(a is not b for a, b in zip(bucket.params, params)):
        bucket = optimizer._damc_grad_bucket = GradBucket(params)
    if verify:
        bucket.verify(group)
    bucket.pack(float(local_batch) / float(global_batch))
    bucket.all_reduce(group)
    bucket.attach()
    if max_norm is None:
        optimizer.step()
        return None
    if hasattr(optimizer, "clip_and_step"):
        return optimizer.clip_and_step(max_norm)
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    optimizer.step()
    return norm
