"""One whole training iteration of the reference driver (``workspace/train_gen_recon.py:187-261``) as a body that a
``torch.cuda.CUDAGraph`` can record once and replay as successive iterations.

``TrainIteration.body()`` enqueues, in the reference's order: the mask, ``z0 = Q_target(x)`` and ``zp = Q(None, b)``,
the posterior and the prior Langevin chains, six Q updates, the G update, the E update, the learning-rate decay, the EMA
of the target and the advance of the iteration clock.  Nothing in it reads a device value on the host, every random
draw comes from a ``damc.graphs.DrawState`` and the two "every Nth iteration" branches are decided on the device
(``damc.schedule``), so replay ``k`` of the recorded graph IS iteration ``clock0 + k``.

Draws.  Each noise consumer has one ``DrawState`` (``make_draws``: seed ``base + index in CONSUMERS``) and moves its
counter by a fixed amount per iteration (``strides``), so with the counters at 0 when the clock reads 0, iteration
``k`` equals these host-seeded calls (``n`` = ``Q.n_interval``, ``B`` = the batch, ``s[c]`` = the consumer's seed;
``offsets(k, ...)`` returns the counters)::

    consumer      stride    iteration k draws
    mask          1         philox_uniform(1, B, s, step_offset=k)[0]; mask = 0 where u < p_mask, else 1
    zt_target     1         philox_normal(1, B, nz, s, step_offset=k)[0]: the initial latent of Q_target(x)
    sweep_target  n         the sweep of Q_target(x); its noisy step j draws index k n + j of stream STREAM_SWEEP:
                            reverse_sweep(noise=philox_normal(n - 1, B, nz, s, step_offset=k n, stream_id=STREAM_SWEEP))
    pe_prior      1         philox_normal(1, B, nz, s, step_offset=k)[0]: the prior-embedding noise of Q(None, B)
    zt_prior      1         philox_normal(1, B, nz, s, step_offset=k)[0]: the initial latent of Q(None, B)
    sweep_prior   n         as sweep_target, for Q(None, B)
    posterior     g_l_steps posterior_langevin(..., seed=s, step_offset=k g_l_steps)
    fresh         1         philox_normal(1, B, nz, s, step_offset=k)[0]: the fresh half of the prior chains' batch
    prior         e_l_steps prior_langevin(..., seed=s, step_offset=k e_l_steps)   (2 B chains)
    q             q_updates Q.calculate_loss(x, zk_pos, mask, seed=s, draw_index=k q_updates + j), j < q_updates

Out of scope for a capture, raising what they raise today: the guided sweep (``cond_w > 0``), train-mode spectral-norm
chains and the unseeded ``calculate_loss``.  The data-parallel all-reduce is not part of the body.
"""
import torch

from . import _lib, amortizer, graphs, langevin
from .schedule import EmaTarget, LrDecay, TrainClock

CONSUMERS = ("mask", "zt_target", "sweep_target", "pe_prior", "zt_prior", "sweep_prior", "posterior", "fresh", "prior",
             "q")


def strides(n_interval, g_l_steps, e_l_steps, q_updates=6):
    """How far one iteration moves each consumer's counter."""
    return {"mask": 1, "zt_target": 1, "sweep_target": int(n_interval), "pe_prior": 1, "zt_prior": 1,
            "sweep_prior": int(n_interval), "posterior": int(g_l_steps), "fresh": 1, "prior": int(e_l_steps),
            "q": int(q_updates)}


def offsets(iteration, n_interval, g_l_steps, e_l_steps, q_updates=6):
    """Every consumer's counter at the start of ``iteration`` (counters 0 at iteration 0): iteration * stride."""
    return {c: int(iteration) * s for c, s in strides(n_interval, g_l_steps, e_l_steps, q_updates).items()}


def seeds(base_seed):
    """The consumers' seeds: ``base_seed + index in CONSUMERS`` (mod 2^64)."""
    return {c: (int(base_seed) + i) & ((1 << 64) - 1) for i, c in enumerate(CONSUMERS)}


def make_draws(base_seed, device, iteration=0, n_interval=None, g_l_steps=None, e_l_steps=None, q_updates=6):
    """One DrawState per consumer, carved from one device buffer.  ``iteration`` > 0 (a resumed run) needs the three
    step counts and starts the counters at ``offsets(iteration, ...)``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DamcError("make_draws: draw states live in device memory (got %s)" % device)
    off = dict.fromkeys(CONSUMERS, 0)
    if iteration:
        if None in (n_interval, g_l_steps, e_l_steps):
            raise _lib.DamcError("make_draws(iteration > 0): needs n_interval, g_l_steps and e_l_steps")
        off = offsets(iteration, n_interval, g_l_steps, e_l_steps, q_updates)
    buf = torch.empty(2 * len(CONSUMERS), dtype=torch.int64, device=device)
    sd = seeds(base_seed)
    return {c: graphs.DrawState(sd[c], device, counter=off[c], words=buf[2 * i:2 * i + 2])
            for i, c in enumerate(CONSUMERS)}


class TrainIteration:
    """The reference iteration over G, E, Q and the EMA target Q_target.

    optimizers: ``(G_optimizer, Q_optimizer, E_optimizer)``, capturable ``damc.optim`` Adam / AdamW.  clock: a
    ``schedule.TrainClock``.  draws: ``make_draws(...)`` (a dict with one DrawState per name in CONSUMERS).  x: the
    batch tensor the body reads; the caller rewrites it in place (``x.copy_(next_batch)``) between iterations.  The
    remaining arguments are the driver's command-line hyper-parameters under their names there; a ``*_max_norm`` of
    None leaves that update unclipped (``*_is_grad_clamp`` off).  ``ema`` / ``lr_decay``: ready-made
    ``schedule.EmaTarget`` / ``schedule.LrDecay`` objects, else built here with the driver's constants (rho 0.005 every
    10th, 0.99 down to 1e-5 every 1000th iteration).

    After ``body()`` (or a replay) ``zk_pos``, ``zk_neg``, ``z_mask``, ``z0`` and ``zp`` hold the iteration's latents:
    device tensors, to be read after a synchronise."""

    def __init__(self, G, E, Q, Q_target, optimizers, clock, draws, x, *, p_mask, g_l_steps, g_llhd_sigma,
                 g_l_step_size, e_l_steps, e_l_step_size, g_l_with_noise=True, e_l_with_noise=True, q_updates=6,
                 q_max_norm=None, g_max_norm=None, e_max_norm=None, rho=0.005, ema_period=10, lr_factor=0.99,
                 lr_floor=1e-5, lr_period=1000, ema=None, lr_decay=None):
        if not isinstance(clock, TrainClock):
            raise _lib.DamcError("TrainIteration: clock takes a damc.schedule.TrainClock")
        missing = [c for c in CONSUMERS if not isinstance(draws.get(c), graphs.DrawState)]
        if missing:
            raise _lib.DamcError("TrainIteration: draws lacks a DrawState for %s (see make_draws)" % ", ".join(missing))
        if len({draws[c].words.data_ptr() for c in CONSUMERS}) != len(CONSUMERS):
            raise _lib.DamcError("TrainIteration: every noise consumer needs a DrawState of its own")
        if x.device.type != "cuda" or x.dtype != torch.float32 or not x.is_contiguous():
            raise _lib.DamcError("TrainIteration: x must be a contiguous float32 tensor on a ROCm device")
        self.G, self.E, self.Q, self.Q_target = G, E, Q, Q_target
        self.G_opt, self.Q_opt, self.E_opt = optimizers
        for o in (self.G_opt, self.Q_opt, self.E_opt):
            if not all(g.get("capturable", False) for g in o.param_groups):
                raise _lib.DamcError("TrainIteration: the optimisers must be damc.optim Adam / AdamW(capturable=True)")
        self.clock, self.draws, self.x = clock, draws, x
        self.p_mask = float(p_mask)
        self.g_l_steps, self.g_llhd_sigma, self.g_l_step_size = int(g_l_steps), float(g_llhd_sigma), float(g_l_step_size)
        self.e_l_steps, self.e_l_step_size = int(e_l_steps), float(e_l_step_size)
        self.g_l_with_noise, self.e_l_with_noise = bool(g_l_with_noise), bool(e_l_with_noise)
        self.q_updates = int(q_updates)
        self.q_max_norm, self.g_max_norm, self.e_max_norm = q_max_norm, g_max_norm, e_max_norm
        self.ema = ema if ema is not None else EmaTarget(list(Q.parameters()), list(Q_target.parameters()), rho=rho,
                                                         period=ema_period, phase=1)
        self.lr_decay = lr_decay if lr_decay is not None else LrDecay([self.G_opt, self.Q_opt, self.E_opt],
                                                                      factor=lr_factor, floor=lr_floor,
                                                                      period=lr_period, phase=1)
        self.z_mask = self.z0 = self.zp = self.zk_pos = self.zk_neg = None

    def strides(self):
        return strides(self.Q.n_interval, self.g_l_steps, self.e_l_steps, self.q_updates)

    @staticmethod
    def _step(opt, max_norm):
        if max_norm is None:
            opt.step()
        else:
            opt.clip_and_step(max_norm)

    def _normal(self, name, rows):
        """(rows, nz) from the consumer's stream at its counter; the counter then moves on by 1."""
        ds = self.draws[name]
        out = langevin.philox_normal(1, rows, self.Q.nz, device=self.x.device, draws=ds)[0]
        ds.advance(1)
        return out

    def body(self):
        G, E, Q, Qt, x, d = self.G, self.E, self.Q, self.Q_target, self.x, self.draws
        B, dev = x.shape[0], x.device
        # :187-190 the mask: 0 where u < p_mask
        u = langevin.philox_uniform(1, B, device=dev, draws=d["mask"])[0]
        d["mask"].advance(1)
        z_mask = torch.ge(u, self.p_mask).to(torch.float32).unsqueeze(-1)
        # :192-198 z0 = Q_target(x), zp = Q(None, B)
        Q.eval(), G.eval(), E.eval()
        with torch.no_grad():
            z0 = self._normal("zt_target", B)
            amortizer.reverse_sweep(Qt, amortizer.encoder_forward(Qt.encoder, x), z0, draws=d["sweep_target"])
            xemb = amortizer.prior_embedding(Q, self._normal("pe_prior", B))
            zp = self._normal("zt_prior", B)
            amortizer.reverse_sweep(Q, xemb, zp, draws=d["sweep_prior"])
            # :199-209 the posterior chains from z0, the prior chains from [z0, fresh normals]
            zk_pos = z0.clone()
            langevin.posterior_langevin(zk_pos, x, G, E, self.g_l_steps, self.g_llhd_sigma, self.g_l_step_size,
                                        self.g_l_with_noise, draws=d["posterior"])
            zk_neg = torch.cat([z0, self._normal("fresh", B)], dim=0)
            langevin.prior_langevin(zk_neg, E, self.e_l_steps, self.e_l_step_size, self.e_l_with_noise,
                                    draws=d["prior"])
        # :211-220 the Q updates
        for _ in range(self.q_updates):
            self.Q_opt.zero_grad()
            Q.train()
            Q.calculate_loss(x=x, z=zk_pos, mask=z_mask, draws=d["q"]).mean().backward()
            self._step(self.Q_opt, self.q_max_norm)
        # :222-231 the G update
        self.G_opt.zero_grad()
        G.train()
        torch.sum((G(zk_pos) - x) ** 2, dim=[1, 2, 3]).mean().backward()
        self._step(self.G_opt, self.g_max_norm)
        # :233-241 the E update
        self.E_opt.zero_grad()
        E.train()
        e_pos, e_neg = E(zk_pos), E(zk_neg)
        (e_pos.mean() - e_neg.mean()).backward()
        self._step(self.E_opt, self.e_max_norm)
        Q.eval(), G.eval(), E.eval()
        # :246-261 the schedule and the EMA, gated on the device by the clock; then the next iteration
        self.lr_decay.step(self.clock)
        self.ema.update(self.clock)
        self.clock.advance(1)
        self.z_mask, self.z0, self.zp, self.zk_pos, self.zk_neg = z_mask, z0, zp, zk_pos, zk_neg

    def capture(self, pool=None):
        """``graphs.capture(self.body)``: body runs ONCE FOR REAL first (the warm-up, one iteration's worth of updates,
        draws and clock); a caller for whom that run must not count restores parameters, optimiser state, the lr
        tensors, the DrawState words and the clock in place before the first replay."""
        return graphs.capture(self.body, pool=pool)
