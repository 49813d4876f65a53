"""The glue of a training iteration on the device: iteration clock, EMA target, learning-rate decay.

The reference driver (``workspace/train_gen_recon.py:247-261``) runs these on the host between its updates::

    if (iteration + 1) % 1000 == 0:  lr = max(lr * 0.99, 1e-5)  -> param_groups[...]["lr"]       (Python doubles)
    if (iteration + 1) % 10 == 0:    target.data.copy_(rho * param.data + (1 - rho) * target.data)  per parameter of Q

A recorded graph takes a host ``if`` always or never.  Here the iteration count is one word in device memory
(``TrainClock``); ``EmaTarget.update(clock)`` and ``LrDecay.step(clock)`` enqueue launches that read it and write nothing
when they are not due (``csrc/schedule.hip``), and ``clock.advance()`` is a launch of its own.  A graph that ends with
the three runs the next iteration on its next replay.  Results are bitwise the host-gated expressions above: the EMA is
two rounded products and a rounded add in fp32 (torch's three kernels), the decay is the Python expression in IEEE
double, rounded to the fp32 scalar the capturable optimiser reads as ``lr`` exactly as ``torch.tensor(lr)`` rounds it.

There is no fallback: CPU tensors raise ``DamcError``.
"""
import ctypes

import torch

from . import _lib
from .optim import _Chunks

_MASK64 = (1 << 64) - 1
_VP = ctypes.c_void_p


def _check(code, what):
    if code != 0:  # the glue calls return -DAMC_ERR_ARG; a HIP error is positive
        raise _lib.DamcError("%s failed: %s (code %d)" % (what, _lib.lib().damc_error_string(abs(code)).decode(), code))


def _no_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise _lib.DamcError("%s inside a capture would replay the captured host values" % what)


class TrainClock:
    """The iteration count as one uint64 word in device memory (held as an int64 tensor of 1).  The gated calls read
    it; only ``advance`` writes it, in a launch of its own."""

    def __init__(self, device, iteration=0):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DamcError("TrainClock lives in device memory (got %s); the HIP path has no CPU fallback" % device)
        self.word = torch.empty(1, dtype=torch.int64, device=device)
        self.device = self.word.device
        self.set(iteration)

    def set(self, iteration):
        """Overwrite the count (eager only: a host value, fixed at capture)."""
        _no_capture("TrainClock.set")
        v = int(iteration) & _MASK64
        self.word.copy_(torch.tensor([v - (1 << 64) if v >= (1 << 63) else v], dtype=torch.int64))

    def advance(self, n=1):
        """count += n on the current stream (``damc_iteration_advance``: one tiny kernel, capturable)."""
        _check(_lib.lib().damc_iteration_advance(self.ptr(), int(n) & _MASK64, _lib.stream_ptr(self.device)),
               "damc_iteration_advance")

    def read(self):
        """The count as a Python int; synchronises."""
        return int(self.word.cpu()[0]) & _MASK64

    def ptr(self):
        return _VP(self.word.data_ptr())


def _clock_ptr(clock):
    if clock is None:
        return None
    if not isinstance(clock, TrainClock):
        raise _lib.DamcError("clock= takes a damc.schedule.TrainClock (or None: apply always)")
    return clock.ptr()


class EmaTarget:
    """``target = rho * source + (1 - rho) * target`` over two parameter lists (train_gen_recon.py:258-261), one
    ``damc_ema_update`` launch per 96 tensors.  ``update(clock)`` applies it when ``(clock + phase) % period == 0``
    -- the reference's ``(iteration + 1) % 10 == 0`` is the default -- and leaves the targets untouched otherwise;
    ``update()`` applies it always.  The tensors are read and written in place at the addresses they have at
    construction (``param.data``): ``load_state_dict`` and ``copy_`` keep them, ``.to()`` does not."""

    def __init__(self, source_params, target_params, rho=0.005, period=10, phase=1):
        src = [p.detach() for p in source_params]
        tgt = [p.detach() for p in target_params]
        if len(src) != len(tgt) or not src:
            raise _lib.DamcError("EmaTarget: needs as many target as source tensors (got %d and %d)" % (len(tgt), len(src)))
        for i, (s, t) in enumerate(zip(src, tgt)):
            for what, x in (("source", s), ("target", t)):
                if x.dtype != torch.float32 or x.is_sparse or not x.is_contiguous():
                    raise _lib.DamcError("EmaTarget %s %d: needs dense contiguous float32 tensors" % (what, i))
            if s.shape != t.shape:
                raise _lib.DamcError("EmaTarget pair %d: source shape %s, target shape %s" % (
                    i, tuple(s.shape), tuple(t.shape)))
        for i, (s, t) in enumerate(zip(src, tgt)):
            if not s.is_cuda or s.device != t.device or s.device != src[0].device:
                raise _lib.DamcError("EmaTarget pair %d: runs on the HIP kernels only, on one ROCm device (source on "
                                     "%s, target on %s)" % (i, s.device, t.device))
        if int(period) < 1 or int(phase) < 0:
            raise _lib.DamcError("EmaTarget: period >= 1 and phase >= 0")
        self.source, self.target = src, tgt
        # Python doubles, rounded to fp32 once each: what torch does with a Python scalar times an fp32 tensor
        self.rho, self.one_minus_rho = float(rho), 1 - float(rho)
        self.period, self.phase = int(period), int(phase)
        self.device = src[0].device
        # this object's own tables (not the optimisers' shared cache): a recorded graph reads their device memory on
        # every replay
        self._chunks = _Chunks([t.numel() for t in tgt], self.device)
        self._args = [((_VP * (t1 - t0))(*[t.data_ptr() for t in tgt[t0:t1]]),
                       (_VP * (t1 - t0))(*[s.data_ptr() for s in src[t0:t1]]))
                      for t0, t1, _, _, _ in self._chunks.slices]

    def update(self, clock=None):
        L = _lib.lib()
        it = _clock_ptr(clock)
        s = _lib.stream_ptr(self.device)
        for (t0, t1, dev, n, _), (tp, sp) in zip(self._chunks.slices, self._args):
            _check(L.damc_ema_update(_VP(dev.data_ptr()), n, tp, sp, t1 - t0, self.rho, self.one_minus_rho, it,
                                     self.period, self.phase, s), "damc_ema_update")


class LrDecay:
    """``lr = max(lr * factor, floor)`` every ``period`` iterations (train_gen_recon.py:247-256) for the groups of
    capturable ``damc.optim`` optimisers.  The doubles live in one fp64 device tensor (the Python chain, bit for bit);
    each group's ``lr`` becomes a 0-d fp32 device tensor -- a view into ``lr32`` -- that ``damc_adam_step_capturable``
    reads on every launch.  ``step(clock)`` is one launch per 8 rates and writes nothing unless
    ``(clock + phase) % period == 0``."""

    def __init__(self, optimizers_or_groups, factor=0.99, floor=1e-5, period=1000, phase=1):
        groups = []
        for o in (optimizers_or_groups if isinstance(optimizers_or_groups, (list, tuple)) else [optimizers_or_groups]):
            groups += o.param_groups if isinstance(o, torch.optim.Optimizer) else [o]
        if not groups:
            raise _lib.DamcError("LrDecay: no parameter group")
        if int(period) < 1 or int(phase) < 0:
            raise _lib.DamcError("LrDecay: period >= 1 and phase >= 0")
        start, device = [], None
        for g in groups:
            if not isinstance(g, dict) or "lr" not in g or not g.get("capturable", False):
                raise _lib.DamcError("LrDecay: needs the param_groups of a capturable=True damc.optim optimiser (a float "
                                     "lr is a kernel argument, fixed at capture)")
        for g in groups:
            ps = g.get("params") or []
            d = ps[0].device if ps else None
            if d is None or d.type != "cuda" or (device is not None and d != device):
                raise _lib.DamcError("LrDecay: the groups' parameters must sit on one ROCm device")
            device = d
            start.append(float(g["lr"]))
        self.groups, self.device = groups, device
        self.factor, self.floor, self.period, self.phase = float(factor), float(floor), int(period), int(phase)
        self.lr64 = torch.tensor(start, dtype=torch.float64).to(device)
        self.lr32 = self.lr64.to(torch.float32)
        for i, g in enumerate(groups):
            g["lr"] = self.lr32[i]

    def step(self, clock):
        L = _lib.lib()
        it = _clock_ptr(clock)
        s = _lib.stream_ptr(self.device)
        for i in range(0, len(self.groups), _lib.LR_DECAY_MAX):
            n = min(_lib.LR_DECAY_MAX, len(self.groups) - i)
            _check(L.damc_lr_decay(_VP(self.lr64.data_ptr() + 8 * i), _VP(self.lr32.data_ptr() + 4 * i), n, self.factor,
                                   self.floor, it, self.period, self.phase, s), "damc_lr_decay")

    def values(self):
        """The rates as Python doubles; synchronises."""
        return self.lr64.cpu().tolist()

    def state_dict(self):
        _no_capture("LrDecay.state_dict")
        return {"lr": self.values(), "factor": self.factor, "floor": self.floor, "period": self.period,
                "phase": self.phase}

    def load_state_dict(self, state):
        """Eager only.  The tensors keep their addresses (a recorded graph and the groups point at them)."""
        _no_capture("LrDecay.load_state_dict")
        lr = [float(v) for v in state["lr"]]
        if len(lr) != len(self.groups):
            raise _lib.DamcError("LrDecay.load_state_dict: %d rates for %d groups" % (len(lr), len(self.groups)))
        self.factor, self.floor = float(state["factor"]), float(state["floor"])
        self.period, self.phase = int(state["period"]), int(state["phase"])
        host = torch.tensor(lr, dtype=torch.float64)
        self.lr64.copy_(host)
        self.lr32.copy_(host.to(torch.float32))


__all__ = ["TrainClock", "EmaTarget", "LrDecay"]
