"""Graph-replayable training: a Philox key that lives on the device, and a capture helper.

Every seeded entry point takes ``seed`` / ``step_offset`` / ``draw_index`` as host values; a ``torch.cuda.CUDAGraph``
bakes them into the kernel arguments at capture, so a replay would draw the noise of the captured iteration again.
``DrawState`` holds the key in device memory instead (``damc_draw_state_t``: seed, counter).  Passed as ``draws=`` where
an entry point takes ``seed=``, the kernels read it at run time: the result is bitwise the seeded call with
``seed = state.seed`` and the host offset plus ``state.counter``.  The high-level wrappers enqueue the advance
themselves (Langevin by ``n_steps``, the sweep by ``n_interval``, ``Q.calculate_loss`` by 1 after its three draws); the
per-op hooks (``philox_*``, ``z_update``, ``q_noise_glue_seeded``) leave the counter alone.  One state per noise
consumer keeps the streams what a seeded loop with one seed per consumer draws.

A captured iteration::

    ds_post, ds_prior, ds_q = (graphs.DrawState(s, dev) for s in (seed_a, seed_b, seed_c))
    opt = damc.optim.AdamW(Q.parameters(), lr=lr_tensor, capturable=True)

    def body():
        langevin.posterior_langevin(z, x, G, E, 30, 0.1, 0.1, True, draws=ds_post)
        opt.zero_grad(set_to_none=False)
        Q.calculate_loss(x, z, mask, draws=ds_q).mean().backward()
        opt.clip_and_step(max_norm)

    graph = graphs.capture(body)   # runs body once for real (warm-up), then records it
    for it in range(n):
        x.copy_(next_batch)        # inputs are rewritten in place
        graph.replay()
"""
import ctypes

import torch

from . import _lib
from ._lib import check

_MASK64 = (1 << 64) - 1


class DrawState:
    """``damc_draw_state_t`` in device memory: two uint64 words (seed, counter), held as an int64 tensor of 2
    (``words=``: the caller's own 2-element int64 device tensor, e.g. a slice of a larger buffer)."""

    def __init__(self, seed, device, counter=0, words=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DamcError("DrawState lives in device memory (got %s); the HIP path has no CPU fallback" % device)
        if words is None:
            words = torch.empty(2, dtype=torch.int64, device=device)
        elif (words.dtype != torch.int64 or words.numel() != 2 or not words.is_contiguous() or
              words.device.type != "cuda" or words.data_ptr() % 8):
            raise _lib.DamcError("DrawState words: a contiguous int64 device tensor of 2 elements")
        self.device = words.device
        self.words = words
        self.set(seed, counter)

    @staticmethod
    def _i64(v):
        v = int(v) & _MASK64
        return v - (1 << 64) if v >= (1 << 63) else v

    def set(self, seed, counter=0):
        """Overwrite both words (eager only: the values are host scalars, fixed at capture)."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.DamcError("DrawState.set inside a capture would replay the same key; use advance()")
        self.words.copy_(torch.tensor([self._i64(seed), self._i64(counter)], dtype=torch.int64))

    def advance(self, n):
        """counter += n on the current stream (``damc_draw_state_advance``: one tiny kernel, capturable)."""
        check(_lib.lib().damc_draw_state_advance(self.ptr(), int(n) & _MASK64, _lib.stream_ptr(self.device)),
              "damc_draw_state_advance")

    def read(self):
        """(seed, counter) as Python ints; synchronises."""
        s, c = self.words.cpu().tolist()
        return s & _MASK64, c & _MASK64

    def ptr(self):
        return ctypes.c_void_p(self.words.data_ptr())


def exclusive(seed, draws, what):
    """The ``draws=`` / ``seed=`` rule of every wrapper: at most one of them; ``draws`` is a DrawState."""
    if draws is None:
        return
    if seed is not None:
        raise _lib.DamcError("%s: draws= and seed= are mutually exclusive (the state carries the seed)" % what)
    if not isinstance(draws, DrawState):
        raise _lib.DamcError("%s: draws= takes a damc.graphs.DrawState" % what)


def capture(body, pool=None):
    """Record ``body()`` into a ``torch.cuda.CUDAGraph`` and return it.

    ``body`` first RUNS ONCE FOR REAL on a side stream -- the warm-up torch.cuda.graphs asks for, which also lets every
    cache on the path (packed-weight plans, workspaces, schedule tables, chunk tables, optimiser state) fill outside
    the capture: restore whatever it changed (parameters, moments, step counts, DrawState words, in place) before the
    first replay if that run must not count.  The capture itself is on one stream with no forked branches.  Tensors
    ``body`` reads are read at their captured addresses on every replay: feed new data with ``copy_``."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=pool):
        body()
    return graph
