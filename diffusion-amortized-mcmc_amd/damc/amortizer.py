"""The amortizer Q on the HIP path: encoder (or prior embedding) + latent reverse sweep.

Mirrors ``_netQ_U.forward`` (workspace/src/diffusion_net.py:585-622):
  x given : xemb = encoder(x)                 -> Encoder_* on the MFMA conv engine + fused IN/LReLU
  x None  : xemb = prior_emb(randn(b, nz))    -> two GEMMs (LeakyReLU 0.01 between)
  zt = randn(b, nz) (host generator, as the reference) then n_interval reverse steps in libdamc.
  cond_w > 0 : classifier-free guidance, both denoiser evaluations of every step in one damc_guided_sweep call.
The toy's _netQ_U_toy (workspace/toy_example/src/diffusion_net.py:141-239) takes the same route: its MLP encoder and
its prior_emb (nz = 2) run as one fused launch (damc_mlp_forward), its sweep in the library's row-resident form.

The per-step schedule scalars (logsnr_t/logsnr_s and the coefficients of pred_x_from_eps /
diffusion_reverse, diffusion_helper_func.py:36-70) and the sinusoidal time embedding input
(SinusoidalPosEmb, diffusion_net.py:447-461) are batch-invariant: they are evaluated once per
call on the host in fp32 with the reference's own op sequence and handed to the kernels.
"""
import ctypes
import math
import os
import threading
import weakref

import torch

from . import _lib
from ._lib import check, ptr


def _dev(t, device):
    t = t.detach()
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    return t


# ----------------------------------------------------------------------------- schedule
def _schedule(t, lmin, lmax):
    """logsnr_schedule_fn (diffusion_helper_func.py:41-50), fp32 op for op."""
    lmin_t = lmin * torch.ones_like(t)
    lmax_t = lmax * torch.ones_like(t)
    b = torch.arctan(torch.exp(-0.5 * lmax_t))
    a = torch.arctan(torch.exp(-0.5 * lmin_t)) - b
    return -2.0 * torch.log(torch.tan(a * t + b))


_TABLES = {}


def cached_step_tables(n_interval, logsnr_min, logsnr_max, var_type, ntemb, device):
    """step_tables depends only on the schedule: computed once per (schedule, device), then reused
    (building it costs ~25 tiny host ops per step, ~10 ms per 100-step sweep)."""
    key = (int(n_interval), float(logsnr_min), float(logsnr_max), str(var_type), int(ntemb), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        coef, temb = step_tables(n_interval, logsnr_min, logsnr_max, var_type, ntemb)
        hit = _TABLES[key] = (coef.contiguous(), temb.to(device))
    return hit


def step_tables(n_interval, logsnr_min, logsnr_max, var_type, ntemb):
    """Host tables for the sweep: coef (n, 6) and the sinusoidal time-embedding input (n, ntemb)."""
    coef = torch.zeros(n_interval, 6, dtype=torch.float32)
    temb = torch.zeros(n_interval, ntemb, dtype=torch.float32)
    half = ntemb // 2
    freqs = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
    for k, i in enumerate(reversed(range(n_interval))):
        it = torch.ones(1, dtype=torch.float32) * float(i)
        lt = _schedule(it / (n_interval - 1.0), logsnr_min, logsnr_max)
        ls = _schedule(torch.clamp(it - 1.0, min=0.0) / (n_interval - 1.0), logsnr_min, logsnr_max)
        c0 = torch.sqrt(1.0 + torch.exp(-lt))
        c1 = torch.rsqrt(1.0 + torch.exp(lt))
        alpha_st = torch.sqrt((1.0 + torch.exp(-lt)) / (1.0 + torch.exp(-ls)))
        alpha_s = torch.sqrt(torch.sigmoid(ls))
        r = torch.exp(lt - ls)
        omr = -torch.expm1(lt - ls)
        if var_type == "large":
            var = omr * torch.sigmoid(-lt)
        elif var_type == "small":
            a_t, a_s = torch.sigmoid(lt), torch.sigmoid(ls)
            var = (1.0 - a_s) / (1.0 - a_t) * (1 - a_t / a_s)
        else:
            raise NotImplementedError(var_type)
        coef[k] = torch.cat([c0, c1, r * alpha_st, omr * alpha_s, torch.sqrt(var),
                             torch.ones(1) if i == 0 else torch.zeros(1)])
        li = torch.arctan(torch.exp(-0.5 * torch.clamp(lt, min=-20.0, max=20.0))) / (0.5 * math.pi)
        li = li * (1000.0 / 1.0)  # SinusoidalPosEmb(max_time=1.) scales its input by 1000
        e = li[:, None] * freqs[None, :]
        temb[k] = torch.cat((e.sin(), e.cos()), dim=-1)[0]
    return coef, temb


# ------------------------------------------------------------------------------ encoder
class EncoderPlan:
    """Encoder_*.net = [Conv2d, InstanceNorm2d(affine), LeakyReLU(.2)]* Conv2d (diffusion_net.py:227-413)."""

    def __init__(self, enc):
        mods = list(enc.net)
        self.stages = []  # (conv, norm or None, slope or None)
        i = 0
        while i < len(mods):
            conv = mods[i]
            if not isinstance(conv, torch.nn.Conv2d) or hasattr(conv, "weight_orig"):
                raise NotImplementedError("unexpected encoder module %r" % (conv,))
            norm, slope = None, None
            if i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.InstanceNorm2d):
                norm = mods[i + 1]
                if not norm.affine or norm.track_running_stats:
                    raise NotImplementedError("InstanceNorm2d must be affine without running stats")
                slope = float(mods[i + 2].negative_slope)
                i += 3
            else:
                i += 1
            self.stages.append((conv, norm, slope))
        self.nemb = enc.nemb
        self._wcache = {}
        self._ws = _lib.WorkspaceCache()
        self._tls = threading.local()  # the cached descriptor (per thread: a call may be issued from several)
        self._cout = self.stages[-1][0].out_channels
        self._slots = []  # (parameter dict, name) of every tensor the descriptor points at
        for conv, norm, _ in self.stages:
            self._slots += [(conv._parameters, "weight"), (conv._parameters, "bias")]
            if norm is not None:
                self._slots += [(norm._parameters, "weight"), (norm._parameters, "bias")]

    def _packed(self, i, conv, dev, L, stream):
        """The conv's weight operand, repacked per call from the live parameter: the nets train between calls,
        and the reference updates its EMA target Q_dummy through param.data.copy_ (train_gen_recon.py:258-261),
        which leaves the parameter's version counter unchanged, so no version-keyed cache could see it.  A layer on
        the limb engine hands the library its PyTorch weight (w_src): damc_q_encoder_fwd packs all of them as extra
        workgroups of the first conv's launch (DAMC_ENC_WSRC=0: one damc_pack_conv2d_x3 launch per layer, before the
        call); the first 3x3 conv keeps the fp32 packing.  Buffers are reused across calls.  Returns (w_packed, w_x3,
        w_src, keep-alive, the packing call as (function, arguments) or None)."""
        k, cout, cin = conv.kernel_size[0], conv.out_channels, conv.in_channels
        w = _dev(conv.weight, dev)
        nb = int(L.damc_conv2d_x3_bytes(cout, cin, k)) if _lib.current_engine() == _lib.ENGINE_LIMB else 0
        if nb and os.environ.get("DAMC_ENC_WSRC", "1") != "0":
            w = w.contiguous()
            if w.data_ptr() % 16 == 0:
                return None, None, w, w, None
        # one buffer per (layer, thread, stream), like the workspace: a call on another stream or thread may still
        # be reading this one's packed weights
        cache = self._wcache.get(i)
        if cache is None:
            cache = self._wcache[i] = _lib.WorkspaceCache()
        buf = cache.get(dev, nb if nb else 4 * k * k * cin * cout, ("encw", i, nb))
        if nb:
            call = (L.damc_pack_conv2d_x3, (ptr(w), cout, cin, k, ptr(buf), stream))
            check(call[0](*call[1]), "pack conv2d x3")
            return None, buf, None, w, call
        buf = buf[:4 * k * k * cin * cout].view(torch.float32)
        call = (L.damc_pack_conv2d, (ptr(w), cout, cin, k, ptr(buf), stream))
        check(call[0](*call[1]), "pack conv2d")
        return buf, None, None, w, call

    def _live(self):
        """What a cached descriptor depends on: the storage of every parameter it points at (load_state_dict into
        the same tensors and .data.copy_ -- the EMA update -- keep storages, and the values are read per call; .to(),
        a replaced Parameter or a dtype change bring a new storage)."""
        return tuple(None if (t := d[n]) is None else t.data_ptr() for d, n in self._slots)

    def forward(self, x):
        """The whole encoder in one damc_q_encoder_fwd call (weights re-packed per call into reused buffers).  The
        descriptor, its workspace and its packing calls are cached per thread for one (device, stream, shape, engine,
        parameter storages) key: a repeated call issues the per-call packings (the fp32 first layer; every layer under
        DAMC_ENC_WSRC=0) and the library call only -- the host side of a call was as long as its kernels at CIFAR
        B=128."""
        L = _lib.lib()
        dev = x.device
        stream = _lib.stream_ptr(dev)
        B, C, H, W = x.shape
        key = (dev.index, stream, B, C, H, W, _lib.current_engine(), os.environ.get("DAMC_ENC_WSRC", "1"), self._live())
        hit = getattr(self._tls, "desc", None)
        if hit is not None and hit[0] == key:
            _, dref, nbytes, ws, calls, _ = hit
            for fn, args in calls:
                check(fn(*args), "pack conv2d")
            out = torch.empty(B, self._cout, dtype=torch.float32, device=dev)
            check(L.damc_q_encoder_fwd(dref, ptr(x), B, ptr(out), ptr(ws), nbytes, stream), "damc_q_encoder_fwd")
            return out
        if len(self.stages) > _lib.MAX_ENC_LAYERS:
            raise NotImplementedError("encoder with %d convolutions" % len(self.stages))
        d = _lib.Encoder()
        d.n_layers, d.nc, d.h, d.w = len(self.stages), C, H, W
        d.engine = _lib.current_engine()
        keep, calls, same = [], [], True
        for i, (conv, norm, slope) in enumerate(self.stages):
            k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            cout, cin = conv.out_channels, conv.in_channels
            wp, w3, wsrc, w, call = self._packed(i, conv, dev, L, stream)
            if call is not None:
                calls.append(call)
            bias = _dev(conv.bias, dev) if conv.bias is not None else None
            e = d.layers[i]
            e.cin, e.cout, e.k, e.stride, e.pad = cin, cout, k, s, p
            e.w_packed, e.bias, e.w_x3, e.w_src = ptr(wp), ptr(bias), ptr(w3), ptr(wsrc)
            keep += [bias, w, wp, w3]
            pairs = [(w, conv.weight), (bias, conv.bias)]
            if norm is not None:
                g, b = _dev(norm.weight, dev), _dev(norm.bias, dev)
                e.in_gamma, e.in_beta, e.in_eps, e.slope = ptr(g), ptr(b), float(norm.eps), slope
                keep += [g, b]
                pairs += [(g, norm.weight), (b, norm.bias)]
            # a pointer into a converted copy would go stale when the parameter's values change: no caching then
            same = same and all(a is None or a.data_ptr() == o.data_ptr() for a, o in pairs)
        nbytes = int(L.damc_q_encoder_workspace_bytes(ctypes.byref(d), B))
        if nbytes == 0:
            raise _lib.DamcError("unsupported encoder configuration for the HIP path")
        ws = self._ws.get(dev, nbytes, ("encoder", B, H, W))
        dref = ctypes.byref(d)
        # (the tuple keeps d, the workspace and every pointed-at buffer alive while the entry lives)
        self._tls.desc = (key, dref, nbytes, ws, calls, (d, keep)) if same else None
        out = torch.empty(B, self._cout, dtype=torch.float32, device=dev)
        check(L.damc_q_encoder_fwd(dref, ptr(x), B, ptr(out), ptr(ws), nbytes, stream), "damc_q_encoder_fwd")
        return out


# ----------------------------------------------------------------------------- denoiser
class DenoiserPlan:
    """Diffusion_UnetA (diffusion_net.py:463-533) as a damc_denoiser_t: pointers to the live parameters in their
    PyTorch layouts (the library re-lays them out into its workspace per call), plus a workspace cached per
    (batch, steps, device) so the library's cached HIP graph of the reverse sweep is reused across calls."""

    def __init__(self, p):
        self.p = p
        self.blocks = list(p.in_layers) + list(p.mid_layers) + list(p.out_layers)
        if len(self.blocks) != 7:
            raise NotImplementedError("Diffusion_UnetA with %d blocks" % len(self.blocks))
        self.nz, self.ntemb, self.nxemb = p.nz, p.ntemb, p.nxemb
        self._ws = None
        self._gws = None

    def pack(self, device):
        from .training import _denoiser_desc, _denoiser_params

        params = [_dev(t, device) for _, _, t in _denoiser_params(self.p)]
        self._keep = params  # copies (only if a parameter lives elsewhere) stay alive for the call
        return _denoiser_desc(self.p, params)

    def workspace(self, desc, B, n, device):
        nbytes = int(_lib.lib().damc_sweep_workspace_bytes(ctypes.byref(desc), B, n))
        if nbytes == 0:
            raise _lib.DamcError("unsupported denoiser configuration for the HIP path")
        if self._ws is None:
            self._ws = _lib.WorkspaceCache()
        return self._ws.get(device, nbytes, (int(B), int(n))), nbytes

    def guided_workspace(self, desc, B, n, device):
        """The guided sweep's workspace (its own cache: a guided and an unguided call do not evict each other), or
        (None, 0) where the library has no guided sweep for this denoiser."""
        nbytes = int(_lib.lib().damc_guided_sweep_workspace_bytes(ctypes.byref(desc), B, n))
        if nbytes == 0:
            return None, 0
        if self._gws is None:
            self._gws = _lib.WorkspaceCache()
        return self._gws.get(device, nbytes, (int(B), int(n))), nbytes


_ENC = weakref.WeakKeyDictionary()
_DEN = weakref.WeakKeyDictionary()


def mlp_desc(seq, device):
    """An nn.Sequential of Linear / ReLU / LeakyReLU as a damc_mlp_t over its live parameters (the toy's encoder and
    prior_emb, workspace/toy_example/src/diffusion_net.py:166-184).  Returns (descriptor, tensors to keep alive)."""
    d = _lib.Mlp()
    keep, n = [], 0
    mods = list(seq)
    i = 0
    while i < len(mods):
        lin = mods[i]
        if not isinstance(lin, torch.nn.Linear) or hasattr(lin, "weight_orig"):
            raise NotImplementedError("unexpected MLP module %r" % (lin,))
        if n >= _lib.MLP_MAX_LAYERS or max(lin.in_features, lin.out_features) > _lib.MLP_MAX_WIDTH:
            raise NotImplementedError("MLP with more than %d layers or a width over %d"
                                      % (_lib.MLP_MAX_LAYERS, _lib.MLP_MAX_WIDTH))
        act, slope = _lib.ACT_NONE, 0.0
        if i + 1 < len(mods) and not isinstance(mods[i + 1], torch.nn.Linear):
            a = mods[i + 1]
            if isinstance(a, torch.nn.ReLU):
                act = _lib.ACT_RELU
            elif isinstance(a, torch.nn.LeakyReLU):
                act, slope = _lib.ACT_LRELU, float(a.negative_slope)
            else:
                raise NotImplementedError("unexpected MLP activation %r" % (a,))
            i += 1
        i += 1
        w = _dev(lin.weight, device)
        b = _dev(lin.bias, device) if lin.bias is not None else None
        e = d.layers[n]
        e.din, e.dout, e.act, e.slope = lin.in_features, lin.out_features, act, slope
        e.w, e.bias = ptr(w), ptr(b)
        keep += [w, b]
        n += 1
    d.n_layers = n
    return d, keep


def mlp_forward(seq, x):
    """seq(x) for an nn.Sequential of Linear / ReLU / LeakyReLU in one damc_mlp_forward launch (no autograd)."""
    x = x.detach().to(dtype=torch.float32).contiguous()
    if x.device.type != "cuda":
        raise _lib.DamcError("MLP input must be on a ROCm device; the HIP path has no CPU fallback")
    d, keep = mlp_desc(seq, x.device)
    if x.dim() != 2 or x.shape[1] != d.layers[0].din:
        raise _lib.DamcError("MLP input must be (batch, %d)" % d.layers[0].din)
    out = torch.empty(x.shape[0], d.layers[d.n_layers - 1].dout, dtype=torch.float32, device=x.device)
    check(_lib.lib().damc_mlp_forward(ctypes.byref(d), ptr(x), x.shape[0], ptr(out), _lib.stream_ptr(x.device)),
          "damc_mlp_forward")
    return out


def encoder_forward(enc, x):
    if isinstance(enc, torch.nn.Sequential):  # the toy's MLP encoder (workspace/toy_example/src/diffusion_net.py:166-174)
        return mlp_forward(enc, x)
    plan = _ENC.get(enc)
    if plan is None:
        plan = _ENC[enc] = EncoderPlan(enc)
    x = x.detach().to(dtype=torch.float32).contiguous()
    if x.device.type != "cuda":
        raise _lib.DamcError("encoder input must be on a ROCm device; the HIP path has no CPU fallback")
    return plan.forward(x)


def prior_embedding(Q, noise):
    """prior_emb = Linear(nz,128) -> LeakyReLU(0.01) -> Linear(128,nxemb) (diffusion_net.py:577-581)."""
    if Q.nz % 4:  # K = nz off the GEMM's float4 rows (the toy, nz = 2): the fused MLP
        return mlp_forward(Q.prior_emb, noise)
    L = _lib.lib()
    dev = noise.device
    stream = _lib.stream_ptr(dev)
    l1, act, l2 = Q.prior_emb[0], Q.prior_emb[1], Q.prior_emb[2]
    w1, b1 = _dev(l1.weight, dev).t().contiguous(), _dev(l1.bias, dev)
    w2, b2 = _dev(l2.weight, dev).t().contiguous(), _dev(l2.bias, dev)
    B = noise.shape[0]
    h = torch.empty(B, l1.out_features, dtype=torch.float32, device=dev)
    out = torch.empty(B, l2.out_features, dtype=torch.float32, device=dev)
    check(L.damc_gemm(ptr(noise), l1.in_features, ptr(w1), l1.out_features, ptr(b1), ptr(h), l1.out_features, B,
                      l1.out_features, l1.in_features, _lib.ACT_LRELU, float(act.negative_slope), stream), "gemm")
    check(L.damc_gemm(ptr(h), l2.in_features, ptr(w2), l2.out_features, ptr(b2), ptr(out), l2.out_features, B,
                      l2.out_features, l2.in_features, _lib.ACT_NONE, 0.0, stream), "gemm")
    return out


def reverse_sweep(Q, xemb, zt, noise=None, seed=None, chain_base=0, eps_log_steps=0, with_noise=None, draws=None):
    """In-place latent reverse sweep on zt (B, nz); returns eps of the first eps_log_steps steps.

    draws (a damc.graphs.DrawState, instead of seed): the sweep's Philox key is read on the device
    (damc_reverse_sweep_ds), bitwise the seeded sweep with seed = the state's and its noisy step k at index counter + k;
    the counter is advanced by n_interval after the sweep is enqueued, so a captured sweep draws anew per replay."""
    from .graphs import exclusive

    exclusive(seed, draws, "reverse_sweep")
    dev = zt.device
    plan = _DEN.get(Q.p)
    if plan is None:
        plan = _DEN[Q.p] = DenoiserPlan(Q.p)
    d = plan.pack(dev)
    n = int(Q.n_interval)
    B = zt.shape[0]
    coef_h, temb_d = cached_step_tables(n, Q.logsnr_min, Q.logsnr_max, Q.var_type, plan.ntemb, dev)
    L = _lib.lib()
    ws, nbytes = plan.workspace(d, B, n, dev)
    with_noise = bool(Q.with_noise) if with_noise is None else bool(with_noise)
    if noise is not None:
        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
    if seed is None and draws is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if with_noise and noise is None else 0
    xemb = xemb.to(dtype=torch.float32).contiguous()
    eps_log = torch.empty(max(eps_log_steps, 1), B, plan.nz, dtype=torch.float32, device=dev) if eps_log_steps else None
    if draws is not None:
        check(L.damc_reverse_sweep_ds(ctypes.byref(d), ptr(xemb), ptr(zt), B, n, ptr(temb_d),
                                      coef_h.numpy().ctypes.data_as(ctypes.c_void_p), int(with_noise), ptr(noise),
                                      draws.ptr(), chain_base, ptr(eps_log), int(eps_log_steps), ptr(ws), nbytes,
                                      _lib.stream_ptr(dev)), "damc_reverse_sweep_ds")
        draws.advance(n)
        return eps_log
    check(L.damc_reverse_sweep(ctypes.byref(d), ptr(xemb), ptr(zt), B, n, ptr(temb_d),
                               coef_h.numpy().ctypes.data_as(ctypes.c_void_p), int(with_noise), ptr(noise), seed,
                               chain_base, ptr(eps_log), int(eps_log_steps), ptr(ws), nbytes, _lib.stream_ptr(dev)),
          "damc_reverse_sweep")
    return eps_log


STREAM_GUIDE = 0x54  # DAMC_STREAM_GUIDE (csrc/common.h): the Philox stream of the guided sweep's prior-embedding noise


def guided_sweep(Q, xemb, xemb_unc, zt, w, noise=None, seed=None, chain_base=0, eps_log_steps=0, with_noise=None,
                 draws=None):
    """In-place guided (classifier-free guidance, cond_w = w > 0) latent reverse sweep on zt (B, nz) in one
    damc_guided_sweep call; xemb (B, nxemb) the conditional embedding, xemb_unc (n, B, nxemb) the unconditional one of
    every step in sweep order.  Returns the guided eps of the first eps_log_steps steps.  Mirrors reverse_sweep, but
    for draws=: the guided sweep has no drawn variant."""
    if draws is not None:
        raise _lib.DamcError("guided_sweep(draws=...): the guided sweep has no device-resident draw state; use seed=")
    dev = zt.device
    plan = _DEN.get(Q.p)
    if plan is None:
        plan = _DEN[Q.p] = DenoiserPlan(Q.p)
    d = plan.pack(dev)
    n = int(Q.n_interval)
    B = zt.shape[0]
    coef_h, temb_d = cached_step_tables(n, Q.logsnr_min, Q.logsnr_max, Q.var_type, plan.ntemb, dev)
    L = _lib.lib()
    ws, nbytes = plan.guided_workspace(d, B, n, dev)
    if ws is None:
        raise _lib.DamcError("the guided sweep does not take this denoiser (its row image does not fit, or nz % 4 != 0)")
    with_noise = bool(Q.with_noise) if with_noise is None else bool(with_noise)
    if noise is not None:
        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if with_noise and noise is None else 0
    xemb = xemb.to(dtype=torch.float32).contiguous()
    xemb_unc = xemb_unc.to(dtype=torch.float32).contiguous()
    if xemb_unc.numel() != n * B * plan.nxemb or xemb.numel() != B * plan.nxemb:
        raise _lib.DamcError("xemb must be (%d, %d) and xemb_unc (%d, %d, %d)" % (B, plan.nxemb, n, B, plan.nxemb))
    eps_log = torch.empty(max(eps_log_steps, 1), B, plan.nz, dtype=torch.float32, device=dev) if eps_log_steps else None
    check(L.damc_guided_sweep(ctypes.byref(d), ptr(xemb), ptr(xemb_unc), float(w), ptr(zt), B, n, ptr(temb_d),
                              coef_h.numpy().ctypes.data_as(ctypes.c_void_p), int(with_noise), ptr(noise), seed,
                              chain_base, ptr(eps_log), int(eps_log_steps), ptr(ws), nbytes, _lib.stream_ptr(dev)),
          "damc_guided_sweep")
    return eps_log


def _guided_fits(Q, b, device):
    plan = _DEN.get(Q.p)
    if plan is None:
        plan = _DEN[Q.p] = DenoiserPlan(Q.p)
    return int(_lib.lib().damc_guided_sweep_workspace_bytes(ctypes.byref(plan.pack(device)), b, int(Q.n_interval))) > 0


def q_forward(Q, x=None, b=None, device=None, cond_w=-1, zt=None, seed=None, chain_base=0, draws=None):
    """_netQ_U.forward on the HIP path (diffusion_net.py:585-622).

    zt / seed / chain_base (not in the reference's signature; sharded callers only): the initial latent
    (default: torch.randn(b, nz) on the host generator, as the reference), the sweep's Philox key and the
    global index of row 0 — a shard that passes its slice of the global zt, the global seed and its slice
    start reproduces its rows of the 1-GPU sweep bit for bit.

    cond_w > 0 (classifier-free guidance, diffusion_net.py:595-620) runs the guided sweep, one launch sequence for
    all steps.  With a seed, the per-step prior-embedding noise is the library's Philox stream 0x54 keyed by the
    global chain index and the step noise the sweep's own in-kernel stream, so the same sharding rule holds; without
    one, torch's draws are taken in the reference's order (_q_forward_guided).

    draws (a damc.graphs.DrawState, instead of seed): reverse_sweep's; a caller that captures the call passes zt too
    (the default initial latent is a host-generator draw, which a graph would replay unchanged).  The guided sweep
    raises DamcError."""
    from .graphs import exclusive

    exclusive(seed, draws, "q_forward")
    if cond_w is not None and cond_w > 0 and x is not None:
        if draws is not None:
            raise _lib.DamcError("q_forward(draws=...): the guided sweep (cond_w > 0) has no device-resident draw "
                                 "state; use seed=")
        if Q.nz % 4:
            raise NotImplementedError("classifier-free guidance (cond_w > 0) is not implemented for nz % 4 != 0 "
                                      "(the toy amortizer): the guided sweep needs float4 rows")
        if seed is None:
            return _q_forward_guided(Q, x, float(cond_w), zt0=zt)
        return _q_forward_guided_seeded(Q, x, float(cond_w), zt, int(seed), int(chain_base))
    if x is not None:
        assert b is None and device is None
        b = len(x)
        device = x.device
        xemb = encoder_forward(Q.encoder, x)
    else:
        device = torch.device(device) if device is not None else torch.device("cuda")
        xemb = prior_embedding(Q, torch.randn(b, Q.nz, device=device))
    if zt is None:  # the reference's host-generator draw, copied without blocking the host (training.to_device_async)
        from .training import to_device_async

        zt = to_device_async(torch.randn(b, Q.nz), device)
    else:
        zt = zt.to(device=device, dtype=torch.float32).clone()
    if zt.device.type != "cuda":
        raise _lib.DamcError("the HIP sweep needs a ROCm device (got %s)" % zt.device)
    if zt.shape != (b, Q.nz):
        raise _lib.DamcError("zt must be (%d, %d)" % (b, Q.nz))
    reverse_sweep(Q, xemb, zt, seed=seed, chain_base=chain_base, draws=draws)
    return zt


def _initial_latent(Q, b, device, zt):
    if zt is None:  # the reference's host-generator draw
        return torch.randn(b, Q.nz).to(device)
    zt = zt.to(device=device, dtype=torch.float32).clone()
    if zt.shape != (b, Q.nz):
        raise _lib.DamcError("zt must be (%d, %d)" % (b, Q.nz))
    return zt


def _q_forward_guided(Q, x, w, eps_trace=None, zt0=None):
    """Classifier-free guidance (cond_w > 0, diffusion_net.py:595-620) on the guided sweep, with the reference's
    draws: torch's, taken before the sweep in the reference's order and with its calls (none depends on zt): the host
    randn(b, nz) for zt, then for i = n-1 .. 0 the device randn(b, nz) of the step's prior embedding and, for
    i != 0, the step's randn_like(zt).  All n prior embeddings are one prior_embedding call over n b rows, handed to
    damc_guided_sweep as xemb_unc with the step noise injected.  eps_trace (tests): a list that receives each step's
    guided eps.  A denoiser the guided sweep does not take runs the step loop (_q_forward_guided_steps)."""
    b, device, n = len(x), x.device, int(Q.n_interval)
    if device.type != "cuda":
        raise _lib.DamcError("the HIP sweep needs a ROCm device (got %s)" % device)
    if not _guided_fits(Q, b, device):
        return _q_forward_guided_steps(Q, x, w, eps_trace, zt0=zt0)
    xemb = encoder_forward(Q.encoder, x)
    zt = _initial_latent(Q, b, device, zt0)
    pe, steps = [], []
    for i in reversed(range(0, n)):
        pe.append(torch.randn(b, Q.nz, device=device))
        if i != 0:
            steps.append(torch.randn_like(zt))
    xemb_unc = prior_embedding(Q, torch.cat(pe, 0))
    noise = torch.stack(steps, 0) if steps and Q.with_noise else None
    eps = guided_sweep(Q, xemb, xemb_unc, zt, w, noise=noise, seed=0,
                       eps_log_steps=n if eps_trace is not None else 0)
    if eps_trace is not None:
        eps_trace.extend(eps[k].clone() for k in range(n))
    return zt


def _q_forward_guided_seeded(Q, x, w, zt, seed, chain_base):
    """The guided sweep on the library's Philox streams: the prior-embedding noise of (step k, row) is stream 0x54 at
    (seed, chain_base + row, k), the step noise the sweep's in-kernel stream.  Both are keyed by the global chain
    index, so a shard reproduces its rows of the whole batch's sweep bit for bit."""
    from .langevin import philox_normal

    b, device, n = len(x), x.device, int(Q.n_interval)
    if device.type != "cuda":
        raise _lib.DamcError("the HIP sweep needs a ROCm device (got %s)" % device)
    xemb = encoder_forward(Q.encoder, x)
    zt = _initial_latent(Q, b, device, zt)
    pn = philox_normal(n, b, Q.nz, seed, device, step_offset=0, chain_base=chain_base, stream_id=STREAM_GUIDE)
    xemb_unc = prior_embedding(Q, pn.view(n * b, Q.nz))
    guided_sweep(Q, xemb, xemb_unc, zt, w, seed=seed, chain_base=chain_base)
    return zt


def _q_forward_guided_steps(Q, x, w, eps_trace=None, zt0=None):
    """Classifier-free guidance (cond_w > 0, diffusion_net.py:595-620; round 5): the reference's step loop with its
    draws in its order (zt from the host generator, then per step a fresh prior embedding's noise and the step's
    noise on the device), each step's two denoiser evaluations on libdamc (Diffusion_UnetA.forward ->
    damc.training.denoiser_apply, the training kernels' forward) and the prior embedding on damc_gemm; the guidance
    combination and the schedule algebra are the reference's own tensor formulas (src/diffusion_helper_func.py).
    This runs one denoiser launch sequence per evaluation: it is the comparator of the guided sweep
    (_q_forward_guided) in the tests, and the path of a denoiser whose row image does not fit the guided sweep.
    eps_trace (tests): a list that receives each step's guided eps_pred.  zt0: the initial latent in place of the
    host draw (which is then not taken)."""
    from src.diffusion_helper_func import diffusion_reverse, logsnr_schedule_fn, pred_x_from_eps

    b, device, n = len(x), x.device, int(Q.n_interval)
    xemb = encoder_forward(Q.encoder, x)
    zt = torch.randn(b, Q.nz).to(device) if zt0 is None else zt0.to(device=device, dtype=torch.float32).clone()
    for i in reversed(range(0, n)):
        i_tensor = torch.ones(b, dtype=torch.float).to(device) * float(i)
        logsnr_t = logsnr_schedule_fn(i_tensor / (n - 1.0), logsnr_min=Q.logsnr_min, logsnr_max=Q.logsnr_max)
        logsnr_s = logsnr_schedule_fn(torch.clamp(i_tensor - 1.0, min=0.0) / (n - 1.0), logsnr_min=Q.logsnr_min,
                                      logsnr_max=Q.logsnr_max)
        eps_pred = Q.p(z=zt, logsnr=logsnr_t, xemb=xemb)
        xemb_unc = prior_embedding(Q, torch.randn(b, Q.nz, device=device))
        eps_pred_unc = Q.p(z=zt, logsnr=logsnr_t, xemb=xemb_unc)
        eps_pred = (1 + w) * eps_pred - w * eps_pred_unc
        if eps_trace is not None:
            eps_trace.append(eps_pred.clone())
        logsnr_t = logsnr_t.reshape((b, 1))
        logsnr_s = logsnr_s.reshape((b, 1))
        pred_z = pred_x_from_eps(z=zt, eps=eps_pred, logsnr=logsnr_t)
        if i == 0:
            zt = pred_z
        else:
            dist = diffusion_reverse(x=pred_z, z_t=zt, logsnr_s=logsnr_s, logsnr_t=logsnr_t, pred_var_type=Q.var_type)
            eps = torch.randn_like(zt)
            zt = dist["mean"] + dist["std"] * eps if Q.with_noise else dist["mean"]
    return zt
