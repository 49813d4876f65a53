"""CPU: the case tables of tests/train_ops_util.py hold what tests/test_gpu_train_ops.py relies on.

  * every denoiser case's fp64 reference keeps its LeakyReLU pre-activations clear of the kink, and an fp32 evaluation
    in another summation order (the batch permuted) meets the accuracy rule against fp64 on its own: the GPU test then
    needs no exclusion logic and its bound is not at the mercy of the reference's conditioning;
  * the route arithmetic the table's comments claim (gemm()'s K split, the grouped kernel's per-wave K runs) is mirrored
    in Python and pinned, so a change of those constants has to touch the table;
  * the host-side contract of the training calls (include/damc.h): workspace queries, argument, workspace, shape, slope
    and alignment refusals.  Everything here returns before a launch; the addresses are never dereferenced."""
import ctypes

import numpy as np
import pytest

import train_ops_util as T


def _L():
    from damc import _lib

    return _lib, _lib.lib()


# ------------------------------------------------------------------------------------------------ case-table pins
@pytest.mark.parametrize("cid", T.DN_IDS)
def test_denoiser_reference_stays_clear_of_the_kink(cid):
    m = T.dn_kink_margin(cid)
    print("%s kink margin %.3e" % (cid, m))
    assert m >= T.KINK_REL, (cid, m)


@pytest.mark.parametrize("cid", T.DN_IDS)
def test_denoiser_permuted_fp32_meets_the_rule(cid):
    r32, r64 = T.dn_refs(cid)
    names = T.dn_tensor_names(cid)
    assert len(names) == 3 + 68
    T.check_rows(cid + " permuted fp32", T.rule_rows(names, T.dn_permuted_fp32(cid), r32, r64, T.DN_FWD))


def test_d7_and_d8_share_net_and_leading_inputs():
    a, b = T.dn_case("D7"), T.dn_case("D8")
    for k in ("zt", "xemb", "se", "grad_eps"):
        assert np.array_equal(a[k][:16].numpy(), b[k].numpy()), k
    for u, v in zip(a["p"].parameters(), b["p"].parameters()):
        assert np.array_equal(u.detach().numpy(), v.detach().numpy())


@pytest.mark.parametrize("case", T.E_CASES, ids=T.case_id)
def test_e_reference_stays_clear_of_the_kink(case):
    m = T.seq_kink_margin(T.e_refs(case)[1]["_pre"])
    print("E %s kink margin %.3e" % (T.case_id(case), m))
    assert m >= T.KINK_REL


@pytest.mark.parametrize("case,slope", T.PE_CASES, ids=[T.case_id(c + (s,)) for c, s in T.PE_CASES])
def test_prior_emb_reference_stays_clear_of_the_kink(case, slope):
    m = T.seq_kink_margin(T.pe_refs(case, slope)[1]["_pre"])
    print("prior emb %s kink margin %.3e" % (T.case_id(case + (slope,)), m))
    assert m >= T.KINK_REL


# ------------------------------------------------------------------------------------------------ route arithmetic
@pytest.mark.parametrize("cid", sorted(T.DN_SPLITS))
def test_weight_gradient_split_is_as_the_table_says(cid):
    """Every K = B weight gradient of D1 / D5 (M = 2 dout rows of the stacked [dl | ds], N = din) takes the slab path
    (M <= 256, one output tile) with the table's slice count and ragged last slice; B % 4 != 0 keeps it off both
    float4 kernels."""
    B = T.DN_CASES[cid][4]
    assert B % 4 != 0 and B >= 97
    for din, dout in T.dn_widths(cid):
        for M, N in ((2 * dout, din), (2 * dout, dout)):
            assert M <= 256
            assert T.gemm_split(M, N, B) == T.DN_SPLITS[cid], (cid, M, N)
    # the activation products (M = B rows): D5's are past the slab limit, D1's have K tiles to split only where K >= 97
    assert T.gemm_split(514, 64, 128, slab=False) == (1, 128)
    assert T.gemm_split(130, 64, 24) == (1, 24)


def test_split_arithmetic_edges():
    assert T.gemm_split(128, 128, 96) == (1, 96)          # 3 K tiles: below the threshold
    assert T.gemm_split(128, 128, 97) == (2, 33)          # the first K that splits
    assert T.gemm_split(256, 128, 128) == (2, 64)         # D4 under DAMC_DN_SMALL_GEMM=0: aligned slices
    assert T.gemm_split(64, 64, 2048) == (16, 128)        # the slice cap


@pytest.mark.parametrize("K", sorted(T.GROUP_RUNS))
def test_grouped_kernel_wave_runs(K):
    runs = T.group_runs(K)
    assert runs == T.GROUP_RUNS[K] and sum(runs) == K
    busy = [r for r in runs if r]
    assert runs == tuple(busy) + (0,) * (4 - len(busy))  # idle waves come last
    assert len(set(busy[:-1])) <= 1 and all(r % 16 == 0 for r in busy[:-1]) and busy[-1] <= busy[0]


def test_tables_reach_the_idle_waves():
    assert T.group_runs(T.DN_CASES["D7"][4])[3] == 0 and T.group_runs(T.DN_CASES["D7"][4])[2] % 16
    assert T.group_runs(T.DN_CASES["D8"][4])[1:] == (0, 0, 0)
    assert T.group_runs(T.DN_CASES["D6"][0] // 2)[0] == 2
    assert any(T.group_runs(B)[3] == 0 for B, _, _ in T.E_CASES)
    assert T.E_CASES[1][2] % 16 == 8  # the 13th column tile, 8 wide


# ------------------------------------------------------------------------------------------------ host-only contract
FAKE = 1 << 20  # addresses handed to calls that return before any launch: never dereferenced


def _dn_desc(cid):
    p = T.dn_case(cid)["p"]
    names = T.dn_param_names(p)
    return p, T.dn_desc(p, lambda n, t: FAKE + 4096 * names.index(n))


def test_denoiser_host_contract():
    _lib, L = _L()
    p, d = _dn_desc("D6")
    B = T.DN_CASES["D6"][4]
    q = L.damc_denoiser_train_workspace_bytes
    nb = int(q(ctypes.byref(d), B))
    assert nb > 0 and nb % 256 == 0
    assert int(q(ctypes.byref(d), 2 * B)) > nb
    assert q(ctypes.byref(d), 0) == 0 and q(ctypes.byref(d), -4) == 0 and q(None, B) == 0
    # bad descriptors: odd nz, a wiring that is not Diffusion_UnetA's, a NULL weight
    for edit in ("nz", "din", "dout", "wl", "bctx", "bmat"):
        _, bad = _dn_desc("D6")
        if edit == "nz":
            bad.nz = 5
        elif edit == "din":
            bad.blocks[4].din += 4
        elif edit == "dout":
            bad.blocks[6].dout += 4
        elif edit == "wl":
            bad.blocks[3].wl = None
        elif edit == "bctx":
            bad.bctx[6] = None
        else:
            bad.bmat = None
        assert q(ctypes.byref(bad), B) == 0, edit
        assert L.damc_denoiser_train_forward(ctypes.byref(bad), FAKE, FAKE, FAKE, B, FAKE, FAKE, 1 << 30,
                                             None) == _lib.DAMC_ERR_ARG, edit
    ws = FAKE * 64
    fwd, bwd = L.damc_denoiser_train_forward, L.damc_denoiser_train_backward
    g = _lib.DenoiserGrads()
    for args in [(None, FAKE, FAKE, B, FAKE), (FAKE, None, FAKE, B, FAKE), (FAKE, FAKE, None, B, FAKE),
                 (FAKE, FAKE, FAKE, B, None), (FAKE, FAKE, FAKE, 0, FAKE)]:
        assert fwd(ctypes.byref(d), *args, ws, nb, None) == _lib.DAMC_ERR_ARG, args
    assert bwd(ctypes.byref(d), None, B, ctypes.byref(g), FAKE, FAKE, ws, nb, None) == _lib.DAMC_ERR_ARG
    assert bwd(ctypes.byref(d), FAKE, B, None, FAKE, FAKE, ws, nb, None) == _lib.DAMC_ERR_ARG
    assert fwd(ctypes.byref(d), FAKE, FAKE, FAKE, B, FAKE, ws, nb - 16, None) == _lib.DAMC_ERR_WORKSPACE
    assert fwd(ctypes.byref(d), FAKE, FAKE, FAKE, B, FAKE, None, nb, None) == _lib.DAMC_ERR_WORKSPACE
    assert bwd(ctypes.byref(d), FAKE, B, ctypes.byref(g), FAKE, FAKE, ws, nb - 16, None) == _lib.DAMC_ERR_WORKSPACE
    # the one alignment the denoiser calls require: the workspace's
    assert fwd(ctypes.byref(d), FAKE, FAKE, FAKE, B, FAKE, ws + 4, nb, None) == _lib.DAMC_ERR_UNSUPPORTED
    assert bwd(ctypes.byref(d), FAKE, B, ctypes.byref(g), FAKE, FAKE, ws + 8, nb, None) == _lib.DAMC_ERR_UNSUPPORTED


def _ebm(nz=8, nh=12, slope=0.2, **over):
    _lib, _ = _L()
    d = _lib.Ebm()
    d.nz, d.nh, d.slope = nz, nh, slope
    for i, k in enumerate(("w1", "b1", "w2", "b2", "w3", "b3")):
        setattr(d, k, over.get(k, FAKE + 4096 * i))
    return d


def _pe(nz=8, nh=12, nout=16, slope=0.01, **over):
    _lib, _ = _L()
    d = _lib.PriorEmb()
    d.nz, d.nh, d.nout, d.slope = nz, nh, nout, slope
    for i, k in enumerate(("w1", "b1", "w2", "b2")):
        setattr(d, k, over.get(k, FAKE + 4096 * i))
    return d


def test_ebm_train_host_contract():
    _lib, L = _L()
    q, fwd, bwd = L.damc_ebm_train_workspace_bytes, L.damc_ebm_train_forward, L.damc_ebm_train_backward
    B, ws = 8, FAKE * 64
    ok = _ebm()
    nb = int(q(ctypes.byref(ok), B))
    assert nb > 0 and q(None, B) == 0 and q(ctypes.byref(ok), 0) == 0
    g = _lib.EbmGrads()

    # each of these is given something that must be refused on the host: this suite also runs where a GPU is present,
    # and a call that launched would touch the made-up addresses
    def f(d, batch=B, z=FAKE, h1=FAKE):
        return fwd(ctypes.byref(d), z, batch, h1, FAKE, FAKE, None)

    def b(d, batch=B, wsp=ws):
        return bwd(ctypes.byref(d), FAKE, FAKE, FAKE, FAKE, 0, batch, ctypes.byref(g), FAKE, wsp, nb, None)

    def both(d, batch):
        return f(d, batch), b(d, batch)

    U = _lib.DAMC_ERR_UNSUPPORTED
    refused = {"B % 4": (ok, 6), "nz % 4": (_ebm(nz=6), B), "nh % 4": (_ebm(nh=10), B),
               "negative slope": (_ebm(slope=-0.2), B), "w1 + 4 B": (_ebm(w1=FAKE + 4), B),
               "w2 + 8 B": (_ebm(w2=FAKE + 8192 + 8), B), "w3 + 4 B": (_ebm(w3=FAKE + 16384 + 4), B)}
    for what, (d, batch) in refused.items():
        assert both(d, batch) == (U, U), what
        assert q(ctypes.byref(d), batch) == 0, what
    assert q(ctypes.byref(_ebm(b1=FAKE + 4, b2=FAKE + 4100, b3=FAKE + 8196)), B) == nb  # biases: any float address
    assert q(ctypes.byref(_ebm(slope=0.0)), B) == nb
    # the call's own pointers: the forward's float4 A rows, the backward's workspace
    assert f(ok, z=FAKE + 4) == U and f(ok, h1=FAKE + 4) == U and b(ok, wsp=ws + 4) == U
    assert fwd(ctypes.byref(ok), None, B, FAKE, FAKE, FAKE, None) == _lib.DAMC_ERR_ARG
    assert fwd(ctypes.byref(_ebm(w2=None)), FAKE, B, FAKE, FAKE, FAKE, None) == U  # a NULL weight: not a descriptor
    assert bwd(ctypes.byref(ok), FAKE, FAKE, FAKE, FAKE, 0, B, None, FAKE, ws, nb, None) == _lib.DAMC_ERR_ARG
    assert bwd(ctypes.byref(ok), FAKE, FAKE, FAKE, FAKE, -1, B, ctypes.byref(g), FAKE, ws, nb, None) == _lib.DAMC_ERR_ARG
    assert bwd(ctypes.byref(ok), FAKE, FAKE, FAKE, FAKE, 0, B, ctypes.byref(g), FAKE, ws, nb - 16,
               None) == _lib.DAMC_ERR_WORKSPACE
    assert bwd(ctypes.byref(ok), FAKE, FAKE, FAKE, FAKE, 0, B, ctypes.byref(g), FAKE, None, nb,
               None) == _lib.DAMC_ERR_WORKSPACE


def test_prior_emb_train_host_contract():
    _lib, L = _L()
    q = L.damc_prior_emb_train_workspace_bytes
    fwd, bwd = L.damc_prior_emb_train_forward, L.damc_prior_emb_train_backward
    B, ws = 8, FAKE * 64
    ok = _pe()
    nb = int(q(ctypes.byref(ok), B))
    assert nb > 0 and q(None, B) == 0 and q(ctypes.byref(ok), 0) == 0
    g = _lib.PriorEmbGrads()

    def f(d, batch=B, x=FAKE, h=FAKE):  # as above: only ever given something the host must refuse
        return fwd(ctypes.byref(d), x, batch, h, FAKE, None)

    def b(d, batch=B, go=FAKE, wsp=ws):
        return bwd(ctypes.byref(d), FAKE, FAKE, go, batch, ctypes.byref(g), wsp, nb, None)

    def both(d, batch):
        return f(d, batch), b(d, batch)

    U = _lib.DAMC_ERR_UNSUPPORTED
    refused = {"B % 4": (ok, 6), "nz % 4": (_pe(nz=6), B), "nh % 4": (_pe(nh=10), B), "nout % 4": (_pe(nout=18), B),
               "negative slope": (_pe(slope=-0.01), B), "w1 + 4 B": (_pe(w1=FAKE + 4), B),
               "w2 + 4 B": (_pe(w2=FAKE + 8192 + 4), B)}
    for what, (d, batch) in refused.items():
        assert both(d, batch) == (U, U), what
        assert q(ctypes.byref(d), batch) == 0, what
    assert q(ctypes.byref(_pe(slope=0.0)), B) == nb
    assert f(ok, x=FAKE + 4) == U and f(ok, h=FAKE + 8) == U
    assert b(ok, go=FAKE + 4) == U and b(ok, wsp=ws + 4) == U
    assert fwd(ctypes.byref(ok), None, B, FAKE, FAKE, None) == _lib.DAMC_ERR_ARG
    assert bwd(ctypes.byref(ok), FAKE, FAKE, FAKE, B, None, ws, nb, None) == _lib.DAMC_ERR_ARG
    assert bwd(ctypes.byref(ok), FAKE, FAKE, FAKE, B, ctypes.byref(g), ws, nb - 16, None) == _lib.DAMC_ERR_WORKSPACE


def test_q_glue_and_loss_refuse_bad_arguments():
    _lib, L = _L()
    A = _lib.DAMC_ERR_ARG
    f = ctypes.c_float
    assert L.damc_q_loss_forward(None, FAKE, 2, 4, FAKE, None) == A
    assert L.damc_q_loss_forward(FAKE, FAKE, 0, 4, FAKE, None) == A
    assert L.damc_q_loss_backward(FAKE, FAKE, FAKE, -1, 2, 4, FAKE, None) == A
    assert L.damc_q_loss_backward(FAKE, FAKE, None, 0, 2, 4, FAKE, None) == A
    assert L.damc_q_noise_glue(None, FAKE, FAKE, 2, 4, f(-5.1), f(9.8), FAKE, 8, None, FAKE, FAKE, None) == A
    assert L.damc_q_noise_glue(FAKE, FAKE, FAKE, 2, 4, f(-5.1), f(9.8), FAKE, 7, None, FAKE, FAKE, None) == A
    assert L.damc_q_noise_glue(FAKE, FAKE, FAKE, 2, 4, f(-5.1), f(9.8), FAKE, 8, None, None, FAKE, None) == A
