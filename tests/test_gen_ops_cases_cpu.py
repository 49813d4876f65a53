"""CPU: the case table of tests/gen_ops_util.py holds what tests/test_gpu_gen_ops.py relies on.

  * the routes the table names, from the route arithmetic of csrc/generator.hip, csrc/wgrad.hip, csrc/gemm.h and
    csrc/smallc.hip restated in Python: a case that stopped landing where the table says fails here, and where the
    library exports the rule (damc_x3_layer_sign_block, damc_generator_layer_packed_sizes) the restatement is compared
    with it;
  * conditioning: no fp64 pre-activation of an activated layer within KINK_REL x its layer's RMS of zero, and the fp32
    reference within 1e-4 of fp64 per tensor, so the 3 x rule is neither at the mercy of a flipped LeakyReLU nor loose;
  * the host-side contract of the G update's calls (include/damc.h).  Everything here returns before a launch; the
    addresses are never dereferenced."""
import ctypes

import numpy as np
import pytest

import gen_ops_util as U


def _L():
    from damc import _lib

    return _lib, _lib.lib()


# ------------------------------------------------------------------------------------------------ the route table
@pytest.mark.parametrize("cid", list(U.CASES))
def test_padded_batch(cid):
    assert U.bp_of(U.CASES[cid]["B"]) == U.BP[cid]
    assert U.bp_of(1) == 32 and U.bp_of(32) == 32 and U.bp_of(33) == 64


def test_layer_kinds_and_maps():
    kinds = lambda cid: [s["kind"] for s in U.layer_specs(cid)]  # noqa: E731
    assert kinds("G2") == [U.PROJ, U.UP2, U.UP2, U.SMALLC]
    assert kinds("G6a") == [U.PROJ, U.SMALLC] and kinds("G8") == [U.LINEAR] * 4
    assert [s["hout"] for s in U.layer_specs("G5")] == [7, 14, 28, 28]
    assert [s["hout"] for s in U.layer_specs("G6a")] == [28, 28]
    assert [s["hout"] for s in U.layer_specs("G6b")] == [32, 32]
    assert [s["hout"] for s in U.layer_specs("G3")] == [4, 8, 16, 32]
    assert U.layer_specs("G6a")[0]["act"] == U.ACT_NONE and U.layer_specs("G6b")[0]["act"] == U.ACT_NONE
    assert [s["bias"] for s in U.layer_specs("G5")] == [True, False, True, True]
    g8 = U.layer_specs("G8")
    assert [(s["act"], s["slope"]) for s in g8] == [(U.ACT_LRELU, 0.0)] * 3 + [(U.ACT_NONE, 0.0)]


@pytest.mark.parametrize("cid", sorted(U.SMALLC_ROWS))
def test_output_layer_row_blocks(cid):
    L, B = U.layer_specs(cid)[-1], U.CASES[cid]["B"]
    assert U.smallc_rows(L, B) == U.SMALLC_ROWS[cid]
    blocks = U.smallc_row_blocks(L, B)
    assert sum(blocks) == L["hin"]
    if cid == "G6a":
        assert blocks == [8, 8, 8, 4]          # the multi-row window with a short last block
    if cid == "G6b":
        assert blocks == [4] * 8


def test_output_layer_templates():
    """(Cout, k) of every case's output layer: each SW(NC, K) instantiation but SW(2, 4), SW(1, 4) and SW(4, 3)."""
    got = {cid: (U.layer_specs(cid)[-1]["cout"], U.layer_specs(cid)[-1]["k"]) for cid in U.SMALLC_ROWS}
    assert got["G6c"] == (4, 4) and got["G6d"] == (2, 3) and got["G3"] == (3, 4) and got["G2"] == (3, 3)
    assert got["G1"] == (1, 3)


@pytest.mark.parametrize("cid", sorted(U.DZ_SLICES))
def test_first_layer_input_gradient_slices(cid):
    S, kp, run = U.dz_split(U.layer_specs(cid))
    assert (S, kp, run) == U.DZ_SLICES[cid]
    if cid in ("G5", "G6a"):
        assert run < S      # the zeroed slab tail
    else:
        assert run == S


def test_slice_arithmetic_edges():
    assert U.proj_slices(255) == 1 and U.proj_slices(512) == 2 and U.proj_slices(1 << 20) == 512
    assert U.proj_k_per(3136, 12) == 288 and U.proj_k_per(6272, 24) == 288 and U.proj_k_per(8192, 32) == 256


@pytest.mark.parametrize("cid", sorted(U.OUT_COLSUM))
def test_output_bias_column_sum_passes(cid):
    L, B = U.layer_specs(cid)[-1], U.CASES[cid]["B"]
    R, C, passes = U.OUT_COLSUM[cid]
    assert (B * L["hout"] * L["hout"], L["cout"]) == (R, C)
    assert U.colsum_passes(R, C) == passes
    # the threshold the issue states: two passes above 8 * 16 * (256 / lanes) rows
    lanes = U.colsum_lanes(C)
    if C % 4:
        assert (R > 8 * 16 * (256 // lanes)) == (passes == 2)


def test_which_other_column_sums_take_two_passes():
    """Hidden-layer bias gradients sum (pixels x Bp / 32) partial rows; the output layer's weight gradient sums one row
    per block: which of them take two passes is part of what the cases run."""
    two = {}
    for cid in U.RUN_IDS:
        specs, B = U.layer_specs(cid), U.CASES[cid]["B"]
        nb = U.bp_of(B) // 32
        for i, L in enumerate(specs):
            if L["kind"] == U.UP2 and L["bias"]:
                two[(cid, "b%d" % i)] = U.colsum_passes(4 * L["hin"] ** 2 * nb, L["cout"])
            elif L["kind"] == U.PROJ and L["bias"]:
                two[(cid, "b%d" % i)] = U.colsum_passes(L["hout"] ** 2 * nb, L["cout"])
            elif L["kind"] == U.SMALLC:
                blocks = B * len(U.smallc_row_blocks(L, B))
                two[(cid, "w%d" % i)] = U.colsum_passes(blocks, L["k"] ** 2 * L["cout"] * L["cin"])
    # all four on the float4 kernel (C % 4 == 0): 12 544 and 8192 partial rows of 8 channels; 2048 blocks of 72 and
    # 216 columns; G2's 528 blocks of 864 columns (more than 32 rows for each of the 16 row lanes)
    assert {k for k, v in two.items() if v == 2} == {("G6a", "b0"), ("G6b", "b0"), ("G6a", "w1"), ("G6b", "w1"),
                                                     ("G2", "w3")}


def test_limb_capabilities():
    for cid, caps in U.X3_CAPS.items():
        ups = [L for L in U.layer_specs(cid) if L["kind"] == U.UP2]
        assert [(U.x3_fwd_cap(L), U.x3_bwd_cap(L)) for L in ups] == caps, cid
    for cid, want in U.X3_PROJ.items():
        assert U.x3_proj_cap(U.layer_specs(cid)[0]) == want, cid
    for cid, want in U.HBITS.items():
        specs = U.layer_specs(cid)
        assert [U.hbits_cap(specs, j) for j in range(len(specs) - 1)] == want, cid
    assert U.CASES["G3"]["nz"] % 32 and U.CASES["G5"]["nz"] % 32 and U.CASES["G1"]["nz"] % 32


def test_limb_capability_matches_the_library():
    """damc_generator_layer_packed_sizes carries a limb copy exactly where the capability holds, and
    damc_x3_layer_sign_block is non-zero there: the Python predicates against the library's own."""
    _lib, L = _L()
    for cid in ("G1", "G2", "G3", "G4", "G5"):
        g = U.host_descriptor(cid)
        for i, s in enumerate(U.layer_specs(cid)):
            n = s["cin"] * s["cout"] * s["k"] ** 2
            f, b = ctypes.c_size_t(), ctypes.c_size_t()
            assert L.damc_generator_layer_packed_sizes(ctypes.byref(g.layers[i]), ctypes.byref(f), ctypes.byref(b)) == 0
            if s["kind"] == U.UP2:
                assert (f.value > n, b.value > n) == (U.x3_fwd_cap(s), U.x3_bwd_cap(s)), (cid, i)
                P = s["hin"] ** 2
                for ig, cap, nk in ((0, U.x3_fwd_cap(s), U.x3_conv_negk(P, s["cout"], 4 * s["cin"], 4)),
                                    (1, U.x3_bwd_cap(s), U.x3_conv_negk(P, s["cin"], 16 * s["cout"], 1))):
                    assert L.damc_x3_layer_sign_block(ctypes.byref(g.layers[i]), ig) == (nk if cap else 0), (cid, i, ig)
            elif s["kind"] == U.PROJ:
                assert (b.value > n) == U.x3_proj_cap(s), (cid, i)


def test_g4_splits_k_and_g2_does_not_need_to():
    L = U.layer_specs("G4")[1]
    assert (L["cin"], L["cout"], L["hin"]) == (256, 64, 4)
    assert U.up2_ksplits(L, U.CASES["G4"]["B"]) == (4, 4)       # K = 1024 both ways, four sign blocks of 256
    assert U.x3_conv_negk(16, 64, 1024, 4) == 256 and U.x3_conv_negk(16, 256, 1024, 1) == 256
    L5 = U.layer_specs("G5")[1]
    assert not U.x3_tapshare_ok(L5["hin"], L5["hin"]) and U.x3_tapshare_ok(4, 4) and U.x3_tapshare_ok(16, 16)


def test_up2_weight_gradient_split_and_reduce_kernel():
    for cid in U.RUN_IDS:
        Bp = U.bp_of(U.CASES[cid]["B"])
        for L in U.layer_specs(cid):
            if L["kind"] != U.UP2:
                continue
            S, kp = U.up2_wgrad_split(L, Bp)
            K = L["hin"] ** 2 * Bp
            assert kp % 32 == 0 and S * kp >= K and (S - 1) * kp < K and 1 <= S <= 16, (cid, S, kp)
    g1 = U.layer_specs("G1")[1]
    assert g1["cout"] % 16 == 8                                    # up2_wgrad_reduce_any_kernel
    assert U.up2_wgrad_split(g1, 32) == (4, 32)
    assert U.up2_wgrad_split(U.layer_specs("G2")[1], 64) == (16, 64)


def test_first_layer_routes():
    """PROJ forward: the limb engine (nz % 32 == 0, limb), else the K-major engine (nz % 32 == 0), else
    launch_small_gemm (nz % 4 == 0): the counts the GPU file asserts."""
    for cid, small in (("G1", 1), ("G3", 1), ("G5", 1), ("G6a", 1), ("G2", 0), ("G4", 0)):
        for _, eng in U.ENGINES:
            c = U.expected_counts(cid, eng)
            assert c["small_gemm"] == small and c["proj_fwd"] == 1, (cid, eng)
    lim, f32 = (U.expected_counts("G2", e) for _, e in U.ENGINES)
    # G2 on limbs: z split once, every later operand written by an epilogue or a limbs-only dgrad
    assert lim["split_x3"] == 1 and f32["split_x3"] == 0
    assert lim["upconv_fwd"] == lim["upconv_dgrad"] == lim["wgrad_up2"] == lim["wgrad_reduce"] == 2
    g3 = U.expected_counts("G3", U.ENGINE_LIMB)
    assert g3["split_x3"] == 1            # h0 for the 32 -> 16 forward; no dgrad reads limbs
    g5 = U.expected_counts("G5", U.ENGINE_LIMB)
    assert g5["split_x3"] == 2 and g5["bias_grad"] == 4   # h0, and the 64 -> 32 dgrad's fp32 operand; no b1
    g8 = U.expected_counts("G8", U.ENGINE_FP32)
    assert [g8[k] for k in ("proj_fwd", "linear_out", "linear_wgrad", "linear_dgrad", "bias_grad")] == [3, 1, 4, 3, 4]


def test_contract_case_is_the_n_mod_8_refusal():
    specs = U.layer_specs(U.CONTRACT_ID)
    assert specs[-2]["kind"] == U.UP2 and specs[-2]["cout"] == 4
    assert not U.train_supported(specs, U.CASES[U.CONTRACT_ID]["B"])
    for cid in U.RUN_IDS:
        assert U.train_supported(U.layer_specs(cid), U.CASES[cid]["B"]), cid


# ------------------------------------------------------------------------------------------------ conditioning
_SMALL = [c for c in U.RUN_IDS]


@pytest.mark.parametrize("cid", _SMALL)
def test_reference_stays_clear_of_the_kink(cid):
    m = U.kink_margin(cid)
    print("%s kink margin %.3e" % (cid, m))
    assert m >= U.KINK_REL, (cid, m)
    if cid in ("G6a", "G6b"):
        assert m == float("inf")   # no activated hidden layer


@pytest.mark.parametrize("cid", _SMALL)
def test_fp32_reference_is_close_to_fp64(cid):
    c = U.case(cid)
    rows = U.rule_rows(c["names"], c["ref32"], c["ref32"], c["ref64"], U.FWD)
    for n, _, e32 in rows:
        print("%-4s %-8s fp32-fp64 %.3e" % (cid, n, e32))
    assert all(np.isfinite(e32) and e32 <= 1e-4 for _, _, e32 in rows), rows
    assert any(e32 > 0 for _, _, e32 in rows)


# ------------------------------------------------------------------------------------------------ host-only contract
FAKE = 1 << 20  # addresses handed to calls that return before any launch: never dereferenced


def test_generator_train_host_contract():
    _lib, L = _L()
    q, fwd, bwd = (L.damc_generator_train_workspace_bytes, L.damc_generator_train_forward,
                   L.damc_generator_train_backward)
    g = U.host_descriptor("G1")
    B = U.CASES["G1"]["B"]
    nb = int(q(ctypes.byref(g), B))
    assert nb > 0 and nb % 256 == 0 and int(q(ctypes.byref(g), 33)) > nb
    assert q(ctypes.byref(g), 0) == 0 and q(ctypes.byref(g), -3) == 0 and q(None, B) == 0
    gr = _lib.GeneratorGrads()
    ws = FAKE * 64
    A, W = _lib.DAMC_ERR_ARG, _lib.DAMC_ERR_WORKSPACE
    for batch in (0, -1):
        assert fwd(ctypes.byref(g), FAKE, batch, FAKE, ws, nb, None) == A
        assert bwd(ctypes.byref(g), FAKE, FAKE, FAKE, batch, ctypes.byref(gr), FAKE, ws, nb, None) == A
    assert fwd(ctypes.byref(g), FAKE, B, FAKE, None, nb, None) == W
    assert fwd(ctypes.byref(g), FAKE, B, FAKE, ws, nb - 1, None) == W
    assert bwd(ctypes.byref(g), FAKE, FAKE, FAKE, B, ctypes.byref(gr), FAKE, None, nb, None) == W
    assert bwd(ctypes.byref(g), FAKE, FAKE, FAKE, B, ctypes.byref(gr), FAKE, ws, nb - 1, None) == W
    assert fwd(ctypes.byref(g), None, B, FAKE, ws, nb, None) == A
    assert fwd(ctypes.byref(g), FAKE, B, None, ws, nb, None) == A
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert bwd(ctypes.byref(g), *args, B, ctypes.byref(gr), FAKE, ws, nb, None) == A
    assert bwd(ctypes.byref(g), FAKE, FAKE, FAKE, B, None, FAKE, ws, nb, None) == A
    # a backward on a workspace no forward has recorded
    assert bwd(ctypes.byref(g), FAKE, FAKE, FAKE, B, ctypes.byref(gr), FAKE, ws, nb, None) == A
    # a descriptor validate() refuses: two engines in one generator
    bad = U.host_descriptor("G1")
    bad.layers[1].engine = U.ENGINE_FP32
    assert q(ctypes.byref(bad), B) == 0 and fwd(ctypes.byref(bad), FAKE, B, FAKE, ws, nb, None) == A


@pytest.mark.parametrize("engine", [e for _, e in U.ENGINES])
def test_contract_case_is_refused_on_the_host(engine):
    """G7's last hidden layer has 4 channels; launch_wgrad_x3 takes N in whole octets.  The refusal used to come half
    way through the backward (after out_delta and the output layer's kernels, with the train record consumed); now the
    workspace query returns 0 and both calls return DAMC_ERR_UNSUPPORTED before any launch, while the plain forward's
    workspace query still answers."""
    _lib, L = _L()
    g = U.host_descriptor(U.CONTRACT_ID, engine)
    B = U.CASES[U.CONTRACT_ID]["B"]
    assert L.damc_generator_train_workspace_bytes(ctypes.byref(g), B) == 0
    assert int(L.damc_posterior_workspace_bytes(ctypes.byref(g), B)) > 0
    gr = _lib.GeneratorGrads()
    Un = _lib.DAMC_ERR_UNSUPPORTED
    assert L.damc_generator_train_forward(ctypes.byref(g), FAKE, B, FAKE, FAKE * 64, 1 << 30, None) == Un
    assert L.damc_generator_train_backward(ctypes.byref(g), FAKE, FAKE, FAKE, B, ctypes.byref(gr), FAKE, FAKE * 64,
                                           1 << 30, None) == Un
    # the same topology with 8 channels there is taken; a first layer whose Cout k0 k0 is no multiple of 8 is not
    ok = U.host_descriptor(U.CONTRACT_ID, engine)
    ok.layers[2].cout = ok.layers[3].cin = 8
    assert int(L.damc_generator_train_workspace_bytes(ctypes.byref(ok), B)) > 0
    p = U.host_descriptor("G1", engine)
    p.layers[0].cout = p.layers[1].cin = 4
    p.layers[0].k = p.layers[0].hout = p.layers[0].wout = p.layers[1].hin = p.layers[1].win = 1
    p.layers[1].hout = p.layers[1].wout = p.layers[2].hin = p.layers[2].win = p.layers[2].hout = p.layers[2].wout = 2
    p.h = p.w = 2
    assert int(L.damc_posterior_workspace_bytes(ctypes.byref(p), B)) > 0
    assert L.damc_generator_train_workspace_bytes(ctypes.byref(p), B) == 0
