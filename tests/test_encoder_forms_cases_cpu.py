"""CPU: the cases of tests/test_gpu_encoder_forms.py (encoder_ops_util.FWD_CASES) reach every kernel instantiation of
csrc/enc_norm.hip, csrc/enc_first.hip and csrc/enc_head.hip that a damc_q_encoder_fwd call on an Encoder_* module can
launch.  encoder_ops_util.forward_kernels restates the forward's dispatch predicates (first_fused, one, mf, px, in1,
strip, f32a_layer, head_geom); the instantiations no module reaches are named below with the reason."""
import pytest

import encoder_ops_util as U

# not launched by any Encoder_* forward
UNREACHED = {
    "in_fused_x3_kernel<2>": "needs 64 < hw <= 128 after a conv; the k4 s2 p1 chains that end at 1 x 1 pass 256, 64, "
                             "16 (196, 49, 9 from 28 x 28)",
    "in_apply_train_kernel": "the training forward (damc_instnorm_lrelu_train_nhwc), never the inference forward",
    "in_bwd_sums_kernel": "the norm's backward (damc_instnorm_lrelu_backward_nhwc)",
    "in_bwd_apply_kernel": "the norm's backward (damc_instnorm_lrelu_backward_nhwc)",
}


def _kernels(case):
    name, hw, nc, nif, sw, engine = case
    return U.forward_kernels(U.enc_layers(name, nc, nif), hw, hw, U.FWD_B, sw, engine)


def test_the_universe_is_36_instantiations():
    assert len(U.FWD_KERNELS) == len(set(U.FWD_KERNELS)) == 36
    assert set(UNREACHED) <= set(U.FWD_KERNELS)


def test_cases_cover_every_reachable_instantiation():
    reached = set()
    for case in U.FWD_CASES:
        ks = _kernels(case)
        assert set(ks) <= set(U.FWD_KERNELS), (case, set(ks) - set(U.FWD_KERNELS))
        reached |= set(ks)
    assert reached == set(U.FWD_KERNELS) - set(UNREACHED), (sorted(set(U.FWD_KERNELS) - set(UNREACHED) - reached),
                                                             sorted(reached & set(UNREACHED)))


def test_case_ids_are_unique():
    ids = [U.fwd_case_id(c) for c in U.FWD_CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case,want", [
    (("cifar10", 32, 3, 64, {}, "limb"),
     ["conv3_in_fused_kernel<3>", "in_fused_x3_kernel<4>", "in_fused_x3_kernel<1>", "in_fused_x3_kernel<1>",
      "enc_head_x3_kernel<4>", "enc_head_reduce_kernel"]),
    (("cifar10", 32, 3, 64, {"IN_ONEPASS": "0"}, "limb"),
     ["conv3_in_fused_kernel<3>", "in_strip_stats_kernel", "in_merge_kernel", "in_apply_f32_kernel",
      "in_stats_kernel", "in_merge_kernel", "in_apply_f32_kernel", "in_stats_kernel", "in_merge_kernel",
      "in_apply_x3_kernel"]),
    (("mnist", 28, 1, 64, {"FIRST_ONEPASS": "0"}, "limb"),
     ["conv3_stats_kernel<1, 4>", "in_merge_kernel", "conv3_apply_x3_kernel<1, 1>", "in_fused_x3_kernel<4>",
      "in_fused_x3_kernel<1>", "in_fused_x3_kernel<1>", "enc_head_x3_kernel<4>", "enc_head_reduce_kernel"]),
    (("celeba64", 64, 3, 64, {}, "limb"),
     ["conv3_mfma_kernel<3, 4, true>", "in_merge_kernel", "conv3_mfma_kernel<3, 4, false>", "in_strip_stats_kernel",
      "in_merge_kernel", "in_apply_f32_kernel", "in_fused_x3_kernel<4>", "in_fused_x3_kernel<1>",
      "in_fused_x3_kernel<1>", "enc_head_x3_kernel<4>", "enc_head_reduce_kernel"]),
    (("cifar10", 32, 3, 64, {}, "fp32"), ["in_stats_pivot_kernel", "in_apply_kernel"] * 4),
], ids=lambda v: U.fwd_case_id(v) if isinstance(v, tuple) else "")
def test_launch_lists_of_the_named_cases(case, want):
    """Five launch lists written out: one per first-layer form and norm form, and the fp32 engine's."""
    assert _kernels(case) == want


@pytest.mark.parametrize("name,nc", [("cifar10", 3), ("cifar10", 4), ("mnist", 1), ("celeba64", 3), ("celeba64", 1),
                                     ("celebaHQ", 3)])
def test_layer_lists_match_the_modules(name, nc):
    from src import diffusion_net as dn

    enc = getattr(dn, "Encoder_" + name)(nc=nc, nemb=U.FWD_NEMB, nif=8)
    assert U.module_layers(enc) == U.enc_layers(name, nc, 8)


def test_the_full_width_strip_norm_takes_its_statistics_in_the_conv_epilogue():
    """CelebA-HQ at B = 8 (tests/test_gpu_configs.py): the convs before the 16384- and 4096-pixel strip norms fill the
    chip and run unsplit, so only the 1024-pixel one is followed by in_strip_stats_kernel; at B = 2 all convs split."""
    full = U.forward_kernels(U.enc_layers("celebaHQ", 3, 64, 1024), 256, 256, 8)
    assert full.count("in_strip_stats_kernel") == 1 and full.count("in_merge_kernel") == 4
    assert full.count("in_apply_f32_kernel") == 3 and "in_stats_kernel" not in full
