"""GPU: every form of damc_q_encoder_fwd's own dispatch, through amortizer.encoder_forward on Encoder_* modules at
nemb = 128, B = 2 (encoder_ops_util.FWD_CASES: each DAMC_ENC_* switch setting that changes which kernel runs, at the
smallest image that reaches the form; tests/test_encoder_forms_cases_cpu.py shows that together they launch every kernel
instantiation a module can reach).  The packing's status word is on (DAMC_ENC_PACK_CHECK=1).  Every xemb is held to the
fp64 evaluation of the module by the project's rule, test_gpu_configs._check with floor 1e-7: its distance to fp64 at
most 3 x the fp32 PyTorch-CPU evaluation's, plus 1e-7.  The two references of a module are computed once and shared by
its switch settings."""
import copy
import functools

import pytest
import torch

import encoder_ops_util as U
from test_gpu_configs import _check

pytestmark = pytest.mark.gpu

SWITCHES = ("FIRST_ONEPASS", "FIRST_MFMA", "FIRST_PX", "IN_ONEPASS", "IN_STRIP", "F32A", "HEAD", "HEAD_PD")


@functools.lru_cache(maxsize=None)
def _module(name, hw, nc, nif):
    """(module on the CPU, x, fp32 reference, fp64 reference); the references are never written to."""
    from damc import synth
    from oracle import damc_oracle as orc
    from src import diffusion_net as dn

    enc = synth.load_into(getattr(dn, "Encoder_" + name)(nc=nc, nemb=U.FWD_NEMB, nif=nif), 3).eval()
    x = torch.from_numpy(synth.uniform_f32(13, 6, (U.FWD_B, nc, hw, hw)))
    with torch.no_grad():
        e32 = orc.encoder_forward(enc, x).numpy()
        e64 = orc.encoder_forward(copy.deepcopy(enc).double(), x.double()).numpy()
    e32.setflags(write=False)
    e64.setflags(write=False)
    return enc, x, e32, e64


@functools.lru_cache(maxsize=None)
def _on_device(name, hw, nc, nif, device):
    enc, x, _, _ = _module(name, hw, nc, nif)
    return copy.deepcopy(enc).to(device).eval(), x.to(device)


def forward(case, device, monkeypatch):
    """xemb of one case as a numpy array: the case's switches set, every other one of SWITCHES unset."""
    from damc import _lib, amortizer

    name, hw, nc, nif, sw, engine = case
    enc, x = _on_device(name, hw, nc, nif, str(device))
    monkeypatch.setenv("DAMC_ENC_PACK_CHECK", "1")
    for key in SWITCHES:
        monkeypatch.delenv("DAMC_ENC_" + key, raising=False)
    for key, v in sw.items():
        assert key in SWITCHES
        monkeypatch.setenv("DAMC_ENC_" + key, v)
    if engine == "fp32":
        with _lib.exact_fp32():
            return amortizer.encoder_forward(enc, x).cpu().numpy()
    return amortizer.encoder_forward(enc, x).cpu().numpy()


@pytest.mark.parametrize("case", U.FWD_CASES, ids=U.fwd_case_id)
def test_forward_form_vs_fp64(gpu_device, monkeypatch, case):
    name, hw, nc, nif, sw, engine = case
    _, _, e32, e64 = _module(name, hw, nc, nif)
    got = forward(case, gpu_device, monkeypatch)
    assert got.shape == (U.FWD_B, U.FWD_NEMB)
    _check("Encoder_%s xemb, %s" % (name, U.fwd_case_id(case)), got, e32, e64, 1e-7)
