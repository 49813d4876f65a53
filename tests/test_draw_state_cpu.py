"""CPU: the host side of the device-resident draw state and of the capturable optimiser (no kernel is launched).

The drawn (_ds) entry points and damc_draw_state_advance are exported and bound; a NULL state is refused on the host,
before any launch, whatever the other arguments are; damc.optim.Adam / AdamW construct with capturable=True (and a
tensor lr) while amsgrad still raises; every wrapper refuses draws= together with seed=."""
import ctypes

import pytest
import torch

DS_SYMBOLS = ("damc_draw_state_advance", "damc_posterior_langevin_ds", "damc_prior_langevin_ds", "damc_z_update_ds",
              "damc_philox_normal_ds", "damc_philox_uniform_ds", "damc_q_noise_glue_seeded_ds", "damc_reverse_sweep_ds",
              "damc_adam_step_capturable")


def test_new_symbols_are_exported_and_bound():
    from damc import _lib

    so = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name in DS_SYMBOLS:
        assert hasattr(so, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.damc_abi_version() == _lib.ABI_VERSION == 3  # additive: the ABI version stays


def test_null_state_is_refused_on_the_host():
    """state == NULL -> DAMC_ERR_ARG.  The other pointers are NULL or not device memory: a launch would fail with a
    HIP error instead (and this test has no device), so 1001 shows the check comes first."""
    from damc import _lib

    L = _lib.lib()
    g, e, d = _lib.Generator(), _lib.Ebm(), _lib.Denoiser()
    assert L.damc_draw_state_advance(None, 1, None) == _lib.DAMC_ERR_ARG
    assert L.damc_posterior_langevin_ds(ctypes.byref(g), ctypes.byref(e), 8, 8, 4, 1, 0.1, 0.1, 1, None, None, 0, 0,
                                        None, 8, 64, None) == _lib.DAMC_ERR_ARG
    assert L.damc_prior_langevin_ds(ctypes.byref(e), 8, 4, 1, 0.1, 1, None, None, 0, 0, None, 1,
                                    None) == _lib.DAMC_ERR_ARG
    assert L.damc_z_update_ds(8, 8, 4, 4, 0.1, 1, None, None, 0, 0, None) == _lib.DAMC_ERR_ARG
    assert L.damc_philox_normal_ds(8, 1, 4, 4, None, 0, 0, 0x51, None) == _lib.DAMC_ERR_ARG
    assert L.damc_philox_uniform_ds(8, 1, 4, None, 0, 0, 0x55, None) == _lib.DAMC_ERR_ARG
    assert L.damc_q_noise_glue_seeded_ds(8, 4, 4, -5.1, 9.8, 8, 16, None, 0, 0, None, 8, None, 8, 8,
                                         None) == _lib.DAMC_ERR_ARG
    assert L.damc_reverse_sweep_ds(ctypes.byref(d), 8, 8, 4, 2, 8, 8, 1, None, None, 0, None, 0, 8, 64,
                                   None) == _lib.DAMC_ERR_ARG
    hp = _lib.AdamCapturable()
    assert L.damc_adam_step_capturable(8, 0, None, None, None, None, 0, ctypes.byref(hp), None, 1, None, None,
                                       None) == _lib.DAMC_ERR_ARG  # no step pointer


def test_capturable_adam_constructs():
    from damc import _lib, optim

    p = torch.nn.Parameter(torch.zeros(4))
    for cls in (optim.Adam, optim.AdamW):
        o = cls([p], capturable=True)
        assert o.param_groups[0]["capturable"] is True
        assert sorted(o.defaults) == sorted(getattr(torch.optim, cls.__name__)([p], capturable=True).defaults)
        with pytest.raises(NotImplementedError):
            cls([p], capturable=True, amsgrad=True)
        with pytest.raises(NotImplementedError):
            cls([p], capturable=True, maximize=True)
        with pytest.raises(NotImplementedError):
            cls([p], capturable=True, differentiable=True)
        with pytest.raises(NotImplementedError):
            cls([p], lr=torch.tensor(1e-3))  # a tensor lr is read by the capturable kernel only
        assert isinstance(cls([p], lr=torch.tensor(1e-3), capturable=True).param_groups[0]["lr"], torch.Tensor)
    # still no fallback: CPU parameters are refused by the step, capturable or not
    p.grad = torch.ones(4)
    with pytest.raises(_lib.DamcError):
        optim.Adam([p], capturable=True).step()


def test_load_state_dict_keeps_the_capturable_flag_and_places_step():
    """A capturable torch state loads into the non-capturable damc optimiser (and the reverse): the flag stays the
    loading optimiser's own, and a non-capturable group's step is a CPU scalar.  (The device placement of a capturable
    group's step is a GPU test.)"""
    from damc import optim

    p = torch.nn.Parameter(torch.zeros(4))
    src = torch.optim.Adam([p], capturable=True)
    src.state[p] = dict(step=torch.tensor(3.0), exp_avg=torch.ones(4), exp_avg_sq=torch.ones(4))
    dst = optim.Adam([torch.nn.Parameter(torch.zeros(4))])
    dst.load_state_dict(src.state_dict())
    assert dst.param_groups[0]["capturable"] is False
    st = dst.state[dst.param_groups[0]["params"][0]]
    assert st["step"].device.type == "cpu" and float(st["step"]) == 3.0


def test_draws_and_seed_are_mutually_exclusive():
    from damc import _lib, amortizer, graphs, langevin, training
    from src import diffusion_net as dn

    with pytest.raises(_lib.DamcError):
        graphs.DrawState(1, "cpu")  # the state lives in device memory
    ds = graphs.DrawState.__new__(graphs.DrawState)  # no device here: the check comes before anything touches it
    z = torch.zeros(4, 128)
    for call in (
            lambda: langevin.posterior_langevin(z, z, None, None, 1, 0.1, 0.1, True, seed=1, draws=ds),
            lambda: langevin.prior_langevin(z, None, 1, 0.1, True, seed=1, draws=ds),
            lambda: langevin.z_update(z, z, 0.1, True, seed=1, draws=ds),
            lambda: langevin.philox_normal(1, 4, 128, seed=1, device="cpu", draws=ds),
            lambda: langevin.philox_uniform(1, 4, seed=1, device="cpu", draws=ds),
            lambda: training.q_noise_glue_seeded(None, z, seed=1, draws=ds),
            lambda: amortizer.reverse_sweep(None, z, z, seed=1, draws=ds),
            lambda: amortizer.q_forward(None, x=z, seed=1, draws=ds),
            lambda: dn._QBase.calculate_loss(None, z=z, seed=1, draws=ds),
    ):
        with pytest.raises(_lib.DamcError, match="mutually exclusive"):
            call()
    with pytest.raises(_lib.DamcError, match="DrawState"):
        langevin.philox_normal(1, 4, 128, device="cpu", draws=object())
    # out of scope: the guided sweep has no drawn form
    with pytest.raises(_lib.DamcError, match="guided"):
        amortizer.guided_sweep(None, z, z, z, 1.0, draws=ds)
    with pytest.raises(_lib.DamcError, match="guided"):
        amortizer.q_forward(None, x=z, cond_w=1.0, draws=ds)
