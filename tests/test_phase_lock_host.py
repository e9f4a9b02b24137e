"""Identity phase locking on the host path (NumPy) against tests/phaselock_reference.py, and the argument errors."""
import numpy as np
import pytest
import torch

import torchfx_amd as fx
from tests import phaselock_reference as L


@pytest.mark.parametrize("rate", [0.5, 0.8, 1.0, 1.25, 2.5])
@pytest.mark.parametrize("bins,F", [(1, 2), (3, 9), (65, 9), (129, 1)])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_host_path_meets_the_bound(dt, bins, F, rate):
    X = L.ladder(2, bins, F, dt)
    ref = L.reference(X, rate)
    assert ref[3] >= 1e-3
    got = fx.phase_vocoder(torch.from_numpy(X), rate, phase_lock="identity")
    L.within(got.numpy(), ref, f"host {dt} bins {bins} F {F} rate {rate}")
    if rate == 1.0:
        assert torch.equal(got, fx.phase_vocoder(torch.from_numpy(X), rate))


def test_flat_spectrum_is_the_plain_vocoder_and_a_nan_poisons_the_row():
    coin = torch.rand((2, 17, 12), generator=torch.Generator().manual_seed(1)) < 0.5
    X = torch.where(coin, torch.tensor(3 + 4j), torch.tensor(-4 + 3j))  # every modulus exactly 5: no peak anywhere
    assert torch.equal(fx.phase_vocoder(X, 0.5, phase_lock="identity"), fx.phase_vocoder(X, 0.5))
    Y = torch.from_numpy(L.ladder(2, 17, 12, "f32"))
    clean = fx.phase_vocoder(Y, 1.25, phase_lock="identity")
    Y[1, 4, 5] = complex("nan")
    got = fx.phase_vocoder(Y, 1.25, phase_lock="identity")
    first = 4                                                           # t = 4 stands on p = 5.0: the first to read frame 5
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1, :, :first], clean[1, :, :first])
    assert bool(torch.isnan(torch.view_as_real(got[1, :, first:])).all())


def test_argument_errors_name_phase_lock():
    x = torch.zeros(1, 4096)
    for call in (lambda: fx.phase_vocoder(torch.zeros(3, 4, dtype=torch.complex64), 1.0, phase_lock="scaled"),
                 lambda: fx.time_stretch(x, 0.8, phase_lock="scaled"), lambda: fx.pitch_shift(x, 3, phase_lock=1),
                 lambda: fx.TimeStretch(0.8, phase_lock="scaled"), lambda: fx.PitchShift(3, phase_lock="scaled"),
                 lambda: fx.Wave(x, 48000).time_stretch(0.8, phase_lock="scaled"),
                 lambda: fx.Wave(x, 48000).pitch_shift(3, phase_lock="scaled")):
        with pytest.raises(ValueError, match="phase_lock"):
            call()
    assert "phase_lock='identity'" in repr(fx.PitchShift(3, phase_lock="identity"))
    from torchfx_amd import torchfx_ext as E
    p = E.phase_vocoder_plan_info(5625, 1025, 0.8, 64, torch.float32, 0, 1)
    assert p["threads"] * p["bins_per_thread"] >= 1025 and p["workgroups"] == 64 * p["segments"] and p["launches"] == 2
    with pytest.raises(RuntimeError, match="phase_lock"):
        E.phase_vocoder_plan_info(100, 4098, 0.8, 1, torch.float32, 0, 1)
