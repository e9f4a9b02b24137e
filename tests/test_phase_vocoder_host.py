"""The phase vocoder without a device: the long-double definition against torchaudio's formula, the NumPy host path against the
definition under the derived bound, the argument errors, the stream processors' refusals and the +12 semitone round trip."""
import math

import numpy as np
import pytest
import torch

from tests import phasevocoder_reference as R

RATES = [0.5, 0.8, 1.0, 1.25, 2.0, 2.0 ** (-3 / 12)]


def spectrum(bins, F, dtype=np.complex128, seed=0):
    g = np.random.default_rng(seed)
    return (g.standard_normal((2, bins, F)) + 1j * g.standard_normal((2, bins, F))).astype(dtype)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("advance", ["default", "other"])
def test_the_definition_is_torchaudios_formula_and_phase_advance_drops_out(rate, advance):
    bins, F, hop = 9, 32, 4
    X = spectrum(bins, F)
    pa = np.linspace(0, math.pi * hop, bins)[:, None] if advance == "default" else np.random.default_rng(1).uniform(-7, 7, (bins, 1))
    want = R.torchaudio_formula(X, rate, pa)
    re, im, mag = R.reference(X, rate)
    assert want.shape == mag.shape
    err = max(np.abs(want.real - re).max(), np.abs(want.imag - im).max())
    assert err <= 1e-9 * float(mag.max()), err


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("rate", RATES)
def test_host_path_meets_the_bound(dtype, rate):
    import torchfx_amd as fx
    X = spectrum(17, 40, dtype, seed=2)
    got = fx.phase_vocoder(torch.from_numpy(X), rate, torch.zeros(17, 1))
    assert got.dtype == torch.from_numpy(X).dtype and got.shape[-1] == R.frames_out(40, rate)
    R.within(got.numpy(), R.reference(X, rate), f"host {np.dtype(dtype).name} rate {rate}")
    one = fx.phase_vocoder(torch.from_numpy(X[0, 3]).reshape(1, -1), rate)          # a track's bits are its own
    assert torch.equal(one[0], got[0, 3])


def test_bad_arguments_raise_value_errors_that_name_them():
    import torchfx_amd as fx
    X = torch.zeros(5, 8, dtype=torch.complex64)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match="rate"):
            fx.phase_vocoder(X, bad)
    for bad in (X.real, X[0]):
        with pytest.raises(ValueError, match="X must be"):
            fx.phase_vocoder(bad, 1.0)
    for pa in (torch.zeros(5), torch.zeros(4, 1), torch.zeros(5, 1, dtype=torch.complex64), [0.0] * 5):
        with pytest.raises(ValueError, match="phase_advance"):
            fx.phase_vocoder(X, 1.0, pa)
    with pytest.raises(ValueError, match="rate"):
        fx.TimeStretch(0.0)
    with pytest.raises(ValueError, match="n_steps"):
        fx.PitchShift(float("nan"))
    with pytest.raises(ValueError, match="bins_per_octave"):
        fx.pitch_shift(torch.zeros(4096), 1, bins_per_octave=0)
    with pytest.raises(ValueError, match="x must be"):
        fx.time_stretch(torch.zeros(4096, dtype=torch.int32), 1.25)
    with pytest.raises(ValueError, match="window must be"):
        fx.time_stretch(torch.zeros(4096), 1.25, window=torch.hann_window(1024))
    with pytest.raises(ValueError, match="longer than n_fft / 2"):
        fx.time_stretch(torch.zeros(1024), 1.25)
    assert fx.phase_vocoder(torch.zeros(5, 0, dtype=torch.complex64), 1.25).shape == (5, 0)


@pytest.mark.parametrize("cls,arg", [("TimeStretch", 0.8), ("PitchShift", 3)])
def test_stream_processors_refuse_the_round_trip_effects(cls, arg):
    import torchfx_amd as fx
    from torchfx_amd import realtime as RT
    effect = getattr(fx, cls)(arg)
    with pytest.raises(TypeError, match=f"^{cls} cannot run in StreamProcessor: the phase vocoder is a transform of the whole signal"):
        RT.StreamProcessor([fx.Gain(0.5), effect], chunk_size=256, device="cpu")
    backend = type("B", (), {"sample_rate": 48000, "channels": 2})()
    with pytest.raises(TypeError, match=f"^{cls} cannot run in RealtimeProcessor"):
        RT.RealtimeProcessor([effect], backend, RT.StreamConfig(), device="cpu")


def test_wave_round_trips_on_the_host_keep_the_rate_and_set_the_length():
    import torchfx_amd as fx
    fs, T = 48000, 16384
    x = torch.sin(2 * math.pi * 440 * torch.arange(T, dtype=torch.float64) / fs).to(torch.float32).reshape(1, T)
    w = fx.Wave(x, fs)
    for rate in (0.8, 1.25):
        y = w.time_stretch(rate, n_fft=1024)
        assert y.fs == fs and y.ys.shape == (1, round(T / rate))
    # the reference chain alone: 440 Hz a whole octave up lies at 880 Hz, within one bin of the result's spectrum
    y = (w | fx.PitchShift(12)).ys
    assert y.shape == x.shape and y.dtype == x.dtype
    peak = int(np.abs(np.fft.rfft(y[0].numpy().astype(np.float64))).argmax())
    assert abs(peak * fs / T - 880.0) <= fs / T
