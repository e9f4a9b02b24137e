"""The phase vocoder on the device (torchfx_amd/csrc/phasevocoder.hip) against tests/phasevocoder_reference.py: the long-double
definition under the derived per-value bound, bit equality across forced segment counts, rows and batches, the reach of a
non-finite bin, the zero frames past the end and the two round trips.  Shapes come from the plan; at most 4 rows."""
import math

import numpy as np
import pytest
import torch

from tests import phasevocoder_reference as R
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

RATES = [0.5, 0.8, 1.0, 1.25, 2.0, 2.0 ** (-3 / 12)]
CDT = {"f32": torch.complex64, "f64": torch.complex128}
RDT = {"f32": torch.float32, "f64": torch.float64}


def fx():
    import torchfx_amd
    return torchfx_amd


def spectrum(n, frames, rows, dt):
    """The device stft (Hann, hop n / 4) of ``rows`` Gaussian rows times a uniform(0.5, 1.5) mask: [rows, n / 2 + 1, frames], in
    the layout stft returns."""
    g = np.random.default_rng(n + frames)
    x = torch.from_numpy(g.standard_normal((rows, max((frames - 1) * (n // 4), n))).astype(np.float32 if dt == "f32" else np.float64)).to(DEV)
    X = fx().stft(x, n, window=torch.hann_window(n, dtype=torch.float64).to(RDT[dt]).to(DEV))
    mask = torch.from_numpy(g.uniform(0.5, 1.5, tuple(X.shape))).to(RDT[dt]).to(DEV)
    return (X * mask)[..., :frames].transpose(-1, -2).contiguous().transpose(-1, -2)


def plan(F, bins, rate, dt, segments=0, rows=2):
    return ext().phase_vocoder_plan_info(F, bins, rate, rows, RDT[dt], segments)


# Frame counts whose output, cut into 7 segments by force, ends just above a segment boundary (the last segment holds one
# frame; two at rate 0.5, whose counts are even), one frame below one, and on one: F -> Fo 25, 27, 28 (32, 34, 42 at 0.5).
EDGE_FRAMES = {0.5: (16, 17, 21), 0.8: (20, 21, 22), 1.0: (25, 27, 28), 1.25: (31, 33, 34), 2.0: (49, 53, 55), RATES[5]: (21, 22, 23)}


@pytest.mark.parametrize("n", [256, 4096])                              # 129 and 2049 bins: both end in a partial tile
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_result_meets_the_derived_bound_at_every_segment_edge(dt, rate, n):
    for F, last in zip(EDGE_FRAMES[rate], ("above", "below", "on")):
        X = spectrum(n, F, 2, dt)
        p = plan(F, n // 2 + 1, rate, dt, 7)
        in_last = p["out_frames"] - 6 * p["seg_frames"]
        assert p["segments"] == 7 and in_last == {"above": 2 if rate == 0.5 else 1, "below": p["seg_frames"] - 1, "on": p["seg_frames"]}[last]
        got = ext().phase_vocoder_forward(X, rate, 7)
        assert got.dtype == CDT[dt] and got.shape == (2, n // 2 + 1, p["out_frames"]) and got.transpose(-1, -2).is_contiguous()
        assert p["launches"] == 2 and p["scratch_bytes"] == 2 * 7 * (n // 2 + 1) * 12 and p["bin_tile"] == 64
        Xh = X.cpu().numpy()
        R.within(got.cpu().numpy(), R.reference(Xh, rate), f"{dt} rate {rate:.4f} bins {n // 2 + 1} frames {F}")
        assert torch.equal(fx().phase_vocoder(X, rate), got)            # the plan's own choice: the same bits
        if rate == 1.0:
            polar = torch.polar(X.cpu().to(torch.complex128).abs(), X.cpu().to(torch.complex128).angle()).numpy()
            assert p["out_frames"] == F
            R.within(got.cpu().numpy(), (polar.real.astype(R.LD), polar.imag.astype(R.LD), np.abs(Xh).astype(R.LD)), "rate 1 against polar")


@pytest.mark.parametrize("rate", [0.8, 1.25])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_forced_cuts_rows_and_batches_give_the_same_bits(dt, rate):
    F, n = {0.8: 149, 1.25: 151}[rate], 256                             # 187 and 121 output frames: no cut below divides them
    X = spectrum(n, F, 4, dt)
    one = ext().phase_vocoder_forward(X, rate, 1)
    assert plan(F, n // 2 + 1, rate, dt, 1, rows=4)["launches"] == 1
    for s in (2, 3, 7):
        p = plan(F, n // 2 + 1, rate, dt, s, rows=4)
        assert p["segments"] == s and p["launches"] == 2 and p["out_frames"] % p["seg_frames"] != 0      # unequal segments
        assert torch.equal(ext().phase_vocoder_forward(X, rate, s), one), s
    assert torch.equal(ext().phase_vocoder_forward(X[2], rate, 3), one[2])                      # a row alone: [bins, F]
    assert torch.equal(ext().phase_vocoder_forward(X.reshape(2, 2, n // 2 + 1, F), rate, 2).reshape(one.shape), one)
    assert torch.equal(ext().phase_vocoder_forward(X.contiguous(), rate, 0), one)               # another layout: one copy


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_non_finite_bin_poisons_its_track_from_the_frame_that_reads_it_across_the_cuts(dt, value):
    F, n, rate, row, k = 150, 256, 0.8, 1, 70
    p = plan(F, n // 2 + 1, rate, dt, 3)
    i, _ = R.positions(F, rate, np.float32)
    j = int(i[p["seg_frames"]])                                         # the frame the second segment's first output stands on
    first = int(np.argmax(i + 1 >= j))
    assert first < p["seg_frames"] and p["segments"] == 3               # read on both sides of the first cut, one more cut after it
    X = spectrum(n, F, 2, dt).clone()
    clean = ext().phase_vocoder_forward(X, rate, 3)
    X[row, k, j] = complex(value, 1.0)
    for s in (3, 1):
        got = ext().phase_vocoder_forward(X, rate, s)
        assert torch.equal(got[row, k, :first], clean[row, k, :first])
        assert bool(torch.isnan(torch.view_as_real(got[row, k, first:])).all())
        got[row, k] = clean[row, k]
        assert torch.equal(got, clean)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_zero_frames_past_the_end(dt):
    # t rate < F for every t < Fo, so i <= F - 1: frame F is read, frame F + 1 (torchaudio pads two) by no output of any rate
    X = spectrum(256, 5, 2, dt)
    got = fx().phase_vocoder(X, 0.5)                                    # the last two outputs stand between frame 4 and the zero frame 5
    assert got.shape[-1] == 10
    R.within(got.cpu().numpy(), R.reference(X.cpu().numpy(), 0.5), f"padding {dt}")
    assert torch.allclose(got[..., 9].abs(), 0.5 * X[..., 4].abs(), rtol=1e-5)                  # half way to the zero frame


def test_round_trips_on_the_device():
    fs, T = 48000, 16384
    x = torch.sin(2 * math.pi * 440 * torch.arange(T, dtype=torch.float64) / fs).to(torch.float32).reshape(1, T).to(DEV)
    w = fx().Wave(x, fs, device=DEV)
    for rate in (0.8, 1.25):
        y = w | fx().TimeStretch(rate)
        assert y.ys.shape == (1, round(T / rate)) and y.fs == fs and y.ys.is_cuda
    shifted = w | fx().PitchShift(12)
    line, = shifted.explain()
    assert all(s in line for s in ("stft_kernel", "phase_vocoder_kernel", "istft_kernel", "resample", "no layout copy")), line
    y = shifted.ys
    assert y.shape == x.shape and y.dtype == x.dtype and y.is_cuda
    peak = int(np.abs(np.fft.rfft(y[0].cpu().numpy().astype(np.float64))).argmax())
    assert abs(peak * fs / T - 880.0) <= fs / T
