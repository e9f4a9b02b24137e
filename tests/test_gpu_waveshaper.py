"""The waveshaper on the device (csrc/waveshaper.hip): torch.equal to the device composition resample -> multiply -> clamp ->
resample for the hard clipper at every length class of the tiling, the per-sample bound of tests/waveshaper_reference.py for
tanh, cubic and three curves under a bias and a partial mix, planted impulses and NaNs at every tile seam, batch independence,
transparency at mix = 0, the effect in a Wave and tap-array windows.  The tile and the reach come from the plan query.

These tests run the default window (LP = 24) and three symmetric tap arrays (LP = 16 and 72) with stages of equal length.  Every
register bucket of waveshaper_kernel, stages of unequal length (a tile origin I0 != 0), asymmetric taps read back exactly, the
extremes of the non-finite reach and the transfer functions' edges are tests/test_gpu_waveshaper_edges.py, over the cases of
tests/waveshaper_cases.py (checked without a device by tests/test_waveshaper_cases_host.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import waveshaper_reference as R
from tests.gpu_common import DEV, ext
from torchfx_amd import Distortion, Wave, resample_poly, waveshape
from torchfx_amd.resample import design_taps

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
LS = [1, 2, 4, 8]
WINDOW = ("kaiser", 5.0)
CURVES = {
    "curve2": np.array([-1.0, 1.0]),
    "curve3": np.array([-0.5, 0.1, 0.8]),
    "curve4096": np.tanh(3.0 * np.linspace(-1.0, 1.0, 4096)),
}
KW = dict(drive_db=9.0, bias=0.15, mix=0.3, output_db=-6.0)
WORST = {}


def plan(T, L, dt, window=None):
    n = (20 * L + 1 if window is None else len(window)) if L > 1 else 0
    return ext().waveshaper_plan_info(T, L, n, n, 0, DT[dt][0])


def lengths(L, dt):
    q = plan(1, L, dt)
    N, rb, ra = q["tile"], q["reach_before"], q["reach_after"]
    return sorted({T for T in (1, 2, ra, rb + ra + 1, N - 1, N, N + 1, 2 * N + rb + 3) if T > 0}), N, rb, ra


def signal(shape, seed, dt):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(DT[dt][1])


def composition(x, L, drive_db, window=WINDOW):
    drive = 10.0 ** (drive_db / 20.0)
    return resample_poly(torch.clamp(resample_poly(x, L, 1, window=window) * drive, -1, 1), 1, L, window=window)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", LS)
def test_hard_has_the_bits_of_the_device_composition(L, dt):
    Ts, N, rb, ra = lengths(L, dt)
    for T in Ts:
        for shape in ((T,), (3, T), (2, 2, T)):
            x = torch.from_numpy(signal(shape, T + len(shape), dt)).to(DEV)
            for drive_db in (0.0, 14.0):
                y = waveshape(x, "hard", drive_db=drive_db, oversample=L)
                assert y.shape == x.shape and y.dtype == x.dtype and y.device == x.device
                assert torch.equal(y, composition(x, L, drive_db)), (T, shape, drive_db)


@functools.lru_cache(maxsize=None)
def taps(L, dt):
    if L == 1:
        return None, None
    return design_taps(L, 1, WINDOW, DT[dt][0]).numpy(), design_taps(1, L, WINDOW, DT[dt][0]).numpy()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("shape", ["tanh", "cubic", "curve2", "curve3", "curve4096"])
def test_other_shapes_stay_within_the_bound(shape, L, dt):
    Ts, N, rb, ra = lengths(L, dt)
    hu, hd = taps(L, dt)
    curve = CURVES.get(shape)
    for T in ((N + 1, 2 * N + rb + 3) if dt == "f32" else (N + 1,)):
        x = signal((3, T), 100 + T, dt)
        q = plan(T, L, dt)
        y = waveshape(torch.from_numpy(x).to(DEV), None if curve is not None else shape, oversample=L, curve=curve, **KW)
        frac = R.check(y.cpu().numpy(), x, L, hu, hd, q["taps_up"], q["taps_dn"], "curve" if curve is not None else shape,
                       what=f"gpu {shape} L={L} {dt} T={T}", curve=curve, **KW)
        WORST[(shape, dt)] = max(WORST.get((shape, dt), 0.0), frac)
    print("largest fraction of the bound so far:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", [2, 4, 8])
def test_impulses_on_both_sides_of_a_seam(L, dt):
    _, N, rb, ra = lengths(L, dt)
    x = torch.zeros(2 * N, dtype=DT[dt][0])
    x[N - 1], x[N] = 1.0, -0.75
    x = x.to(DEV)
    y = waveshape(x, "hard", drive_db=3.0, oversample=L)
    assert torch.equal(y, composition(x, L, 3.0))
    assert float(y[:N - 1 - rb].abs().sum()) == 0.0 and float(y[N + ra + 1:].abs().sum()) == 0.0      # nothing outside the reach
    assert float(y[N - 1]) != 0.0 and float(y[N]) != 0.0


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", LS)
def test_a_nan_poisons_exactly_its_window(L, dt):
    _, N, rb, ra = lengths(L, dt)
    T = 2 * N + rb + 3
    base = signal((T,), 9, dt)
    for i in (0, T - 1, N - 1, N):
        for bad in (np.nan, np.inf):
            x, x0 = base.copy(), base.copy()
            x[i], x0[i] = bad, 0.0
            y = waveshape(torch.from_numpy(x).to(DEV), "tanh", drive_db=6.0, bias=0.1, oversample=L, mix=0.7).cpu().numpy()
            y0 = waveshape(torch.from_numpy(x0).to(DEV), "tanh", drive_db=6.0, bias=0.1, oversample=L, mix=0.7).cpu().numpy()
            want = np.zeros(T, bool)
            want[max(0, i - rb):min(T, i + ra + 1)] = True
            assert np.array_equal(np.isnan(y), want), (i, bad, np.flatnonzero(np.isnan(y) != want)[:8])
            assert np.array_equal(y[~want], y0[~want]), (i, bad)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_rows_do_not_depend_on_the_batch(dt):
    for L in LS:
        _, N, rb, ra = lengths(L, dt)
        x = torch.from_numpy(signal((3, N + 5), 21, dt)).to(DEV)
        y = waveshape(x, "cubic", oversample=L, **KW)
        for k in range(3):
            assert torch.equal(y[k], waveshape(x[k].clone(), "cubic", oversample=L, **KW))
        b = waveshape(x.reshape(1, 3, -1).expand(2, 3, -1).contiguous(), "cubic", oversample=L, **KW)
        assert torch.equal(b[0], y) and torch.equal(b[1], y)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_mix_zero_returns_the_input(dt):
    for L in LS:
        _, N, rb, ra = lengths(L, dt)
        x = torch.from_numpy(signal((2, N + 7), 33, dt)).to(DEV)
        assert torch.equal(waveshape(x, "tanh", drive_db=24.0, bias=0.2, oversample=L, mix=0.0), x)


def test_distortion_in_a_wave_is_the_function():
    x = torch.from_numpy(signal((2, 5000), 41, "f32"))
    w = Wave(x, 48000, device=DEV)
    out = w | Distortion()
    line, = out.explain()                                            # before .ys runs the pipeline
    assert line.startswith("Distortion: native (waveshaper_kernel, L = 4, tanh, 21 taps per phase up and 85 taps down, ")
    assert torch.equal(out.ys, waveshape(w.ys, "tanh", drive_db=12.0, oversample=4))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_tap_array_windows(dt):
    for L, n in ((2, 128), (4, 37), (8, 512)):                       # at the cap, odd and short, at the cap
        h = np.hanning(n + 2)[1:-1] / (n / 2)
        q = plan(1, L, dt, window=h)
        x = torch.from_numpy(signal((2, q["tile"] + q["reach_before"] + 9), 51, dt)).to(DEV)
        assert torch.equal(waveshape(x, "hard", drive_db=10.0, oversample=L, window=h), composition(x, L, 10.0, window=h))
    with pytest.raises(ValueError, match="at most 64 \\* oversample = 256"):
        waveshape(torch.zeros(64, device=DEV), oversample=4, window=np.ones(257))
    with pytest.raises(RuntimeError, match="at most 64"):
        ext().waveshaper_forward(torch.zeros(64, device=DEV), 4, "hard", None, 1.0, 0.0, 0.0, 1.0, torch.ones(257), torch.ones(257))
