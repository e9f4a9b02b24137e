"""True peak on the device (tfx_true_peak_forward, csrc/resample.hip): bit equality with the composition
resample_poly(x, L, 1).abs().amax(-1) at the kernel's own seams, parity with SciPy, where the peak sits, inter-sample peaks,
row independence, non-finite samples; and loudness_range / LoudnessNormalize(max_true_peak=...) / Wave.true_peak on device
tensors against their CPU paths."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import truepeak_signals as S
from tests.gpu_common import DEV, TOL_CONV_F32, TOL_CONV_F64, dev, ext

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
FACTORS = [2, 4, 8]
FS = {2: 96000, 4: 48000, 8: 48000}             # a rate at which the factor is allowed (4 and 2 are the defaults there)


def fx():
    import torchfx_amd
    return torchfx_amd


def plan(up, dtype=torch.float32, T=1000):
    """(Lp, tile_in) of the default interpolator for `up`."""
    info = ext().true_peak_plan_info(1, T, up, 20 * up + 1, dtype)
    return info["Lp"], info["tile_in"]


def lengths(up, dtype):
    Lp, tile = plan(up, dtype)
    return [1, 7, Lp - 1, Lp, tile - 1, tile, tile + 1, 2 * tile + 3]


@functools.lru_cache(maxsize=None)
def uniform(dtype, T, lead):
    """uniform(-1, 1) host data [*lead, T]; shared between the tests, never modified."""
    g = torch.Generator().manual_seed(1000 * len(lead) + T)
    return ((torch.rand(*lead, T, generator=g, dtype=torch.float64) * 2 - 1).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("up", FACTORS)
def test_bit_equal_to_the_composition(dtype, up):
    L = fx()
    for T in lengths(up, dtype):
        for lead in ((), (3,), (2, 2)):
            x = uniform(dtype, T, lead).to(DEV)
            got = L.true_peak_linear(x, FS[up], oversample=up)
            ref = L.resample_poly(x, up, 1).abs().amax(-1)
            assert got.shape == ref.shape and got.dtype == dtype and got.device == x.device
            assert torch.equal(got, ref), (T, lead, (got - ref).abs().max().item())
            assert torch.equal(L.true_peak(x, FS[up], oversample=up), 20.0 * torch.log10(got.to(torch.float64)))
    empty = torch.zeros(3, 0, dtype=dtype, device=DEV)
    assert torch.equal(L.true_peak_linear(empty, FS[up], oversample=up), torch.zeros(3, dtype=dtype, device=DEV))
    assert bool(torch.isneginf(L.true_peak(empty, FS[up], oversample=up)).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("up", FACTORS)
def test_parity_with_scipy(dtype, up):
    from scipy.signal import resample_poly
    L = fx()
    tol = TOL_CONV_F32 if dtype == torch.float32 else TOL_CONV_F64
    for T in lengths(up, dtype):
        for lead in ((), (3,), (2, 2)):
            x = uniform(dtype, T, lead)
            ref = np.abs(resample_poly(x.numpy(), up, 1, axis=-1)).max(-1)
            assert ref.dtype == x.numpy().dtype
            got = L.true_peak_linear(x.to(DEV), FS[up], oversample=up).cpu().numpy()
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
            assert err <= tol * max(1.0, float(np.abs(ref).max())), (T, lead, err)


def test_sample_peak_and_the_callers_taps_on_the_device():
    L = fx()
    from torchfx_amd.resample import design_taps
    x = uniform(torch.float32, 4097, (3,)).to(DEV)
    assert torch.equal(L.true_peak_linear(x, 192000), x.abs().amax(-1))
    assert torch.equal(L.true_peak_linear(x, 48000, oversample=1), x.abs().amax(-1))
    assert torch.equal(L.true_peak(x, 48000, taps=design_taps(4, 1)), L.true_peak(x, 48000))
    assert torch.equal(L.true_peak_linear(x, 48000, taps=[1.0, 1.0, 1.0, 1.0]), x.abs().amax(-1))
    # the longest filter the kernel takes (64 taps per phase, 65 with SciPy's leading zero) against the composition
    h = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, 256).astype(np.float32))
    ref = ext().resample_forward(x, 4, 1, h).abs().amax(-1)
    assert torch.equal(ext().true_peak(x, h, 4), ref)
    x64 = uniform(torch.float64, 4097, (3,)).to(DEV)
    ref = ext().resample_forward(x64, 4, 1, h.double()).abs().amax(-1)
    assert torch.equal(ext().true_peak(x64, h.double(), 4), ref)
    with pytest.raises(RuntimeError, match="64 \\* up"):
        ext().true_peak(x, torch.zeros(257), 4)
    with pytest.raises(RuntimeError, match="dtype"):
        ext().true_peak(x, torch.zeros(81, dtype=torch.float64), 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_where_the_peak_sits(dtype):
    L = fx()
    from torchfx_amd.resample import design_taps
    _, tile = plan(4, dtype)
    T = 2 * tile + 3
    centre = design_taps(4, 1, dtype=dtype)[40]
    assert abs(float(centre) - 1.000637) <= 1e-6
    places = [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, T - 1]
    x = torch.zeros(2 * len(places), T, dtype=dtype)
    for k, p in enumerate(places):
        x[2 * k, p], x[2 * k + 1, p] = 1.0, -1.0
    got = L.true_peak_linear(x.to(DEV), 48000).cpu()
    assert torch.equal(got, centre.expand(2 * len(places))), got.tolist()
    two = torch.zeros(T, dtype=dtype)
    two[tile // 2], two[tile + tile // 2] = 0.5, -0.75
    assert torch.equal(L.true_peak_linear(two.to(DEV), 48000).cpu(), centre * 0.75)
    two[tile // 2], two[tile + tile // 2] = -0.75, 0.5
    assert torch.equal(L.true_peak_linear(two.to(DEV), 48000).cpu(), centre * 0.75)


def test_inter_sample_peak_of_the_tech3341_tone():
    L = fx()
    for fs in (48000, 44100, 96000):
        for div, phase in S.TONES:
            err = float(L.true_peak(dev(S.tone(div, phase)), fs)) - 20.0 * math.log10(0.5)
            assert -S.TP_TOL_BELOW <= err <= S.TP_TOL_ABOVE, (fs, div, phase, err)
    x = dev(S.tone(4, 45.0))
    assert float(L.true_peak(x, 48000)) - float(L.true_peak(x, 48000, oversample=1)) > 2.9


def test_rows_are_independent_and_calls_repeat():
    L = fx()
    _, tile = plan(4)
    x = uniform(torch.float32, 2 * tile + 3, (5,)).to(DEV)
    batch = L.true_peak_linear(x, 48000)
    assert torch.equal(batch, torch.stack([L.true_peak_linear(x[r], 48000) for r in range(5)]))
    assert torch.equal(batch, L.true_peak_linear(x, 48000))
    wide = uniform(torch.float32, 2 * tile + 3, (2, 2)).to(DEV)
    view = wide[:, :, 5:tile + 100]
    assert not view.is_contiguous()
    assert torch.equal(L.true_peak_linear(view, 48000), L.true_peak_linear(view.contiguous(), 48000))
    assert torch.equal(L.true_peak_linear(wide.transpose(0, 1), 48000), L.true_peak_linear(wide, 48000).transpose(0, 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_samples_stay_in_their_row(dtype):
    L = fx()
    _, tile = plan(4, dtype)
    x = uniform(dtype, 2 * tile + 3, (3,)).clone()
    clean = L.true_peak_linear(x.to(DEV), 48000)
    x[1, tile + 5] = math.nan
    got = L.true_peak_linear(x.to(DEV), 48000)
    assert bool(torch.isnan(got[1])) and torch.equal(got[[0, 2]], clean[[0, 2]])
    assert bool(torch.isnan(L.true_peak(x.to(DEV), 48000)[1]))
    x[1, tile + 5] = math.inf
    got = L.true_peak_linear(x.to(DEV), 48000)
    assert not bool(torch.isfinite(got[1])) and torch.equal(got[[0, 2]], clean[[0, 2]])
    x[1, tile + 5] = 0.0
    x[1, 0], x[2, -1] = math.nan, -math.inf                             # the first and the last sample of a row
    got = L.true_peak_linear(x.to(DEV), 48000)
    assert bool(torch.isnan(got[1])) and not bool(torch.isfinite(got[2])) and torch.equal(got[0], clean[0])


def test_loudness_range_on_the_device():
    L = fx()
    fs = 8000
    unit = float(L.integrated_loudness(torch.from_numpy(S.stereo_sine(fs, S.LRA_TONE[fs], 5)), fs))
    for dtype in (np.float32, np.float64):
        x = torch.from_numpy(S.lra_signal((-20.0, -30.0), 20, fs, unit).astype(dtype))
        cpu, got = L.loudness_range(x, fs), L.loudness_range(x.to(DEV), fs)
        assert got.device.type == "cuda" and got.dtype == torch.float64 and got.shape == ()
        assert abs(float(got) - float(cpu)) <= 1e-9 and abs(float(got) - 10.0) <= S.LRA_TOL
    xb = torch.stack([x, 0.5 * x.flip(-1)]).to(DEV)
    gb = L.loudness_range(xb, fs)
    assert gb.shape == (2,) and torch.equal(gb[0], L.loudness_range(xb[0], fs)) and torch.equal(gb[1], L.loudness_range(xb[1], fs))
    assert float(L.loudness_range(torch.zeros(2, 4 * fs, device=DEV), fs)) == 0.0
    assert float(L.loudness_range(x[:, :2 * fs].to(DEV), fs)) == 0.0
    assert abs(L.Wave(x, fs, device=DEV).loudness_range() - float(cpu)) <= 1e-9


def test_loudness_normalize_ceiling_on_the_device():
    """The applied gain equals the CPU path's to 1e-9 dB on a float64 signal (there the two true-peak readings agree to
    rounding in float64); a float32 signal's device reading differs from SciPy's by float32 summation order, TOL_CONV_F32 of
    the peak = 9e-5 dB, and the result still sits within 1e-3 dB of the ceiling."""
    L = fx()
    fs = 48000
    ln = L.LoudnessNormalize(-14, max_true_peak=-1.0, fs=fs)
    x64 = torch.from_numpy(S.accent_tone(dtype=np.float64))
    cpu, got = ln(x64), ln(x64.to(DEV))
    assert got.device.type == "cuda" and got.dtype == torch.float64
    k = int(cpu.abs().argmax())
    assert abs(20.0 * math.log10(abs(float(got[k])) / abs(float(cpu[k])))) <= 1e-9
    assert float((got.cpu() - cpu).abs().max()) <= 1e-9 * math.log(10.0) / 20.0 * float(cpu.abs().max())
    x32 = torch.from_numpy(S.accent_tone()).to(DEV)
    y = ln(x32)
    assert y.dtype == torch.float32 and abs(float(L.true_peak(y, fs).amax()) - (-1.0)) <= 1e-3
    assert float(L.true_peak(L.LoudnessNormalize(-14, fs=fs)(x32), fs).amax()) > 0.0
    quiet = dev(S.tone(4, 45.0, 0.05, 96000))
    assert torch.equal(ln(quiet), L.LoudnessNormalize(-14, fs=fs)(quiet))
    route = ln.route(x32)
    assert "sos_block_energy_kernel" in route and "true_peak_kernel" in route
    st = torch.stack([x32, 0.5 * x32])
    assert L.Wave(st, fs, device=DEV).true_peak() == float(L.true_peak(st, fs).amax())
    out = L.Wave(st, fs, device=DEV) | ln
    assert abs(out.true_peak() - (-1.0)) <= 1e-3
