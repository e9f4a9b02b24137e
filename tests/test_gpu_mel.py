"""Mel spectrogram on the device (torchfx_amd/csrc/mel.hip) against tests/mel_reference.py: exact selection of spectrogram's
bits, band seams around the plan's lanes_per_filter, mel banks end to end, frame independence, non-finite samples, the log forms
and the composition.  Shapes come from mel_plan_info; every case first asserts the route it means."""
import numpy as np
import pytest
import torch

from tests import mel_reference as R
from tests import stft_reference as SR
from tests.gpu_common import DEV, TOL_CONV_F32, dev, ext

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
DTYPES = {"f32": np.float32, "f64": np.float64}
TDT = {np.float32: torch.float32, np.float64: torch.float64}
BANKS = [dict(sample_rate=16000, n_mels=40), dict(sample_rate=48000, n_mels=80, norm="slaney", mel_scale="slaney")]


def S():
    import torchfx_amd.spectral as sp
    return sp


def gauss(rows, T, seed, dtype):
    return np.random.default_rng(seed).standard_normal((rows, T)).astype(dtype)


def design(n_fft, dtype, sample_rate, **kw):
    return S().mel_filterbank(n_fft // 2 + 1, sample_rate, dtype=TDT[dtype], **kw).numpy()


def plan(x, n_fft, hop, fb, pad_mode="reflect"):
    return ext().mel_plan_info(n_fft, hop, n_fft, x.shape[-1], int(np.prod(x.shape[:-1])), TDT[x.dtype.type], True, pad_mode, fb.shape[1],
                               int(R.band_lengths(fb).sum()))


def run(x, n_fft, hop, fb, pad_mode="reflect", **kw):
    """``fb`` as a caller's bank on a device copy of ``x`` -> NumPy ``[rows, filters, frames]``, once the plan takes the kernel."""
    info = plan(x, n_fft, hop, fb, pad_mode)
    assert info["route"] == "lds", info
    y = S().mel_spectrogram(dev(x), 1, n_fft, hop, pad_mode=pad_mode, filterbank=dev(fb), **kw)
    torch.cuda.synchronize()
    assert y.shape[-2:] == (fb.shape[1], info["frames"]) and y.transpose(-1, -2).is_contiguous()
    return y.cpu().numpy()


def spec(x, n_fft, hop, power=2.0, pad_mode="reflect"):                 # the device's own spectrogram, [rows, frames, bins]
    return np.swapaxes(S().spectrogram(dev(x), n_fft, hop, power=power, pad_mode=pad_mode).cpu().numpy(), -1, -2)


def plan_g(n_fft, dtype):
    return ext().stft_plan_info(n_fft, n_fft // 4, n_fft, 10 * n_fft, 1, TDT[dtype])["frames_per_workgroup"]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_single_ones_select_spectrograms_bits(n_fft, dt):
    dtype, M = DTYPES[dt], n_fft // 2
    bins = [0, 1, 7, M // 3, M - 1, M]
    fb = np.zeros((M + 1, len(bins) + 1), dtype)                         # the last column stays zero
    fb[bins, np.arange(len(bins))] = 1
    x = gauss(2, 5 * n_fft + 3, n_fft, dtype)
    for power in (1.0, 2.0):
        got, P = run(x, n_fft, n_fft // 4, fb, power=power), spec(x, n_fft, n_fft // 4, power)
        assert np.array_equal(got[:, :-1, :], np.swapaxes(P[:, :, bins], -1, -2)) and (got[:, -1, :] == 0).all() and P.max() > 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", [256, 1024])
def test_band_lengths_around_the_lanes_of_a_filter(n_fft, dt):
    """Bands of 1, S - 1, S, S + 1, 2 S + 1, M + 1 weights (S: lanes_per_filter), ramps -1 ... 1; then two filters, a larger S."""
    dtype, M = DTYPES[dt], n_fft // 2
    x = gauss(3, 9 * n_fft // 2 + 1, 5, dtype)
    P = spec(x, n_fft, n_fft // 4)
    lanes = []
    for pick in (slice(None), slice(4, 6)):
        n = len(range(6)[pick])
        S_ = ext().mel_plan_info(n_fft, n_fft // 4, n_fft, x.shape[-1], 3, TDT[dtype], True, "reflect", n, M + 1)["lanes_per_filter"]
        lengths = [1, S_ - 1, S_, S_ + 1, 2 * S_ + 1, M + 1][pick]
        fb = np.zeros((M + 1, n), dtype)
        for m, L in enumerate(lengths):
            lo = (37 * (m + 1)) % (M + 2 - L)
            fb[lo:lo + L, m] = 1 if L == 1 else np.linspace(-1, 1, L)
        assert plan(x, n_fft, n_fft // 4, fb)["lanes_per_filter"] == S_ and (R.band_lengths(fb) == lengths).all()
        lanes.append(S_)
        R.within(run(x, n_fft, n_fft // 4, fb), R.project(fb, P), R.projection_bound(fb, P), f"n_fft {n_fft} {dt} S {S_} bands {lengths}")
    assert lanes[1] > max(1, lanes[0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_mel_banks_end_to_end(n_fft, dt):
    """3 rows of 2 G + 1 frames: the float64 sum over the device's spectrogram, then the float64 result from the samples."""
    dtype, hop = DTYPES[dt], n_fft // 4
    x = gauss(3, 2 * plan_g(n_fft, dtype) * hop + 1, n_fft + 1, dtype)
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64).to(TDT[dtype]).numpy()
    for pad_mode in ("reflect", "constant") if n_fft == 512 else ("reflect",):
        s = SR.windowed(x, n_fft, hop, n_fft // 2, pad_mode, w)
        for kw in BANKS:
            fb = design(n_fft, dtype, **kw)
            assert plan(x, n_fft, hop, fb, pad_mode)["route"] == "lds"
            for power in (1.0, 2.0):
                got = S().mel_spectrogram(dev(x), n_fft=n_fft, hop_length=hop, power=power, pad_mode=pad_mode, **kw).cpu().numpy()
                P = spec(x, n_fft, hop, power, pad_mode)
                what = f"n_fft {n_fft} {dt} {pad_mode} {kw['n_mels']} mels power {power}"
                R.within(got, R.project(fb, P), R.projection_bound(fb, P), what + " over the device's spectrogram")
                R.within(got, *R.from_samples(fb, s, SR.bound(s), power, dtype), what + " from the samples")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", [256, 1024])
def test_a_frames_mel_bits_depend_on_its_own_samples_alone(n_fft, dt):
    dtype = DTYPES[dt]
    G, fb, block, seen = plan_g(n_fft, dtype), design(n_fft, dtype, **BANKS[0]), gauss(1, n_fft, 77, dtype)[0], []
    for hop, f, row in ((n_fft // 4, 2, 0), (n_fft // 4, G + 3, 2), (n_fft // 2, 2 * G, 1), (100, 6, 2), (2 * n_fft, G + 2, 0)):
        x = gauss(3, (2 * G + 3) * hop + n_fft + 1, hop + f, dtype)
        x[row, f * hop - n_fft // 2:f * hop + n_fft // 2] = block
        got = run(x, n_fft, hop, fb, log="db" if hop == 100 else None)
        alone = run(x[row:row + 1], n_fft, hop, fb, log="db" if hop == 100 else None)
        assert np.array_equal(alone[0], got[row]), "a row alone and the same row in a batch"
        seen.append(got[row, :, f] if hop != 100 else run(x, n_fft, hop, fb)[row, :, f])
    assert all(np.array_equal(seen[0], other) for other in seen[1:]) and np.isfinite(seen[0]).all() and seen[0].max() > 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", [256, 1024])
def test_a_non_finite_sample_reaches_exactly_the_frames_that_hold_it(n_fft, dt):
    dtype, hop = DTYPES[dt], n_fft // 4
    T = (2 * plan_g(n_fft, dtype) + 2) * hop + 1
    x, fb = gauss(3, T, 31, dtype), design(n_fft, dtype, sample_rate=16000, n_mels=64)       # at 129 bins one filter is empty
    full = R.band_lengths(fb) > 0
    assert (n_fft != 256) or (0 < full.sum() < full.size)
    where = SR.frames(np.arange(T)[None, :], n_fft, hop, n_fft // 2)[0]
    for log in (None, "db"):
        clean = run(x, n_fft, hop, fb, log=log)
        for bad, t in ((np.nan, 3), (np.inf, T // 2 + 1), (-np.inf, T - 2), (np.nan, T - 2), (np.inf, 3)):
            y = x.copy()
            y[1, t] = bad
            hit = (where == t).any(-1)
            got = run(y, n_fft, hop, fb, log=log)
            assert 0 < hit.sum() < hit.size and not np.isfinite(got[1][np.ix_(full, hit)]).any(), f"{bad} at {t}"
            got[1][np.ix_(full, hit)] = clean[1][np.ix_(full, hit)]
            assert np.array_equal(got, clean), f"{bad} at {t}: a value outside the frames that hold it changed"


@pytest.mark.parametrize("dt", DTYPES)
def test_log_forms(dt):
    dtype, n_fft, hop = DTYPES[dt], 512, 128
    x, fb = gauss(3, 40 * hop + 1, 9, dtype), design(512, dtype, sample_rate=16000, n_mels=64)
    x[1] = 0                                                             # a silent row: the floor in every frame
    x[2] *= 1e-4
    amin = float(dtype(1e-10))
    for power in (1.0, 2.0):
        v = run(x, n_fft, hop, fb, power=power).astype(np.float64)
        for log, c in (("db", 10.0 if power == 2.0 else 20.0), ("log10", 1.0), ("ln", np.log(10.0))):
            got = run(x, n_fft, hop, fb, power=power, log=log)
            exact = c * np.log10(np.maximum(v, amin))
            frac = float((np.abs(got - exact) / (R.LOG_ULPS * R.U[np.dtype(dtype)] * np.abs(exact))).max())
            print(f"{dt} power {power} {log}: {frac:.3e} of the bound")
            assert frac <= 1.0 and (got[1] == got[1].flat[0]).all() and (v[1] == 0).all()
    raw = S().mel_spectrogram(dev(x), 1, n_fft, hop, filterbank=dev(fb), log="db")
    assert torch.equal(S().mel_spectrogram(dev(x), 1, n_fft, hop, filterbank=dev(fb), log="db", top_db=80.0), torch.maximum(raw, raw.amax() - 80.0))
    assert float(raw.amax() - raw.amin()) > 80.0


def test_fallbacks_layouts_and_the_prepared_form():
    sp, E = S(), ext()
    x = gauss(6, 9000, 2, np.float32)
    cases = [dict(n_fft=400, n_mels=40), dict(n_fft=512, filterbank=np.abs(gauss(257, 32, 4, np.float32))),
             dict(n_fft=512, filterbank=design(512, np.float64, sample_rate=16000, n_mels=40))]
    for kw in cases:
        fb = kw.pop("filterbank", None)
        if fb is None:
            assert E.mel_plan_info(400, 100, 400, 9000, 6, n_filters=40, total_band=400)["route"] == "composition"
        elif fb.dtype == np.float32:
            assert plan(x, 512, 128, fb)["route"] == "composition"
        want = sp.mel_spectrogram(torch.from_numpy(x), 16000, log="db", filterbank=None if fb is None else torch.from_numpy(fb), **kw).numpy()
        got = sp.mel_spectrogram(dev(x), 16000, log="db", filterbank=None if fb is None else dev(fb), **kw)
        assert got.dtype == torch.float32 and got.is_cuda and np.abs(got.cpu().numpy() - want).max() <= TOL_CONV_F32 * max(1.0, np.abs(want).max())
    mel = sp.MelSpectrogram(16000, 512, n_mels=40, log="db", top_db=60.0)
    flat = sp.mel_spectrogram(dev(x), 16000, 512, n_mels=40, log="db")
    assert flat.shape == (6, 40, 71) and flat.stride() == (40 * 71, 1, 40)
    batch = sp.mel_spectrogram(dev(x).view(2, 3, -1), 16000, 512, n_mels=40, log="db")
    assert torch.equal(batch, flat.view(2, 3, 40, 71)) and torch.equal(sp.mel_spectrogram(dev(x)[4], 16000, 512, n_mels=40, log="db"), flat[4])
    wide = dev(np.repeat(x, 2, axis=1))[:, ::2]                          # a strided input
    assert not wide.is_contiguous() and torch.equal(sp.mel_spectrogram(wide, 16000, 512, n_mels=40, log="db"), flat)
    clamped = torch.maximum(batch, batch.amax(dim=(1, 2, 3), keepdim=True) - 60.0)
    assert torch.equal(mel(dev(x).view(2, 3, -1)), clamped) and torch.equal(mel(dev(x)[:3]), clamped[0])
    from torchfx_amd import Wave
    assert torch.equal(Wave(dev(x)[:2], 16000, device=DEV).mel_spectrogram(512, n_mels=40, log="db"), flat[:2])
    E.clear_caches()
    assert torch.equal(sp.mel_spectrogram(dev(x), 16000, 512, n_mels=40, log="db"), flat) and torch.equal(mel(dev(x)[:3]), clamped[0])
