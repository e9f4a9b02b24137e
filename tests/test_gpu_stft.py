"""The short-time Fourier transform on the device (csrc/stft.hip through torchfx_amd.stft / spectrogram) against
tests/stft_reference.py: the float64 rfft of the same rounded windowed samples under the derived bound (float64 signals: twice
the bound, both sides carrying it, and a long-double DFT under the bound itself at 256), and against the CPU float32 torch.stft
on the same inputs (largest per-frame l2 error at most 4x its).  Shapes come from the plan -- G frames per workgroup -- never
from a workload; at most 4 rows.  Frames are independent to the bit and a non-finite sample reaches exactly the frames that hold
it: an Inf arrives as NaN or Inf (Inf - Inf and Inf * 0 inside the transform), so "non-finite" is what is asserted."""
import math

import numpy as np
import pytest
import torch

from tests import stft_reference as R
from tests.gpu_common import DEV, TOL_CONV_F32, dev, ext

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
DTYPES = {"f32": np.float32, "f64": np.float64}
TDT = {np.float32: torch.float32, np.float64: torch.float64}
_CACHE: dict = {}


def S():
    import torchfx_amd.spectral as sp
    return sp


def gauss(rows, T, seed, dtype):
    key = (rows, T, seed, np.dtype(dtype).name)
    if key not in _CACHE:
        _CACHE[key] = np.random.default_rng(seed).standard_normal((rows, T)).astype(dtype)
    return _CACHE[key]


def hann(n, dtype):
    return torch.hann_window(n, periodic=True, dtype=torch.float64).to(TDT[dtype]).numpy()


def run(x, n_fft, hop, window=None, win_length=None, center=True, pad_mode="reflect", normalized=False, power=None):
    """The public function on a device copy of ``x`` -> NumPy, after checking that the plan takes the kernel."""
    rows = int(np.prod(x.shape[:-1]))
    wl = n_fft if win_length is None else win_length
    info = ext().stft_plan_info(n_fft, hop, wl, x.shape[-1], rows, TDT[x.dtype.type], center, pad_mode)
    assert info["route"] == "lds", info
    w = None if window is None else dev(np.asarray(window, x.dtype))
    if power is None:
        y = S().stft(dev(x), n_fft, hop, win_length, w, center, pad_mode, normalized)
    else:
        y = S().spectrogram(dev(x), n_fft, hop, win_length, "rect" if w is None else w, power, center, pad_mode, normalized)
    torch.cuda.synchronize()
    assert y.shape[-2:] == (n_fft // 2 + 1, info["frames"]) and y.transpose(-1, -2).is_contiguous()
    return y.cpu().numpy()


def plan_g(n_fft, dtype):
    return ext().stft_plan_info(n_fft, n_fft // 4, n_fft, 10 * n_fft, 1, TDT[dtype])["frames_per_workgroup"]


def check(got, x, n_fft, hop, what, window=None, win_length=None, center=True, pad_mode="reflect"):
    """Within the bound of the float64 rfft (twice the bound for float64 signals); returns (s, the fraction reached)."""
    s = R.windowed(x, n_fft, hop, n_fft // 2 if center else 0, pad_mode, window, win_length)
    return s, R.within(got, s, what, 2.0 if x.dtype == np.float64 else 1.0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_every_size_and_hop_within_the_bound_and_4x_the_cpu_transform(n_fft, dt):
    """Three rows of odd length (rows start off a 16-byte boundary), 2 G + 1 frames or more (three workgroups or more share a
    row; exactly 2 G + 1, the last workgroup holding a single frame, wherever that row is long enough to reflect), Hann window,
    reflect padding; hop n/4 also with zero padding."""
    dtype = DTYPES[dt]
    G = plan_g(n_fft, dtype)
    w = hann(n_fft, dtype)
    hops = [n_fft // 4, n_fft // 2, n_fft, 2 * n_fft, 100] + ([1] if n_fft == 256 else [])
    for hop in hops:
        T = 301 if hop == 1 else max(2 * G * hop, n_fft // 2 + hop) + 1        # reflect needs more than n_fft / 2 samples
        x = gauss(3, T, n_fft + hop, dtype)
        got = run(x, n_fft, hop, w)
        assert got.shape[-1] == 1 + T // hop >= 2 * G + 1 and T % 2 == 1
        s, _ = check(got, x, n_fft, hop, f"n_fft {n_fft} hop {hop} {dt}", w)
        if dtype == np.float32:
            cpu = torch.stft(torch.from_numpy(x), n_fft, hop, window=torch.from_numpy(w), return_complex=True).numpy()
            X = R.exact(s)
            e_dev, e_cpu = R.frame_errors(got, X)[0].max(), R.frame_errors(cpu, X)[0].max()
            print(f"n_fft {n_fft} hop {hop}: largest frame l2 error, device / CPU torch.stft = {e_dev / e_cpu:.3f}")
            assert e_dev <= 4 * e_cpu
        elif n_fft == 256:
            R.within(got, s, f"n_fft 256 hop {hop} f64 against the long-double DFT", 1.0, R.exact_longdouble(s))
    x = gauss(3, 2 * G * (n_fft // 4) + 1, n_fft, dtype)
    check(run(x, n_fft, n_fft // 4, w, pad_mode="constant"), x, n_fft, n_fft // 4, f"n_fft {n_fft} zero padding {dt}", w, pad_mode="constant")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_frame_counts_around_the_workgroup(n_fft, dt):
    dtype = DTYPES[dt]
    G, hop = plan_g(n_fft, dtype), n_fft // 4
    for frames in sorted({max(1, G - 1), G, G + 1, 2 * G + 1}):
        for center in (True, False):
            T = (frames - 1) * hop + (1 if center else n_fft)
            if center and T <= n_fft // 2:
                continue                                   # reflect needs pad < T; the shortest legal row has its own test
            x = gauss(2, T, frames, dtype)
            got = run(x, n_fft, hop, center=center)
            assert got.shape[-1] == frames
            check(got, x, n_fft, hop, f"n_fft {n_fft} {frames} frames center={center} {dt}", center=center)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", [256, 4096])
def test_shortest_rows(n_fft, dt):
    dtype = DTYPES[dt]
    x = gauss(3, n_fft // 2 + 1, 5, dtype)                  # the shortest row reflect padding allows: every frame is mostly reflection
    for mode in ("reflect", "constant"):
        for hop in (n_fft // 4, 1 if n_fft == 256 else n_fft // 2):
            check(run(x, n_fft, hop, pad_mode=mode), x, n_fft, hop, f"T = n_fft / 2 + 1, {mode}, hop {hop}, {dt}", pad_mode=mode)
    with pytest.raises(RuntimeError, match="Padding size should be less than"):
        S().stft(dev(x[:, :-1]), n_fft)
    one = gauss(3, n_fft, 6, dtype)
    got = run(one, n_fft, n_fft // 4, center=False)
    assert got.shape == (3, n_fft // 2 + 1, 1)
    check(got, one, n_fft, n_fft // 4, f"one frame, {dt}", center=False)
    with pytest.raises(RuntimeError, match="expected 0 < n_fft"):
        S().stft(dev(one[:, :-1]), n_fft, center=False)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", [256, 1024])
def test_windows(n_fft, dt):
    dtype = DTYPES[dt]
    G, hop = plan_g(n_fft, dtype), n_fft // 4
    x = gauss(2, (G + 2) * hop + 1, 9, dtype)
    odd = n_fft - 55                                        # 201 in 256
    ramp = lambda n: (np.arange(n) + 1.0) / n               # asymmetric: reversed indexing would show
    for what, w, wl in (("rectangular", None, None), ("hann", hann(n_fft, dtype), None), ("ramp", ramp(n_fft), None),
                        ("short rectangular", None, odd), ("short ramp", ramp(odd), odd), ("one tap", np.array([1.5]), 1),
                        ("one tap of ones", None, 1)):
        got = run(x, n_fft, hop, w, wl)
        check(got, x, n_fft, hop, f"n_fft {n_fft} {what} {dt}", w, wl)
    # one tap: bin 0 of a frame is 1.5 times the sample under the tap, exactly
    centre = R.frames(x, n_fft, hop, n_fft // 2)[:, :, (n_fft - 1) // 2]         # where torch centres a window of one value
    assert np.array_equal(np.abs(run(x, n_fft, hop, np.array([1.5]), 1)[:, 0, :]), np.abs(dtype(1.5) * centre))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_exact_results(n_fft, dt):
    dtype = DTYPES[dt]
    G, hop = plan_g(n_fft, dtype), n_fft // 2
    frames = 2 * G + 4
    T = (frames - 1) * hop + n_fft
    # silence up to the start of frame G + 2, then ones: frames 0 .. G lie wholly in the silence and are exactly zero in every bin,
    # frames G + 2 .. lie wholly in the ones and have bin 0 == n_fft exactly; the second row is the first one reversed
    x = np.zeros((2, T), dtype)
    x[0, (G + 2) * hop:] = 1
    x[1] = x[0, ::-1]
    got = run(x, n_fft, hop, center=False)
    fr = R.frames(x, n_fft, hop, 0)
    zero, ones = (fr == 0).all(-1), (fr == 1).all(-1)
    assert (zero.sum(-1) >= G + 1).all() and (ones.sum(-1) >= G + 1).all()
    g = np.swapaxes(got, -1, -2)
    assert (g[zero] == 0).all() and (g[ones][:, 0] == n_fft).all()
    check(got, x, n_fft, hop, f"steps n_fft {n_fft} {dt}", center=False)
    # a unit impulse at offset m of a frame (frames side by side, hop = n_fft): |X_k| = 1 and the phase of exp(-2 pi i k m / n),
    # within the bound (||s|| = 1)
    u = R.U[np.dtype(dtype)]
    bound = 8 * u * (math.log2(n_fft) + 2) * math.sqrt(n_fft)
    k = np.arange(n_fft // 2 + 1)
    offsets = {0: 1, 1: n_fft // 2 + 3, G + 1: n_fft - 1, G + 2: 0, G + 3: n_fft // 2}
    x = np.zeros((1, (G + 4) * n_fft), dtype)
    for f, m in offsets.items():
        x[0, f * n_fft + m] = 1
    got = run(x, n_fft, n_fft, center=False)[0]
    assert got.shape[-1] == G + 4
    for f, m in offsets.items():
        exp = np.exp(-2j * np.pi * ((k * m) % n_fft) / n_fft)
        assert np.abs(got[:, f] - exp).max() <= bound and np.abs(np.abs(got[:, f]) - 1).max() <= bound, (f, m)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_a_frames_bits_depend_on_its_own_samples_alone(n_fft, dt):
    """The same n_fft samples at another frame index, in another row, under another hop, at another place in the workgroup,
    centred or not, alone or in a batch: the same bits."""
    dtype = DTYPES[dt]
    G = plan_g(n_fft, dtype)
    w = hann(n_fft, dtype)
    block = gauss(1, n_fft, 77, dtype)[0]
    seen = []
    for hop, f, row, center in ((n_fft // 4, 1, 0, False), (n_fft // 4, G + 1, 2, False), (n_fft // 2, 2 * G, 1, False), (100, 3, 2, False),
                                (2 * n_fft, G + 2 if G > 1 else 2, 0, False), (n_fft // 4, 2, 1, True), (n_fft, 1, 0, True)):
        pad = n_fft // 2 if center else 0
        T = (2 * G + 3) * hop + n_fft + 1
        x = gauss(3, T, hop + f, dtype).copy()
        at = f * hop - pad
        x[row, at:at + n_fft] = block
        got = run(x, n_fft, hop, w, center=center)
        seen.append(got[row, :, f].copy())
        alone = run(x[row:row + 1], n_fft, hop, w, center=center)
        assert np.array_equal(alone[0], got[row]), "a row alone and the same row in a batch"
    for other in seen[1:]:
        assert np.array_equal(seen[0].view(dtype), other.view(dtype))
    assert np.isfinite(seen[0]).all() and np.abs(seen[0]).max() > 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_a_non_finite_sample_reaches_exactly_the_frames_that_hold_it(n_fft, dt):
    dtype = DTYPES[dt]
    G, hop = plan_g(n_fft, dtype), n_fft // 4
    T = (2 * G + 2) * hop + 1
    x = gauss(3, T, 31, dtype)
    w = hann(n_fft, dtype)                                  # its first value is 0: the product is still formed, NaN * 0 = NaN
    clean = run(x, n_fft, hop, w)
    clean_p = run(x, n_fft, hop, w, power=2.0)
    where = R.frames(np.arange(T)[None, :], n_fft, hop, n_fft // 2)[0]           # the sample index behind every frame's every tap
    for bad in (np.nan, np.inf, -np.inf):
        for t in (3, T // 2 + 1, T - 2):                    # behind the reflected start, in the middle, behind the reflected end
            y = x.copy()
            y[1, t] = bad
            hit = (where == t).any(-1)
            assert 0 < hit.sum() < hit.size
            for power, ref in ((None, clean), (2.0, clean_p)):
                got = run(y, n_fft, hop, w, power=power)
                assert not np.isfinite(got[1][:, hit]).any(), f"{bad} at {t}: a bin of a frame that holds it is finite"
                assert np.array_equal(got[1][:, ~hit], ref[1][:, ~hit]) and np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    # through the reflected edge: sample 3 sits at padded positions pad - 3 and pad + 3, so frame 0 holds it twice
    assert (where[0] == 3).sum() == 2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", [512, 1024])
def test_power_magnitude_and_normalisation_are_formed_from_the_devices_own_spectrum(n_fft, dt):
    dtype = DTYPES[dt]
    u = R.U[np.dtype(dtype)]
    G, hop = plan_g(n_fft, dtype), n_fft // 4
    x = gauss(2, (G + 1) * hop + 1, 41, dtype)
    w = hann(n_fft, dtype)
    for normalized in (False, True):
        X = run(x, n_fft, hop, w, normalized=normalized)
        re, im = X.real.astype(np.float64), X.imag.astype(np.float64)
        p2, p1 = run(x, n_fft, hop, w, normalized=normalized, power=2.0), run(x, n_fft, hop, w, normalized=normalized, power=1.0)
        assert p2.dtype == p1.dtype == dtype
        assert (np.abs(p2 - (re * re + im * im)) <= 2 * u * (re * re + im * im)).all()
        assert (np.abs(p1 - np.hypot(re, im)) <= 2 * u * np.hypot(re, im)).all()
    # normalized: one more rounding per component of the plain result
    plain, norm = run(x, n_fft, hop, w), run(x, n_fft, hop, w, normalized=True)
    scale = float(dtype(1.0 / math.sqrt(n_fft)))
    for a, b in ((plain.real, norm.real), (plain.imag, norm.imag)):
        exp = a.astype(np.float64) * scale
        assert (np.abs(b - exp) <= u * np.abs(exp)).all()


def test_geometries_off_the_route_fall_back_to_torch_on_the_device():
    x = gauss(3, 4801, 51, np.float32)
    xd = dev(x)
    for kw in (dict(n_fft=400), dict(n_fft=256, onesided=False), dict(n_fft=256, pad_mode="replicate")):
        info = ext().stft_plan_info(kw["n_fft"], kw["n_fft"] // 4, kw["n_fft"], 4801, 3, torch.float32, True, kw.get("pad_mode", "reflect"),
                                    kw.get("onesided", True))
        assert info["route"] == "torch"
        got = S().stft(xd, **kw)
        exp = torch.stft(torch.from_numpy(x), return_complex=True, **kw)
        assert got.is_cuda and got.shape == exp.shape and got.stride() == exp.stride()
        g, e = torch.view_as_real(got.cpu()).numpy(), torch.view_as_real(exp).numpy()
        scale = max(1.0, float(np.abs(e).max()))
        err = float(np.abs(g - e).max())
        print(f"{kw}: fallback differs from the CPU torch.stft by {err:.3e} (allowed {TOL_CONV_F32 * scale:.3e})")
        assert err <= TOL_CONV_F32 * scale
    p = S().spectrogram(xd, 400)
    e = torch.stft(torch.from_numpy(x), 400, window=torch.hann_window(400), return_complex=True).abs().square().numpy()
    assert p.dtype == torch.float32 and np.abs(p.cpu().numpy() - e).max() <= TOL_CONV_F32 * max(1.0, float(e.max()))


def test_layout_batches_and_the_wave_methods():
    from torchfx_amd import Wave
    x = gauss(4, 6001, 61, np.float32)
    xd = dev(x)
    ref = torch.stft(xd, 1024, 256, window=torch.hann_window(1024, device=DEV), return_complex=True)
    got = S().stft(xd, 1024, 256, window=torch.hann_window(1024, device=DEV))
    assert got.shape == ref.shape and got.stride() == ref.stride() and got.dtype == ref.dtype
    b = S().stft(xd.reshape(2, 2, -1), 1024, 256, window=torch.hann_window(1024, device=DEV))
    assert b.shape == (2, 2, 513, got.shape[-1]) and torch.equal(b.reshape(got.shape), got)
    assert torch.equal(S().stft(xd[1], 1024, 256, window=torch.hann_window(1024, device=DEV)), got[1])
    assert torch.equal(S().stft(xd.t().contiguous().t(), 1024, 256, window=torch.hann_window(1024, device=DEV)), got)     # strided input
    wave = Wave(xd, 48000, device=DEV)
    assert torch.equal(wave.stft(1024, 256, window=torch.hann_window(1024, device=DEV)), got)
    sg = wave.spectrogram(1024, 256)
    assert sg.dtype == torch.float32 and sg.shape == got.shape
    assert torch.equal(sg, S().spectrogram(xd, 1024, 256))
    assert torch.equal(wave.spectrogram(1024, 256, power=None), S().stft(xd, 1024, 256, window=S().named_window("hann", 1024, device=DEV)))
    ext().clear_caches()                                    # the tables come back
    assert torch.equal(S().stft(xd, 1024, 256, window=torch.hann_window(1024, device=DEV)), got)
