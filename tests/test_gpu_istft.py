"""The inverse short-time Fourier transform on the device (torchfx_amd/csrc/istft.hip) against tests/istft_reference.py: the
float64 irfft of the given bins, overlap-added in float64, under the derived per-sample bound (float64 results: twice the bound,
both sides carrying it, and a long-double inverse DFT under the bound itself at 256), and against the CPU float32 torch.istft on
the same bins (largest error at most 4x its).  The inputs are the device stft of Gaussian rows times a uniform(0.5, 1.5) mask:
arbitrary spectra, not consistent STFTs.  Shapes come from the plan -- the tile and the G frames of a batch -- never from a
workload; at most 4 rows.  A sample's bits depend on the frames that cover it alone, and a non-finite bin reaches exactly the
samples its frame covers.

Hann at hop = n_fft has no inverse (w[0] = 0 stands alone under the envelope and torch raises), so that hop runs with the
rectangular window; so does everything with center=False."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import istft_reference as R
from tests.gpu_common import DEV, TOL_CONV_F32, ext

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096]
CDT = {"f32": torch.complex64, "f64": torch.complex128}
RDT = {"f32": torch.float32, "f64": torch.float64}


def S():
    import torchfx_amd.spectral as S_
    return S_


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


def hann(n, dt):
    return torch.hann_window(n, dtype=torch.float64).to(RDT[dt]).to(DEV)


def relayout(X):
    """``X`` in the layout stft returns: the transpose of a contiguous [..., frames, bins] buffer."""
    return X.transpose(-1, -2).contiguous().transpose(-1, -2)


@functools.lru_cache(maxsize=None)
def spectrum(n, hop, frames, rows, dt, seed=0):
    """The device stft (Hann) of ``rows`` Gaussian rows times a uniform(0.5, 1.5) mask, cut to ``frames`` frames: [rows, bins, frames]."""
    g = np.random.default_rng(1000 * seed + n + hop)
    T = max((frames - 1) * hop, n)
    x = torch.from_numpy(g.standard_normal((rows, T)).astype(np.float32 if dt == "f32" else np.float64)).to(DEV)
    X = S().stft(x, n, hop, window=hann(n, dt))
    assert X.shape[-1] >= frames and X.dtype == CDT[dt]
    mask = torch.from_numpy(g.uniform(0.5, 1.5, tuple(X.shape))).to(RDT[dt]).to(DEV)
    return relayout((X * mask)[..., :frames])


def plan(n, hop, frames, dt, wl=None, center=True, rows=1, length=None):
    return ext().istft_plan_info(n, hop, wl or n, frames, rows, RDT[dt], center, length)


def check(X, n, hop, dt, window=None, wl=None, center=True, length=None, normalized=False, what="", cpu_ratio=True):
    """istft(X) within the bound of the reference; float32 also against the CPU float32 torch.istft on the same bins."""
    got = S().istft(X, n, hop, wl, window, center, normalized, None, length)
    Xc = X.cpu()
    wc = None if window is None else window.cpu()
    pad = n // 2 if center else 0
    y, b = R.reference(Xc.numpy(), n, hop, pad, None if wc is None else wc.numpy(), wl, length, normalized)
    assert got.dtype == RDT[dt] and got.device.type == "cuda" and got.is_contiguous()
    g = got.cpu().numpy().reshape(y.shape)
    _, err = R.within(g, y, b, what, factor=1.0 if dt == "f32" else 2.0)
    if dt == "f32" and cpu_ratio:
        cpu = torch.istft(Xc.reshape((-1,) + tuple(Xc.shape[-2:])), n, hop, wl, wc, center, normalized, None, length).numpy()
        cpu_err = float(np.abs(cpu - y).max())
        print(f"{what}: largest error {err:.3e}, CPU float32 torch.istft {cpu_err:.3e}, ratio {err / cpu_err:.2f}")
        assert err <= 4 * cpu_err
    return got


def three_tiles(n, hop, dt, wl=None):
    """The frame count that puts three tiles on a (centred) row, the last holding at most one hop."""
    tile = plan(n, hop, 8, dt, wl)["tile"]
    frames = 2 * tile // hop + 2
    p = plan(n, hop, frames, dt, wl)
    assert p["route"] == "lds" and 2 * tile < p["length"] <= 2 * tile + hop and p["workgroups"] == 3
    return frames


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_hop_within_the_bound(n, dt):
    for hop in [n // 4, n // 2, 100] + ([1] if n == 256 else []):
        frames = three_tiles(n, hop, dt)
        check(spectrum(n, hop, frames, 3, dt), n, hop, dt, hann(n, dt), what=f"{dt} {n}/{hop} hann, {frames} frames")
    frames = three_tiles(n, n, dt)
    check(spectrum(n, n, frames, 3, dt), n, n, dt, None, what=f"{dt} {n}/{n} rectangular, {frames} frames")
    wl = 3 * n // 4                                  # a rectangular window shorter than n_fft, its copies side by side
    frames = three_tiles(n, wl, dt, wl)
    check(spectrum(n, wl, frames, 3, dt), n, wl, dt, None, wl, what=f"{dt} {n}/{wl} rectangular of {wl}, {frames} frames")
    check(spectrum(n, n // 4, 9, 2, dt), n, n // 4, dt, hann(n, dt), normalized=True, what=f"{dt} {n} normalized")


def test_float64_at_256_against_the_long_double_inverse_dft():
    n, hop = 256, 64
    X = spectrum(n, hop, three_tiles(n, hop, "f64"), 2, "f64")
    w = hann(n, "f64")
    got = S().istft(X, n, hop, window=w).cpu().numpy()
    Xn = X.cpu().numpy()
    y, b = R.reference(Xn, n, hop, n // 2, w.cpu().numpy(), frames_exact=R.exact_frames_longdouble(Xn, n))
    R.within(got, y, b, "f64 256/64 against the long-double inverse DFT")


@pytest.mark.parametrize("dt,n", [("f32", 256), ("f32", 1024), ("f64", 512)])
def test_frame_counts_around_the_batch_and_the_tile(dt, n):
    hop = n // 4
    p = plan(n, hop, 8, dt)
    G, tile = p["frames_per_batch"], p["tile"]
    assert tile % hop == 0
    counts = {G - 1, G, G + 1, 2 * G + 1}
    centred = counts | {tile // hop + 1 + d for d in (-1, 0, 1)}                        # T = (F - 1) hop = tile - hop, tile, tile + hop
    apart = counts | {(tile - n) // hop + 1 + d for d in (-1, 0, 1)} | {1}              # T = (F - 1) hop + n
    for frames in sorted(f for f in centred if f >= 2):
        assert (frames - 1) * hop in (tile - hop, tile, tile + hop) or frames in counts
        check(spectrum(n, hop, frames, 2, dt, 1), n, hop, dt, hann(n, dt), what=f"{dt} {n}: {frames} frames, centred")
    for frames in sorted(f for f in apart if f >= 1):
        got = check(spectrum(n, hop, frames, 2, dt, 1), n, hop, dt, None, center=False, what=f"{dt} {n}: {frames} frames, not centred")
        assert got.shape == (2, (frames - 1) * hop + n)


def test_length_shorter_is_the_prefix_and_longer_ends_in_zeros():
    n, hop = 512, 128
    frames = three_tiles(n, hop, "f32")
    X = spectrum(n, hop, frames, 2, "f32")
    w = hann(n, "f32")
    nat = S().istft(X, n, hop, window=w)
    tile = plan(n, hop, frames, "f32")["tile"]
    for length in (1, hop - 1, tile - 1, tile, tile + 1, nat.shape[-1] - 1):
        assert torch.equal(S().istft(X, n, hop, window=w, length=length), nat[:, :length])
    natr = S().istft(X, n, hop)                     # rectangular: Hann's envelope vanishes in the half frame past the natural end
    for extra in (1, n // 2, n // 2 + 1, 2 * tile + 3):
        got = check(X, n, hop, "f32", None, length=natr.shape[-1] + extra, what=f"length natural + {extra}")
        assert torch.equal(got[:, :natr.shape[-1]], natr)
        assert (got[:, natr.shape[-1] + n // 2:] == 0).all() and got.shape[-1] == natr.shape[-1] + extra


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_exact_results(dt):
    for n in (256, 2048):
        tile = plan(n, n, 8, dt)["tile"]
        frames = 2 * tile // n + 3
        Z = torch.zeros(2, n // 2 + 1, frames, dtype=CDT[dt], device=DEV)
        for hop in (n, n // 2):
            y = S().istft(relayout(Z), n, hop)
            assert y.shape[-1] == (frames - 1) * hop and (y == 0).all()
            assert (S().istft(relayout(Z), n, hop, window=hann(n, dt)) == 0).all() if hop < n else True
            D = Z.clone()
            D[:, 0, :] = n
            assert (S().istft(relayout(D), n, hop) == 1).all()                           # X[0] = n_fft alone: the constant 1
            assert (S().istft(relayout(D), n, hop, center=False) == 1).all()
        ones = torch.ones_like(Z)                                                        # X[k] = 1: a unit impulse at each frame's start
        check(relayout(ones), n, n // 2, dt, None, center=False, what=f"{dt} {n} impulses", cpu_ratio=False)
        y, _ = R.reference(ones.cpu().numpy(), n, n // 2, 0)                             # what the bound was taken against:
        exp = np.zeros_like(y)
        exp[:, :frames * (n // 2):n // 2] = 0.5                                          # two rectangular windows cover every sample ...
        exp[:, 0] = 1.0                                                                  # ... but those of the first half frame
        assert np.abs(y - exp).max() < 1e-12


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_bits_do_not_depend_on_the_cut(dt):
    n, hop = 1024, 256
    frames = three_tiles(n, hop, dt)
    X = spectrum(n, hop, frames, 4, dt, 2)
    w = hann(n, dt)
    y = S().istft(X, n, hop, window=w)
    for r in range(4):                                                                   # a row alone and in the batch
        assert torch.equal(S().istft(relayout(X[r]), n, hop, window=w), y[r])
        assert torch.equal(S().istft(relayout(X[r:r + 1]), n, hop, window=w)[0], y[r])
    assert torch.equal(S().istft(relayout(X.reshape(2, 2, n // 2 + 1, frames)), n, hop, window=w).reshape(y.shape), y)
    Xc = X.contiguous()                                                                  # [rows, bins, frames] contiguous: the copy path
    assert not Xc.transpose(-1, -2).is_contiguous() and torch.equal(S().istft(Xc, n, hop, window=w), y)
    assert torch.equal(S().istft(X[::2], n, hop, window=w), y[::2])                      # a strided batch
    tile = plan(n, hop, frames, dt)["tile"]
    for k in (1, 3, 7):                                                                  # k zero frames in front shift every later sample
        assert (k * hop) % tile != 0
        X2 = relayout(torch.cat([torch.zeros_like(X[..., :k]), X], dim=-1))
        y2 = S().istft(X2, n, hop, window=w)
        assert torch.equal(y2[:, n + k * hop:], y[:, n:])
    ext().clear_caches()                                                                 # the tables are rebuilt to the same bits
    assert torch.equal(S().istft(X, n, hop, window=w), y)


@pytest.mark.parametrize("dt,n,wl", [("f32", 256, 256), ("f32", 2048, 1500), ("f64", 1024, 1024)])
def test_a_non_finite_bin_reaches_exactly_the_samples_its_frame_covers(dt, n, wl):
    hop = n // 4 if wl == n else wl // 4
    frames = three_tiles(n, hop, dt, wl)
    X = spectrum(n, hop, frames, 3, dt, 3)
    w = hann(wl, dt)                                                                     # zeros at its ends, and zero padding when wl < n
    clean = S().istft(X, n, hop, wl, w)
    T, pad, M = clean.shape[-1], n // 2, n // 2
    for f in (1, frames // 2, frames - 1):
        lo, hi = max(0, f * hop - pad), min(T, f * hop + n - pad)
        for (k, part), bad in zip(((M // 3, "imag"), (0, "real"), (M, "real")), (float("nan"), float("inf"), float("-inf"))):
            Xb = X.clone()
            getattr(Xb, part)[1, k, f] = bad
            got = S().istft(Xb, n, hop, wl, w)
            assert not torch.isfinite(got[1, lo:hi]).any(), (f, k, bad)
            assert torch.equal(got[1, :lo], clean[1, :lo]) and torch.equal(got[1, hi:], clean[1, hi:])
            assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    Xb = X.clone()                                                                       # the imaginary parts of bins 0 and M are not read
    Xb.imag[:, 0, :] = float("nan")
    Xb.imag[:, M, :] = float("nan")
    assert torch.equal(S().istft(Xb, n, hop, wl, w), clean)


def test_a_vanishing_envelope_raises_and_the_op_only_sets_the_flag():
    n, hop = 512, 128
    X = spectrum(n, hop, three_tiles(n, hop, "f32"), 2, "f32")
    E = ext()
    for kw, pad in ((dict(window=torch.zeros(n, device=DEV)), n // 2), (dict(window=hann(n, "f32"), center=False), 0)):
        with pytest.raises(RuntimeError, match="window overlap add min"):
            S().istft(X, n, hop, **kw)
        y, flag = E.istft_forward(X, kw["window"], n, hop, pad)
        assert flag.shape == (1,) and flag.dtype == torch.int32 and int(flag.item()) == 1
    y, flag = E.istft_forward(X, hann(n, "f32"), n, hop, n // 2)
    assert int(flag.item()) == 0 and torch.equal(y, S().istft(X, n, hop, window=hann(n, "f32")))
    with pytest.raises(RuntimeError, match="not on the LDS route"):
        E.istft_forward(torch.zeros(2, 201, 9, dtype=torch.complex64, device=DEV), None, 400, 100, 200)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_round_trip(dt):
    for n in (256, 4096):
        for hop in (n // 4, n // 2):
            frames = three_tiles(n, hop, dt)
            g = np.random.default_rng(n + hop)
            x = torch.from_numpy(g.standard_normal((2, (frames - 1) * hop)).astype(np.float32 if dt == "f32" else np.float64))
            w = hann(n, dt)
            xd = x.to(DEV)
            back = S().istft(S().stft(xd, n, hop, window=w), n, hop, window=w)
            cpu = torch.istft(torch.stft(x, n, hop, window=w.cpu(), return_complex=True), n, hop, window=w.cpu())
            err, cpu_err = float((back.cpu() - x).abs().max()), float((cpu - x).abs().max())
            print(f"{dt} {n}/{hop}: round trip error {err:.3e}, through CPU torch {cpu_err:.3e}")
            assert back.shape == x.shape and err <= 4 * cpu_err


def test_off_the_route_is_torch_istft_on_the_device():
    g = np.random.default_rng(9)
    for n, kw in ((400, dict()), (256, dict(onesided=False))):
        x = torch.from_numpy(g.standard_normal((2, 4000)).astype(np.float32))
        w = torch.hann_window(n)
        X = torch.stft(x, n, window=w, return_complex=True, onesided=kw.get("onesided", True))
        exp = torch.istft(X, n, window=w, **kw).numpy()
        got = S().istft(X.to(DEV), n, window=w.to(DEV), **kw)
        assert got.device.type == "cuda" and got.dtype == torch.float32
        scale = max(1.0, float(np.abs(exp).max()))
        err = float(np.abs(got.cpu().numpy() - exp).max())
        print(f"n_fft {n} {kw}: fallback differs from the CPU torch.istft by {err:.3e} (allowed {TOL_CONV_F32 * scale:.3e})")
        assert err <= TOL_CONV_F32 * scale
    from torchfx_amd import Wave
    X = spectrum(512, 128, 40, 2, "f32")
    wave = Wave.from_stft(X, 48000, 512, 128, window=hann(512, "f32"))
    assert wave.ys.device.type == "cuda" and torch.equal(wave.ys, S().istft(X, 512, 128, window=hann(512, "f32")))
