"""The short-time Fourier transform's reference and error bound (tests/test_stft_host.py, tests/test_gpu_stft.py).

A frame's windowed samples are ``s = fl(w x)``: one rounded product per sample, in the signal's dtype.  The reference is the
float64 ``numpy.fft.rfft`` of those same rounded samples (for float64 signals also a long-double direct DFT at small sizes), and
the bound on a frame's spectrum is

    || Xhat - X ||_2  <=  8 u (log2 n_fft + 2) sqrt(n_fft) || s ||_2,      u = 2^-24 (float32) or 2^-53 (float64):

Higham's bound for a radix-2 FFT with correctly rounded twiddles (Accuracy and Stability of Numerical Algorithms, theorem
24.2: a relative l2 error of log2(n) eta, eta a small multiple of u -- 8 u here), two more such terms for the window product
and the real-input post-twiddle, and ``|| X ||_2 <= sqrt(n_fft) || s ||_2`` over the one-sided bins.  Every bin is held to the
same right-hand side."""
import math

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def n_frames(T, n_fft, hop, pad):
    return 1 + (T + 2 * pad - n_fft) // hop


def full_window(window, win_length, n_fft, dtype):
    """``window`` (None: ones) of ``win_length`` values centred in ``n_fft`` zeros, in ``dtype`` -- torch.stft's padding."""
    w = np.ones(win_length, dtype) if window is None else np.asarray(window, dtype)
    assert w.shape == (win_length,)
    left = (n_fft - win_length) // 2
    full = np.zeros(n_fft, dtype)
    full[left:left + win_length] = w
    return full


def frames(x, n_fft, hop, pad, pad_mode="reflect"):
    """``x [rows, T]`` -> ``[rows, frames, n_fft]``: the samples of every frame of the padded rows, untouched."""
    x = np.atleast_2d(x)
    xp = np.pad(x, ((0, 0), (pad, pad)), mode=pad_mode) if pad else x
    nf = n_frames(x.shape[-1], n_fft, hop, pad)
    idx = hop * np.arange(nf)[:, None] + np.arange(n_fft)[None, :]
    return xp[:, idx]


def windowed(x, n_fft, hop, pad, pad_mode="reflect", window=None, win_length=None):
    """``s = fl(w x) [rows, frames, n_fft]`` in ``x``'s dtype."""
    w = full_window(window, n_fft if win_length is None else win_length, n_fft, x.dtype)
    with np.errstate(invalid="ignore"):
        s = frames(x, n_fft, hop, pad, pad_mode) * w
    assert s.dtype == x.dtype
    return s


def exact(s):
    """float64 rfft of the rounded samples: ``[rows, frames, n_fft / 2 + 1]``."""
    return np.fft.rfft(s.astype(np.float64), axis=-1)


def exact_longdouble(s):
    """Direct DFT of the rounded samples in long double (small n_fft only): ``[rows, frames, n_fft / 2 + 1]`` complex long double."""
    n = s.shape[-1]
    k = np.arange(n // 2 + 1, dtype=np.longdouble)[:, None] * np.arange(n, dtype=np.longdouble)[None, :]
    ang = 8 * np.arctan(np.longdouble(1)) * (k % n) / n         # 2 pi in long double
    sl = s.astype(np.longdouble)
    return (sl @ np.cos(ang).T) - 1j * (sl @ np.sin(ang).T)


def bound(s):
    """The right-hand side per frame, ``[rows, frames]``."""
    n = s.shape[-1]
    return 8 * U[s.dtype] * (math.log2(n) + 2) * math.sqrt(n) * np.linalg.norm(s.astype(np.float64), axis=-1)


def frame_errors(got, X):
    """``got [rows, bins, frames]`` (torch.stft's layout) against ``X [rows, frames, bins]`` -> (l2 error per frame, largest bin
    error per frame), each ``[rows, frames]`` float64."""
    d = np.abs(np.swapaxes(np.asarray(got), -1, -2).astype(np.clongdouble) - X).astype(np.float64)
    return np.sqrt((d * d).sum(-1)), d.max(-1)


def within(got, s, what, factor=1.0, X=None):
    """Assert ``got`` within ``factor`` times the bound of ``X`` (default: :func:`exact` of ``s``), per frame in l2 and per bin;
    prints and returns the largest fraction of the (unscaled) bound reached."""
    X = exact(s) if X is None else X
    got = np.asarray(got)
    if got.ndim == 2:
        got = got[None]
    assert got.shape == (X.shape[0], X.shape[2], X.shape[1]), f"{what}: shape {got.shape} against frames {X.shape}"
    l2, worst = frame_errors(got, X)
    b = bound(s)
    assert np.isfinite(l2).all(), f"{what}: non-finite result"
    tiny = np.finfo(np.float64).tiny
    frac_l2, frac_bin = float((l2 / np.maximum(b, tiny)).max()), float((worst / np.maximum(b, tiny)).max())
    print(f"{what}: l2 error {frac_l2:.3e} of the bound, largest bin {frac_bin:.3e}")
    assert (l2 <= factor * b).all(), f"{what}: frame l2 error reaches {frac_l2:.3e} of the bound"
    assert (worst <= factor * b).all(), f"{what}: a bin's error reaches {frac_bin:.3e} of the bound"
    return frac_l2
