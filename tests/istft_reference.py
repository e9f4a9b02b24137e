"""The inverse short-time Fourier transform's reference and error bound (tests/test_istft_host.py, tests/test_gpu_istft.py).

The reference takes the *given* bins: frame ``f`` is the float64 ``numpy.fft.irfft`` of ``X[..., :, f]`` (which does not read the
imaginary parts of bins 0 and n_fft / 2; for float64 results at small sizes also a long-double direct inverse DFT), the
overlap-add of ``w s_f`` and of ``w w`` runs in float64, and ``y = num / env``.

The bound carries the project's frame bound (tests/stft_reference.py: Higham, Accuracy and Stability of Numerical Algorithms,
theorem 24.2, ``8 u (log2 n + 2)`` relative in l2) through the sum.  A computed frame differs from the exact one by at most
``8 u (log2 n + 2) ||s_f||_2`` in every sample; the product with the window, the ``c(t) - 1`` additions of ``c(t)`` terms, the
same for the envelope and the division add ``(c(t) + 3) u`` relative to the sum of the magnitudes:

    | yhat[t] - y[t] |  <=  ( sum_f |w_f| 8 u (log2 n + 2) ||s_f||_2  +  (c(t) + 3) u sum_f |w_f s_f| ) / env[t],

the sums over the ``c(t)`` frames that cover ``t``, ``w_f = w[t - f hop]``, ``s_f`` the exact frame, ``u`` 2^-24 or 2^-53."""
import math

import numpy as np

from tests.stft_reference import U, full_window


def natural_length(frames, n_fft, hop, pad):
    return (frames - 1) * hop + n_fft - 2 * pad


def exact_frames(X, n_fft, normalized=False):
    """``X [rows, bins, frames]`` -> the exact frames ``[rows, frames, n_fft]`` in float64 (torch's scaling)."""
    s = np.fft.irfft(np.swapaxes(np.asarray(X), -1, -2).astype(np.complex128), n_fft, axis=-1)
    return s * math.sqrt(n_fft) if normalized else s


def exact_frames_longdouble(X, n_fft):
    """Direct inverse DFT of the one-sided bins in long double (small n_fft only): ``[rows, frames, n_fft]``."""
    Xl = np.swapaxes(np.asarray(X), -1, -2)
    re, im = Xl.real.astype(np.longdouble), Xl.imag.astype(np.longdouble)
    M = n_fft // 2
    k = np.arange(M + 1, dtype=np.longdouble)[:, None] * np.arange(n_fft, dtype=np.longdouble)[None, :]
    ang = 8 * np.arctan(np.longdouble(1)) * (k % n_fft) / n_fft
    wgt = np.full(M + 1, 2, np.longdouble)
    wgt[0] = wgt[M] = 1
    c, s = np.cos(ang) * wgt[:, None], np.sin(ang) * wgt[:, None]
    s[0] = s[M] = 0                                     # the imaginary parts of bins 0 and M are not read
    return (re @ c - im @ s) / n_fft


def overlap_add(s, w, hop):
    """``s [rows, frames, n_fft]``, ``w [n_fft]`` -> (num, env, bound numerators A, B, cover count) over the padded time axis
    ``[(frames - 1) hop + n_fft]``: ``A = sum |w| ||s_f||_2``, ``B = sum |w s_f|``."""
    rows, frames, n = s.shape
    L = (frames - 1) * hop + n
    num, A, B = np.zeros((rows, L), s.dtype), np.zeros((rows, L), np.float64), np.zeros((rows, L), np.float64)
    env, cnt = np.zeros(L, s.dtype), np.zeros(L, np.int64)
    w = w.astype(s.dtype)
    norm = np.linalg.norm(s.astype(np.float64), axis=-1)
    for f in range(frames):
        sl = slice(f * hop, f * hop + n)
        num[:, sl] += w * s[:, f]
        env[sl] += w * w
        A[:, sl] += np.abs(w.astype(np.float64))[None, :] * norm[:, f, None]
        B[:, sl] += np.abs((w * s[:, f]).astype(np.float64))
        cnt[sl] += 1
    return num, env, A, B, cnt


def reference(X, n_fft, hop, pad, window=None, win_length=None, length=None, normalized=False, frames_exact=None):
    """``X [rows, bins, frames]`` -> (y ``[rows, T]`` float64 (or long double with ``frames_exact``), the bound per sample
    ``[rows, T]`` for results of ``X``'s precision).  Positions past the last frame are 0 with bound 0."""
    X = np.asarray(X)
    if X.ndim == 2:
        X = X[None]
    real = np.float32 if X.dtype == np.complex64 else np.float64
    u = U[np.dtype(real)]
    w = full_window(window, n_fft if win_length is None else win_length, n_fft, np.float64)
    s = exact_frames(X, n_fft, normalized) if frames_exact is None else frames_exact
    num, env, A, B, cnt = overlap_add(s, w, hop)
    T = natural_length(X.shape[-1], n_fft, hop, pad) if length is None else length
    y, b = np.zeros((X.shape[0], T), num.dtype), np.zeros((X.shape[0], T), np.float64)
    m = min(T, num.shape[-1] - pad)
    e = env[pad:pad + m].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        y[:, :m] = num[:, pad:pad + m] / env[pad:pad + m]
        b[:, :m] = (8 * u * (math.log2(n_fft) + 2) * A[:, pad:pad + m] + (cnt[pad:pad + m] + 3) * u * B[:, pad:pad + m]) / e
    return y, b


def within(got, y, b, what, factor=1.0):
    """Assert ``|got - y| <= factor * b`` per sample; prints and returns (largest fraction of the unscaled bound, largest error)."""
    got = np.asarray(got)
    if got.ndim == 1:
        got = got[None]
    assert got.shape == y.shape, f"{what}: shape {got.shape} against {y.shape}"
    assert np.isfinite(got).all(), f"{what}: non-finite result"
    d = np.abs(got.astype(np.longdouble) - y).astype(np.float64)
    tiny = np.finfo(np.float64).tiny
    frac = float((d / np.maximum(b, tiny))[b > 0].max()) if (b > 0).any() else 0.0
    print(f"{what}: error {frac:.3e} of the bound, largest {d.max():.3e}")
    assert (d <= factor * b).all(), f"{what}: a sample's error reaches {frac:.3e} of the bound"
    return frac, float(d.max())
