"""The mel spectrogram's reference and error bounds (tests/test_mel_host.py, tests/test_gpu_mel.py): plain float64 NumPy.

Filterbank: ``torchaudio.functional.melscale_fbanks``' formulas, written out below.

Projection.  ``v_m = sum_k w_k P_k`` over a band of L weights, evaluated in the signal's dtype as a sum of L fused
multiply-adds (the lane tree of the kernel adds S partial sums pairwise: never more roundings on a term's path than the
sequential sum has).  Higham (Accuracy and Stability of Numerical Algorithms, section 3.1): ``|vhat - v| <= gamma_L sum |w_k|
|P_k|`` with ``gamma_L = L u / (1 - L u) <= (L + 1) u`` for the band lengths here -- :func:`projection_bound`.

From the samples.  With ``Xhat = X + e`` the device's spectrum, ``||e||_2 <= B`` per frame (tests/stft_reference.py) and X the
exact transform of the rounded windowed samples:
  power 2:  ``| |Xhat_k|^2 - |X_k|^2 | <= 2 |X_k| |e_k| + |e_k|^2``, so the weighted sum moves by at most ``max|w| (2 ||X||_2 B +
            B^2)`` (Cauchy-Schwarz over the bins); forming ``re^2 + im^2`` costs two more roundings and the projection L + 1:
            ``(L + 3) u sum |w_k| |X_k|^2`` to first order.
  power 1:  ``| |Xhat_k| - |X_k| | <= |e_k|``, so ``||w||_2 B``, and the square root is one more rounding: ``(L + 3) u sum |w_k|
            |X_k|`` covers it.
Logarithm: the device library states 2 ulp for the float32 logarithms and 1 ulp for float64; one more rounding for the factor c
and one for slack: ``4 u |exact|`` -- :data:`LOG_ULPS`."""
import math

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
LOG_ULPS = 4.0


def hz_to_mel(f, mel_scale="htk"):
    f = np.asarray(f, np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1.0) / 1000.0) / math.log(6.4))


def mel_to_hz(m, mel_scale="htk"):
    m = np.asarray(m, np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp(math.log(6.4) * (m - 15.0) / 27.0))


def fbanks(n_freqs, sample_rate, n_mels, f_min=0.0, f_max=None, norm=None, mel_scale="htk"):
    f_max = sample_rate / 2 if f_max is None else f_max
    freqs = np.linspace(0.0, sample_rate / 2, n_freqs)
    pts = mel_to_hz(np.linspace(hz_to_mel(f_min, mel_scale), hz_to_mel(f_max, mel_scale), n_mels + 2), mel_scale)
    fb = np.zeros((n_freqs, n_mels))
    for m in range(n_mels):
        down = (freqs - pts[m]) / (pts[m + 1] - pts[m])
        up = (pts[m + 2] - freqs) / (pts[m + 2] - pts[m + 1])
        fb[:, m] = np.maximum(0.0, np.minimum(down, up)) * (2.0 / (pts[m + 2] - pts[m]) if norm == "slaney" else 1.0)
    return fb


def band_lengths(fb):                                                   # first to last non-zero weight; 0 for an all-zero column
    nz = np.asarray(fb) != 0
    return np.where(nz.any(0), fb.shape[0] - nz[::-1].argmax(0) - nz.argmax(0), 0)


def project(fb, P):                                                     # [..., frames, bins] -> [..., frames, filters] in float64
    return P.astype(np.float64) @ np.asarray(fb, np.float64)


def projection_bound(fb, P, extra=1):
    """``(L + extra) u sum_k |w_k| |P_k|`` per output, u of ``P``'s dtype."""
    return (band_lengths(fb) + extra) * U[P.dtype] * project(np.abs(fb), np.abs(P))


def within(got, exact, bound, what):
    """``got [..., filters, frames]`` against ``exact`` / ``bound [..., frames, filters]``; prints the largest fraction reached."""
    err = np.abs(np.swapaxes(np.asarray(got), -1, -2).astype(np.float64) - exact)
    assert err.shape == bound.shape and np.isfinite(err).all(), what
    frac = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{what}: {frac:.3e} of the bound")
    assert (err <= bound).all(), f"{what}: {frac:.3e} of the bound"
    return frac


def from_samples(fb, s, B, power, dtype):
    """(exact result, bound) ``[rows, frames, filters]`` from the rounded windowed samples ``s`` and their frame bound ``B``."""
    X = np.abs(np.fft.rfft(s.astype(np.float64), axis=-1))
    w = np.asarray(fb, np.float64)
    norm2 = np.linalg.norm(X, axis=-1)[..., None]
    B = B[..., None]
    lead = np.abs(w).max(0) * (2 * norm2 * B + B * B) if power == 2.0 else np.linalg.norm(w, axis=0) * B
    P = X * X if power == 2.0 else X
    factor = 2.0 if np.dtype(dtype) == np.float64 else 1.0            # float64 signals: twice the bound, as for the STFT
    return project(w, P), factor * (lead + (band_lengths(w) + 3) * U[np.dtype(dtype)] * project(np.abs(w), P))
