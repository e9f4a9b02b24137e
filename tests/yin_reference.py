"""The reference of the YIN tests: the definition of ``torchfx_amd.pitch.yin`` in extended precision (``numpy.longdouble``, at
least float64) from the same rounded samples, the derived error bounds, and the pick (steps 4 and 5) on a given array.

The bound on ``d'``.  With unit roundoff u, every term ``fl(fl(a - b)^2)`` of ``d(tau)`` carries at most 2 roundings and then
passes through at most W - 1 additions (in any order: blocks, then the blocks' sums), so ``d^(tau) = sum t_j (1 + theta_j)``
with ``|theta_j| <= gamma(W + 1)``, ``gamma(n) = n u / (1 - n u)``; all terms are non-negative, so the same relative bound holds
for the sum.  ``S(tau)`` adds tau such values in tau - 1 more additions: relative error ``gamma(W + tau)``.  ``d' = tau d / S``
takes a product and a quotient (the conversion of tau is exact; the quotient is allowed 3 roundings, for a division that is
not correctly rounded): ``(1 + theta_{W+1}) (1 + theta_4) / (1 + theta_{W+tau})``.  Numerator and denominator err independently
-- the numerator's roundings do not cancel against the denominator's -- so the quotient is within ``gamma(2 W + tau + 6)`` of
the exact one (Higham, Accuracy and Stability, Lemma 3.3, rounded up by one).  That is the form ``gamma(W + tau + c) d'`` with
``c = W + 6``.  Where ``S(tau) = 0`` every term is exactly 0 and ``d' = 1`` exactly.
"""
import math

import numpy as np

L = np.longdouble


def unit(dtype) -> float:
    return float(np.finfo(dtype).eps) / 2


def lags(fs, fmin, fmax):
    return max(1, int(math.floor(fs / fmax))), int(math.ceil(fs / fmin))


def cmndf_bound(W: int, n_lags: int, dtype) -> np.ndarray:
    """``gamma(2 W + tau + 6)`` for tau = 0 .. n_lags - 1, for the arithmetic of ``dtype`` plus the reference's own."""
    n = 2 * W + np.arange(n_lags, dtype=np.float64) + 6
    return sum(n * u / (1 - n * u) for u in (unit(dtype), unit(L)))


def pick(cm, fs, tau_min, tau_max, threshold):
    """Steps 4 and 5 on one frame's ``d'`` in its dtype: ``(tau, delta, f0, aperiodicity)``."""
    R = cm.dtype.type
    tau = None
    for t in range(tau_min, tau_max + 1):
        if cm[t] < R(threshold):
            tau = t
            while tau < tau_max and cm[tau + 1] < cm[tau]:
                tau += 1
            break
    if tau is None:
        tau = min(range(tau_min, tau_max + 1), key=lambda t: (cm[t], t))
    a, b, c = cm[tau - 1], cm[tau], cm[tau + 1]
    den = a - R(2) * b + c
    delta = R(0.5) * (a - c) / den if den > 0 and b <= a and b <= c else R(0)
    return tau, delta, R(fs) / (R(tau) + delta), b


def f0_tolerance(cm, tau, fs, beta, u) -> float:
    """How far ``f0 = fs / (tau + delta)`` may move when a, b, c = cm[tau - 1 .. tau + 1] each move by the relative ``beta`` and
    the parabola and the division are rounded with unit roundoff ``u`` (the sum over both sides of a comparison).  With
    ``den = a - 2 b + c``: ``|d delta| <= beta / 2 ((a + c) / den + |a - c| (a + 2 b + c) / den^2)`` from the data, and
    ``|delta| (2 K + 5) u`` with ``K = (a + 2 b + c) / den`` from the rounding (two additions of terms up to a + 2 b + c in den,
    one subtraction, a quotient of up to 3 roundings, the halving exact); then ``f0`` moves by ``f0 d delta / (tau + delta)`` and
    by 5 u of itself (fs, the sum, a quotient of up to 3 roundings)."""
    a, b, c = (float(v) for v in cm[tau - 1:tau + 2])
    den = a - 2 * b + c
    ddelta, delta = 0.0, 0.0
    if den > 0 and b <= a and b <= c:
        K = (a + 2 * b + c) / den
        delta = 0.5 * (a - c) / den
        ddelta = 0.5 * beta * ((a + c) / den + abs(a - c) * K / den) + abs(delta) * (2 * K + 5) * u
    f0 = fs / (tau + delta)
    return f0 * (ddelta / (tau + delta) + 5 * u)


def reference(x, fs, fmin, fmax, frame_length, win_length, hop, threshold=0.1, center=True, pad_mode="constant"):
    """``x [..., T]`` (already rounded to its dtype) -> dict of ``cmndf [..., frames, Lmax + 1]`` (longdouble), ``tau``, ``f0``,
    ``aper`` ``[..., frames]`` and ``bad`` (the frames whose W + Lmax samples are not all finite; their tau is -1, the rest NaN)."""
    tau_min, tau_max = lags(fs, fmin, fmax)
    Lmax, W, pad = tau_max + 1, win_length, frame_length // 2 if center else 0
    rows = np.asarray(x).reshape(-1, x.shape[-1])
    xp = np.pad(rows, ((0, 0), (pad, pad)), mode=pad_mode) if pad else rows
    frames = 1 + (xp.shape[-1] - frame_length) // hop
    fr = np.stack([xp[:, f * hop:f * hop + W + Lmax] for f in range(frames)], axis=1).astype(L)
    with np.errstate(invalid="ignore"):
        d = np.stack([np.square(fr[..., :W] - fr[..., t:t + W]).sum(axis=-1) for t in range(Lmax + 1)], axis=-1)
        S = np.cumsum(d[..., 1:], axis=-1)
        cm = np.ones_like(d)
        cm[..., 1:] = np.where(S == 0, L(1), np.arange(1, Lmax + 1) * d[..., 1:] / np.where(S == 0, L(1), S))
    bad = ~np.isfinite(fr).all(axis=-1)
    tau = np.full(bad.shape, -1)
    f0, ap = np.full(bad.shape, np.nan), np.full(bad.shape, np.nan)
    for i in zip(*np.nonzero(~bad)):
        tau[i], _, f0[i], ap[i] = pick(cm[i], fs, tau_min, tau_max, threshold)
    lead = x.shape[:-1]
    return dict(cmndf=cm.reshape(lead + cm.shape[1:]), tau=tau.reshape(lead + (frames,)), f0=f0.reshape(lead + (frames,)),
                aper=ap.reshape(lead + (frames,)), bad=bad.reshape(lead + (frames,)), tau_min=tau_min, tau_max=tau_max)


def tone(f, fs, T, dtype, noise=0.0, seed=0, shape=()):
    """Four harmonics of ``f`` with amplitudes 1 / k, plus ``noise`` times seeded Gaussian noise, rounded to ``dtype``."""
    t = np.arange(T) / fs
    x = sum(np.sin(2 * np.pi * k * f * t) / k for k in range(1, 5))
    return (x + noise * np.random.default_rng(seed).standard_normal(shape + (T,))).astype(dtype)


# the tone cases of the host and the device tests: fs 16000, 1024 / 512 / 128, fmin 60, fmax 1200; 57 frames, 47 interior
TONE = dict(fs=16000.0, fmin=60.0, fmax=1200.0, frame_length=1024, win_length=512, hop=128)
TONE_T = 7200
TONES = (110.0, 261.63, 440.0)
