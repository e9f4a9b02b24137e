"""The loudness oracle: ITU-R BS.1770-4 block energies and gated loudness in NumPy, with SciPy's ``sosfilt`` in float64.

Nothing here imports the product.  Definitions (the ones the product documents):

* K-weighting at ``fs`` from the analogue prototypes behind the standard's 48 kHz table (bilinear transform with
  ``K = tan(pi f0 / fs)``).
* Sub-block ``i`` holds the samples ``[e_i, e_(i+1))`` with ``e_i = (i * num) // den`` (100 ms: ``num / den = fs / 10``);
  ``nblk = (T * den) // num``; ``S[r, i]`` is the sum of the squares of the filtered row over the sub-block.
* A NaN / Inf sample makes non-finite the sub-block that holds it and every later one of its row (the recursion never
  forgets one; a cascade whose sections are all FIR would, and the rule still stands).
* Gating: windows of four sub-blocks at a hop of one, absolute gate at -70 LUFS, relative gate 10 LU under the loudness
  of the mean of the absolutely gated windows; ``-inf`` with no window or none above the absolute gate, NaN with any NaN
  window.
"""
import math

import numpy as np
from scipy.signal import sosfilt


def kweighting_sos(fs):
    def section(f0, q, vh=None, vb=None):
        k = math.tan(math.pi * f0 / fs)
        a0 = 1 + k / q + k * k
        a = [1.0, 2 * (k * k - 1) / a0, (1 - k / q + k * k) / a0]
        if vh is None:
            return [1.0, -2.0, 1.0] + a
        return [(vh + vb * k / q + k * k) / a0, 2 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0] + a

    vh = 10 ** (3.999843853973347 / 20)
    return np.array([section(1681.974450955533, 0.7071752369554196, vh, vh ** 0.4996667741545416),
                     section(38.13547087602444, 0.5003270373238773)])


def edges(T, num, den=1):
    nblk = (T * den) // num
    return np.array([(i * num) // den for i in range(nblk + 1)], dtype=np.int64)


def filtered(x, sos):
    """The float64 cascade along the last axis, from zero state."""
    with np.errstate(invalid="ignore", over="ignore"):
        return sosfilt(np.asarray(sos, dtype=np.float64), np.asarray(x, dtype=np.float64), axis=-1)


def block_energy(x, sos, num, den=1, y=None):
    """``S [.., nblk]`` of ``x [.., T]``; every sub-block at or after a row's first non-finite input sample is NaN unless
    the recursion already made it non-finite."""
    x = np.asarray(x)
    e = edges(x.shape[-1], num, den)
    y = filtered(x, sos) if y is None else y
    s = np.zeros(x.shape[:-1] + (len(e) - 1,))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(e) - 1):
            s[..., i] = np.sum(y[..., e[i]:e[i + 1]] ** 2, axis=-1)
    if s.size == 0:
        return s
    bad = ~np.isfinite(np.asarray(x, dtype=np.float64))
    rows = s.reshape(-1, s.shape[-1])
    for r, b in enumerate(bad.reshape(-1, x.shape[-1])):
        if b.any():
            p = int(np.argmax(b))
            first = int(np.searchsorted(e, p, side="right")) - 1
            tail = rows[r, first:]
            tail[np.isfinite(tail)] = np.nan
    return s


def window_power(s, fs, weights=None, width=4):
    """``P [.., J]`` from ``S [.., C, nblk]``: the weighted mean square of the windows of ``width`` sub-blocks."""
    s = np.asarray(s, dtype=np.float64)
    channels, nblk = s.shape[-2], s.shape[-1]
    w = np.ones(channels) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (channels,):
        raise ValueError("one weight per channel")
    count = max(0, nblk - width + 1)
    e = np.array([(i * fs) // 10 for i in range(nblk + 1)], dtype=np.int64)
    p = np.zeros(s.shape[:-2] + (count,))
    for j in range(count):
        z = np.sum(s[..., j:j + width], axis=-1) / float(e[j + width] - e[j])
        p[..., j] = np.sum(w * z, axis=-1)
    return p


def lufs(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10 * np.log10(p)


def gate(p):
    """One row of window powers -> (integrated loudness, absolute mask, both-gates mask, relative threshold)."""
    p = np.asarray(p, dtype=np.float64)
    none = np.zeros(len(p), dtype=bool)
    if len(p) == 0:
        return -math.inf, none, none, -math.inf
    if np.isnan(p).any():
        return math.nan, none, none, math.nan
    l = lufs(p)
    above = l > -70.0
    if not above.any():
        return -math.inf, above, none, -math.inf
    thr = float(lufs(np.mean(p[above]))) - 10.0
    both = above & (l > thr)
    return float(lufs(np.mean(p[both]))) if both.any() else math.nan, above, both, thr


def signal_block_energy(x, fs):
    return block_energy(x, kweighting_sos(fs), fs, 10)


def _as_items(x):
    x = np.asarray(x)
    return x.reshape((1, 1) + x.shape) if x.ndim == 1 else (x[None] if x.ndim == 2 else x), x.ndim


def integrated_loudness(x, fs, weights=None):
    items, nd = _as_items(x)
    out = np.array([gate(window_power(signal_block_energy(it, fs), fs, weights))[0] for it in items])
    return out if nd == 3 else float(out[0])


def windowed_loudness(x, fs, weights=None, width=4):
    items, nd = _as_items(x)
    out = np.stack([lufs(window_power(signal_block_energy(it, fs), fs, weights, width)) for it in items])
    return out if nd == 3 else out[0]


def gating_signal(fs, T, dtype=np.float32):
    """Three channels of uniform noise whose thirds have the envelopes 1, -36 dB and 1e-5: windows that pass both gates,
    windows between the gates and windows under the absolute gate."""
    x = np.random.default_rng(5).uniform(-1, 1, (3, T))
    env = np.ones(T)
    env[T // 3:2 * (T // 3)] = 10 ** (-36 / 20)
    env[2 * (T // 3):] = 1e-5
    return (x * env).astype(dtype)


GATING_WEIGHTS = [1.0, 1.0, 1.41]
GATING_CASES = [(8000, 48123), (44100, 132377), (11025, 55626)]
