"""Plain reference for the edge tests of csrc/effects.hip (tests/test_gpu_effects_edges.py, tests/test_effects_reference_host.py):
numpy only, no fixtures.  One definition per launch:

    gain        y = x * dtype(g), then (clamp) v < -1 ? -1 : v > 1 ? 1 : v      -- one rounding: exact, NaN stays NaN
    absmax      max |x|, NaN anywhere wins (torch.max)                           -- exact
    sumsq       sum x^2, exactly rounded (float32 squares are exact in float64)  -- the device sums in float64, any order
    normalize   s = dtype(stat);  y = s > 0 ? (x / s) * dtype(peak) : x           -- two correctly rounded operations: exact
    delay line  c = dtype(mix * decay);  y*[n] = x[n] + c * v[n - D] over v = [hist | x] (no term for an index before v)

The delay line's two operations may be fused on the device or not (the build contracts within a statement), so its reference
is the exact value y* with the per-sample bound eps * (|c v[n - D]| + |y*|), eps = 2^-24 / 2^-53.  Two roundings give
fl(x + fl(c v)) - y* = c v d1 (1 + d2) + y* d2 with |d| <= eps / (1 + eps) (round to nearest), and (1 + 2 eps) <= (1 + eps)^2, so
the error is below eps |c v| + eps |y*|; the fused evaluation rounds once: below eps |y*|.  Derived, not measured (results in
the subnormal range are not used).  np.longdouble holds c * v exactly for float32 (48 bits of 64) and to 2^-64 for float64."""
import math

import numpy as np

EPS = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def gain_ref(x, g, clamp):
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        y = x * x.dtype.type(g)
        if clamp:
            one = x.dtype.type(1)
            y = np.where(y < -one, -one, np.where(y > one, one, y))        # a NaN fails both comparisons and is kept
    assert y.dtype == x.dtype
    return y


def absmax_ref(x):
    """max |x| over the last axis as float64; NaN if any element is NaN; 0 for an empty row."""
    a = np.abs(np.asarray(x)).astype(np.float64)
    if a.shape[-1] == 0:
        return np.zeros(a.shape[:-1])
    return np.where(np.isnan(a).any(axis=-1), np.nan, np.fmax.reduce(a, axis=-1))


def sumsq_ref(x):
    """sum x^2 over the last axis, rounded once to float64 (math.fsum of float64 squares: exact for float32 input; float64
    input goes through np.longdouble squares, exact to 2^-64)."""
    x = np.asarray(x)
    rows = x.reshape(-1, x.shape[-1])
    if x.dtype == np.float32:
        out = [math.fsum((r.astype(np.float64) ** 2).tolist()) for r in rows]
    else:
        out = [float(np.sum(r.astype(np.longdouble) ** 2, dtype=np.longdouble)) for r in rows]
    return np.array(out, np.float64).reshape(x.shape[:-1])


def rms_ref(x):
    """sqrt(sumsq / n) in float64, as stat_forward(RMS) decodes it."""
    with np.errstate(all="ignore"):
        return np.sqrt(sumsq_ref(x) / np.float64(np.asarray(x).shape[-1]))


def normalize_apply_ref(x, s, peak):
    """x [rows, T] (or [T]); s: the statistic as float64, one value or one per row."""
    x = np.asarray(x)
    dt = x.dtype.type
    with np.errstate(all="ignore"):
        sd = np.asarray(s, np.float64).astype(x.dtype)
        sd = sd.reshape(-1, 1) if sd.size > 1 else sd.reshape(())
        on = np.broadcast_to(sd > 0, x.shape)                                # False for 0 and for NaN
        y = np.where(on, (x / np.where(sd > 0, sd, dt(1))) * dt(peak), x)
    assert y.dtype == x.dtype
    return y


def delay_line_ref(x, D, decay, mix, hist=None):
    """(y*, bound, term) as np.longdouble / float64 / float64 arrays of x's shape [rows, T]: the exact result, its per-sample
    bound and |c v[n - D]| (0 where nothing is added)."""
    x = np.asarray(x)
    assert x.ndim == 2 and D >= 0
    rows, T = x.shape
    c = np.longdouble(x.dtype.type(mix * decay))
    h = np.zeros((rows, D), x.dtype) if hist is None else np.asarray(hist)
    assert h.shape == (rows, D) and h.dtype == x.dtype
    v = np.concatenate([h, x], axis=1).astype(np.longdouble)                # v[j] = sample n = j - D
    with np.errstate(all="ignore"):
        add = c * v[:, :T]                                                   # v[n - D + D]
        if hist is None:
            add[:, :min(D, T)] = 0                                           # no term at all (an inf before the row start adds nothing)
        y = x.astype(np.longdouble) + add
        term = np.abs(add).astype(np.float64)
        bound = EPS[x.dtype] * (term + np.abs(y).astype(np.float64))
    return y, bound, term


def hist_ref(x, D, hist=None):
    """The newest D samples of [hist | x] per row (hist None = zeros)."""
    x = np.asarray(x)
    h = np.zeros((x.shape[0], D), x.dtype) if hist is None else np.asarray(hist)
    return np.concatenate([h, x], axis=1)[:, x.shape[1]:]
