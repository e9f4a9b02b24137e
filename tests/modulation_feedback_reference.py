"""The modulated delay line with feedback as a per-sample float64 loop (include/torchfx_hip.h,
tfx_modulated_delay_feedback_forward), the cases the host and device tests share, and the bound they hold the product to.
The bound is derived, not tuned: one pass through the voices is the feed-forward effect applied to the line w, whose error is
tests/modulation_reference.py's tol with E = max|w_ref| of the row; it enters w scaled by |feedback| and comes back through an
interpolant of norm L sum|g_v| (L = 1 linear, 1.25 cubic): a geometric series in rho = |feedback| L sum|g_v| < 1, so
|y - ref| <= tol / (1 - rho), plus 2^-24 |ref| for float32 results."""
import functools
import math

import numpy as np

from tests import modulation_reference as R

FS = 8000
T = 1500
DRY, SPREAD, POSITION = 0.7, 0.25, 12345
# name: ((delay, depth, rate, phase, gain) rows for linear interpolation -- cubic adds its one sample to every delay --, feedback,
# the block B = floor(min(delay - depth)) the plan must report)
TABLES = {
    "B1": ([(3.5, 2.25, 23.0, 0.0, 0.6)], 0.9, 1),                      # fully serial, 64 rows per wave
    "B5": ([(8.75, 3.5, 17.0, 0.1, -0.7)], 0.8, 5),                     # 12 rows per wave; 5 batch items leave a remainder
    "B47": ([(70.5, 23.25, 11.0, 0.4, 0.6)], -0.9, 47),                 # one row per wave, 17 idle lanes
    "B150": ([(170.3, 20.1, 29.0, 0.7, 0.5)], 0.95, 150),               # sub-blocks of 64, the last one short
    "two": ([(12.5, 4.25, 19.0, 0.0, 0.5), (40.0, 9.5, 7.0, 0.3, -0.4)], -0.8, 8),
}


def voices(name, interpolation):
    pad = 1.0 if interpolation == "cubic" else 0.0
    return [(b + pad, d, r, p, g) for b, d, r, p, g in TABLES[name][0]]


def feedback_ref(x, fs, table, feedback, dry=1.0, spread=0.0, shape="sine", interpolation="linear", position=0):
    """x [B, C, T] -> (y, w), both unrounded float64 [B, C, T]."""
    xr = np.asarray(x, dtype=np.float64)
    batch, C, n_samples = xr.shape
    rows = R.voice_rows(table, fs)
    y, w = np.empty_like(xr), np.zeros_like(xr)
    zero = np.zeros(batch)
    for c in range(C):
        offs = [(p + float(c) * spread) - math.floor(p + float(c) * spread) for _, _, _, p, _ in rows]
        for j in range(n_samples):
            r = 0.0
            for (base, depth, inc, _, gain), off in zip(rows, offs):
                i, f = R.delay_at(position + j, base, depth, inc, off, shape)
                at = lambda m: w[:, c, m] if m >= 0 else zero                       # noqa: E731
                m = j - i
                if interpolation == "linear":
                    wd = at(m) + f * (at(m - 1) - at(m))
                else:
                    wd = ((-f * (f - 1.0) * (f - 2.0) / 6.0) * at(m + 1) + ((f + 1.0) * (f - 1.0) * (f - 2.0) / 2.0) * at(m)
                          + (-(f + 1.0) * f * (f - 2.0) / 2.0) * at(m - 1) + ((f + 1.0) * f * (f - 1.0) / 6.0) * at(m - 2))
                r = r + gain * wd
            w[:, c, j] = xr[:, c, j] + feedback * r
            y[:, c, j] = dry * xr[:, c, j] + r
    return y, w


@functools.lru_cache(maxsize=None)
def case(name, interpolation, lfo):
    """(x float32 [5, 2, T] with float32-representable values, so one reference serves both dtypes; y_ref; w_ref), read-only."""
    x = np.random.default_rng(len(name)).uniform(-1.0, 1.0, (5, 2, T)).astype(np.float32)
    y, w = feedback_ref(x, FS, voices(name, interpolation), TABLES[name][1], DRY, SPREAD, lfo, interpolation, POSITION)
    for a in (x, y, w):
        a.setflags(write=False)
    return x, y, w


def check(got, name, interpolation, lfo, what, rows=slice(None), length=T, ref=None):
    """got (rows `rows`, first `length` samples of the case) within the bound of the loop's result (or of `ref`)."""
    _, y, w = case(name, interpolation, lfo)
    ref, got = y[rows, :, :length] if ref is None else ref, np.asarray(got)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    rho = abs(TABLES[name][1]) * sum(abs(v[4]) for v in TABLES[name][0]) * (1.25 if interpolation == "cubic" else 1.0)
    tol = R.tolerance(w[rows], FS, voices(name, interpolation), DRY) / (1.0 - rho)
    bound = tol + (2.0 ** -24 * np.abs(ref) if got.dtype == np.float32 else 0.0)
    dev = np.abs(got.astype(np.float64) - ref)
    share = float((dev / bound).max()) if dev.size else 0.0
    print(f"{what}: largest deviation {float(dev.max()) if dev.size else 0.0:.3e}, largest share of the bound {share:.3f}")
    assert np.isfinite(share) and share <= 1.0, f"{what}: the deviation is {share:.3f} of the bound"
