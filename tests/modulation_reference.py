"""The modulated delay line's definition as a per-sample float64 loop (include/torchfx_hip.h, tfx_modulated_delay_forward),
independent of the product's vectorised host path, and the error bound the tests hold the product to.

    y[n] = dry x[n] + sum_v g_v x(n - d_v[n]),   d_v[n] = base_v + depth_v lfo(frac(n inc_v) + frac(phase_v + c spread))

The bound is derived, not tuned.  With E = max|x| of the row and its history, G = sum |g_v|, depths and delays in samples:

    tol = E [2^-47 (|dry| + 1.25 G) + 2.4 sum_v |g_v| (depth_v 2^-47 + (base_v + depth_v) 2^-52)]

1.25 and 2.4 are the Lebesgue constant and the largest slope sum of the 4-point Lagrange interpolant (1.25 and 2.334; they cover
the linear one), 2^-47 allows for the LFO value (the rounding of 2 pi a for a < 2 plus a few ulp of either sine routine) and
the 2^-52 term for d being rounded once or twice.  float64 signals: |y - ref| <= tol; float32 signals: |y - ref| <= 2^-24 |ref| +
tol with ref unrounded float64 from the float32 input."""
import math

import numpy as np


def voice_rows(voices, fs):
    """(delay, depth, rate, phase, gain) rows -> (base, depth, inc, phase, gain)."""
    return [(float(b), float(d), float(r) / fs, float(p), float(g)) for b, d, r, p, g in voices]


def delay_at(n, base, depth, inc, off, shape):
    t = float(n) * inc
    a = (t - math.floor(t)) + off
    if shape == "sine":
        l = math.sin(2.0 * math.pi * a)
    else:
        z = a + 0.25
        l = 1.0 - 4.0 * abs((z - math.floor(z)) - 0.5)
    d = base + depth * l
    i = math.floor(d)
    return int(i), d - i


def modulated_delay_ref(x, fs, voices, dry=1.0, spread=0.0, shape="sine", interpolation="linear", position=0, hist=None):
    """x [T], [C, T] or [B, C, T] (float32 / float64 array) -> unrounded float64 of the same shape.  hist [rows, H]: the samples
    before x[..., 0] (None: silence)."""
    x = np.asarray(x)
    T = x.shape[-1]
    C = x.shape[-2] if x.ndim >= 2 else 1
    xr = x.reshape(-1, C, T).astype(np.float64)
    B = xr.shape[0]
    H = 0 if hist is None else hist.shape[-1]
    hr = None if hist is None else np.asarray(hist).reshape(B, C, H).astype(np.float64)
    rows = voice_rows(voices, fs)
    y = np.empty_like(xr)
    zero = np.zeros(B)

    def at(c, m):                       # sample m of channel c for every batch item
        if m >= 0:
            return xr[:, c, m]
        return hr[:, c, H + m] if hr is not None and m >= -H else zero

    for c in range(C):
        offs = []
        for base, depth, inc, phase, gain in rows:
            z = phase + float(c) * spread
            offs.append(z - math.floor(z))
        for j in range(T):
            acc = dry * xr[:, c, j]
            for (base, depth, inc, phase, gain), off in zip(rows, offs):
                i, f = delay_at(position + j, base, depth, inc, off, shape)
                m = j - i
                if interpolation == "linear":
                    x0 = at(c, m)
                    xd = x0 + f * (at(c, m - 1) - x0)
                else:
                    xd = ((-f * (f - 1.0) * (f - 2.0) / 6.0) * at(c, m + 1) + ((f + 1.0) * (f - 1.0) * (f - 2.0) / 2.0) * at(c, m)
                          + (-(f + 1.0) * f * (f - 2.0) / 2.0) * at(c, m - 1) + ((f + 1.0) * f * (f - 1.0) / 6.0) * at(c, m - 2))
                acc = acc + gain * xd
            y[:, c, j] = acc
    return y.reshape(x.shape)


def tolerance(x, fs, voices, dry, hist=None):
    """The bound per row, shaped to broadcast against x: [..., 1]."""
    x = np.asarray(x, dtype=np.float64)
    E = np.abs(x).max(-1, keepdims=True) if x.shape[-1] else np.zeros(x.shape[:-1] + (1,))
    if hist is not None and hist.shape[-1]:
        E = np.maximum(E, np.abs(np.asarray(hist, dtype=np.float64)).max(-1).reshape(E.shape))
    rows = voice_rows(voices, fs)
    G = sum(abs(g) for *_, g in rows)
    k = 2.0 ** -47 * (abs(dry) + 1.25 * G) + 2.4 * sum(abs(g) * (d * 2.0 ** -47 + (b + d) * 2.0 ** -52) for b, d, _, _, g in rows)
    return E * k


def check(got, ref, x, fs, voices, dry, hist=None, what=""):
    """Print the largest deviation and the largest excess over the bound; pass only with excess <= 0."""
    got = np.asarray(got)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    tol = np.broadcast_to(tolerance(x, fs, voices, dry, hist), ref.shape)
    bound = tol + (2.0 ** -24 * np.abs(ref) if got.dtype == np.float32 else 0.0)
    dev = np.abs(got.astype(np.float64) - ref)
    excess = float((dev - bound).max()) if dev.size else 0.0
    worst = float(dev.max()) if dev.size else 0.0
    print(f"{what}: largest deviation {worst:.3e}, largest excess over the bound {excess:.3e} (<= 0 passes), "
          f"smallest tol {float(tol.min()) if tol.size else 0.0:.3e}")
    assert np.isfinite(worst) and excess <= 0.0, f"{what}: deviation {worst:.3e} exceeds the bound by {excess:.3e}"
    return worst, excess


def at_work(ref, x, fs, voices, dry, what=""):
    """The effect does something: the result differs from dry * x by more than 100 tol somewhere in every row."""
    tol = tolerance(x, fs, voices, dry)
    gap = np.abs(ref - dry * np.asarray(x, dtype=np.float64))
    assert np.all(gap.max(-1, keepdims=True) > 100.0 * tol), f"{what}: the wet part is not at work"
