"""The waveshaper's definition in float64 (or numpy's long double) from the dtype-rounded taps, and its per-sample bound
(tests/test_waveshaper_host.py, tests/test_gpu_waveshaper.py).  numpy only.

    u = resample(x, L, 1);  v = drive u + bias;  w = f(v) - c0;  z = resample(w, 1, L);  y = dry x + wet z

with the resampler of tests/resample_reference.py (zeros outside the signal), drive, bias, c0, dry and wet as the signal's dtype
holds them, and every operation after that in the wide type.

The bound, per output sample, for a kernel that works in the signal's dtype (u its unit roundoff, gamma(n) = n u / (1 - n u)):

    |y - y_ref| <= wet ( sum|h_dn| e_w + gamma(Lp_dn) sum|h_dn| |w| ) + 2u (|dry x| + |wet z|)
    e_w = Lip(f) ( drive gamma(Lp_up) sum|h_up| |x| + 2u |v| ) + E_SHAPE u (|w| + |c0|) + u |w|

Lip(f) = 1 for hard and tanh, 1.5 for cubic, max|dc| (N - 1) / 2 for a curve.  E_SHAPE is the transfer function's own largest
error over u |f(v)|: measured by tools/shape_sweep.cpp for the float32 tanh and cubic (its max_rel_u column, rounded up: 5 and
2), 8 for the float64 device tanh (a stated cap), 0 for hard.  A curve's lookup error is not relative to its value (a table may
cross zero), so it enters e_w as the absolute term of `curve_abs_error`, derived there from the rule's roundings.  The E_SHAPE
term multiplies |f(v)| <= |w| + |c0|, not |w|: the function's error is relative to its own value, and under a bias the
difference w = f(v) - c0 can be far smaller than f(v) (a silent stretch has w = 0 exactly in the reference, while the kernel's
f(bias) and the float64-evaluated c0 differ by that error).  With bias = 0, c0 = 0 and the term is E_SHAPE u |w|.
"""
import numpy as np

from tests import resample_reference as RR
from tests.fir_reference import gamma

E_SHAPE_F32 = {"hard": 0, "cubic": 2, "tanh": 5}       # tools/shape_sweep.cpp, max_rel_u rounded up to a whole unit
E_TANH_F64 = 8


def np_dtype(x):
    return np.asarray(x).dtype.type


def shape_wide(v, shape, curve=None):
    """f in the precision of v (float64 or long double)."""
    if shape == "hard":
        return np.minimum(np.maximum(v, -1), 1)
    if shape == "cubic":
        c = np.minimum(np.maximum(v, -1), 1)
        return 1.5 * c - 0.5 * c * c * c
    if shape == "tanh":
        return np.tanh(v)
    c = np.asarray(curve).astype(v.dtype)
    n = len(c)
    pos = np.minimum(np.maximum((v + 1) * ((n - 1) / v.dtype.type(2)), 0), n - 1)
    i = np.minimum(np.floor(pos), n - 2).astype(np.int64)
    return c[i] + (pos - i) * (c[i + 1] - c[i])


def lipschitz(shape, curve=None):
    if shape == "cubic":
        return 1.5
    if shape == "curve":
        c = np.asarray(curve, np.float64)
        return float(np.abs(np.diff(c)).max()) * (len(c) - 1) / 2.0
    return 1.0


def e_shape(shape, dt, curve=None):
    """E_SHAPE: the function's own largest error over u |f|; 0 for hard (exact) and for a curve, whose lookup error is not
    relative to its value and enters the bound through `curve_abs_error`."""
    if shape == "curve" or shape == "hard":
        return 0
    if dt == np.float32:
        return E_SHAPE_F32[shape]
    return E_TANH_F64 if shape == "tanh" else E_SHAPE_F32[shape]          # float64 cubic: the same three roundings


def curve_abs_error(v, curve, u):
    """Absolute error of the table lookup for the exact argument v: the two roundings of pos move it by 2u |pos| <= 2u (N - 1)
    columns of slope max|dc| each; the difference, the product and the sum round at most 3u (2 max|c|)."""
    c = np.asarray(curve, np.float64)
    n = len(c)
    return 2 * u * (n - 1) * float(np.abs(np.diff(c)).max()) + 6 * u * float(np.abs(c).max()) + 0 * np.abs(v)


def params(dt, drive_db=0.0, bias=0.0, mix=1.0, output_db=0.0):
    """drive, bias, dry, wet as dtype dt holds them (float64 values)."""
    return (float(dt(10.0 ** (drive_db / 20.0))), float(dt(bias)), float(dt(1.0 - mix)), float(dt(mix * 10.0 ** (output_db / 20.0))))


def c0_of(dt, shape, bias, curve=None):
    """f(bias) in float64 from the dtype-rounded bias and curve, rounded to dt."""
    c = None if curve is None else np.asarray(curve).astype(dt).astype(np.float64)
    return float(dt(shape_wide(np.array([float(dt(bias))], np.float64), shape, c)[0]))


def ref(x, L, h_up, h_dn, shape, drive_db=0.0, bias=0.0, mix=1.0, output_db=0.0, curve=None, wide=False, parts=False):
    """The definition for x [T] or [C, T] of dtype float32 / float64, taps as the product runs them (design_taps, in x's dtype).
    Returns y in float64 / long double (and the intermediates with `parts`)."""
    x = np.asarray(x)
    dt = np_dtype(x)
    acc = np.longdouble if wide else np.float64
    drive, b, dry, wet = params(dt, drive_db, bias, mix, output_db)
    c0 = c0_of(dt, shape, bias, curve)
    cq = None if curve is None else np.asarray(curve).astype(dt)
    u = RR.ref(x, h_up, L, 1, wide) if L > 1 else x.astype(acc)
    v = acc(drive) * u + acc(b)
    w = shape_wide(v, shape, cq) - acc(c0)
    z = RR.ref(w, h_dn, 1, L, wide) if L > 1 else w
    y = acc(dry) * x.astype(acc) + acc(wet) * z
    return (y, u, v, w, z, (drive, b, dry, wet, c0)) if parts else y


def bound(x, L, h_up, h_dn, Lp_up, Lp_dn, shape, drive_db=0.0, bias=0.0, mix=1.0, output_db=0.0, curve=None):
    """The per-sample bound of the module docstring, float64 [like x]."""
    x = np.asarray(x)
    dt = np_dtype(x)
    uu = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    _, u, v, w, z, (drive, b, dry, wet, c0) = ref(x, L, h_up, h_dn, shape, drive_db, bias, mix, output_db, curve, parts=True)
    u, v, w, z = (np.abs(np.asarray(a, np.float64)) for a in (u, v, w, z))
    lip = lipschitz(shape, curve)
    ax = np.abs(x.astype(np.float64))
    if L > 1:
        hu, hd = np.abs(np.asarray(h_up, np.float64)), np.abs(np.asarray(h_dn, np.float64))
        su = RR.ref(ax, hu, L, 1)
        g_up, g_dn = gamma(Lp_up, uu), gamma(Lp_dn, uu)
    else:
        su, g_up, g_dn = ax, 0.0, 0.0
    e_w = lip * (abs(drive) * g_up * su + 2 * uu * v) + e_shape(shape, dt, curve) * uu * (w + abs(c0)) + uu * w
    if shape == "curve":
        e_w = e_w + curve_abs_error(v, np.asarray(curve).astype(dt), uu)
    if L > 1:
        filt = RR.ref(e_w, hd, 1, L) + g_dn * RR.ref(w, hd, 1, L)
    else:
        filt = e_w
    return abs(wet) * filt + 2 * uu * (np.abs(dry) * ax + abs(wet) * z)


def check(y, x, L, h_up, h_dn, Lp_up, Lp_dn, shape, what="", **kw):
    """Assert |y - ref| <= bound per sample; returns the largest observed fraction of the bound."""
    x = np.asarray(x)
    wide = np_dtype(x) == np.float64
    r = ref(x, L, h_up, h_dn, shape, wide=wide, **kw)
    bd = bound(x, L, h_up, h_dn, Lp_up, Lp_dn, shape, **kw)
    y = np.asarray(y)
    assert y.shape == x.shape and y.dtype == x.dtype, (what, y.shape, y.dtype)
    err = np.abs(y.astype(r.dtype) - r).astype(np.float64)
    assert np.isfinite(err).all(), f"{what}: non-finite output"
    tiny = np.finfo(np_dtype(x)).tiny
    frac = float((err / (bd + tiny)).max()) if err.size else 0.0
    k = int(np.argmax(err / (bd + tiny))) if err.size else 0
    print(f"waveshaper {what}: largest fraction of the bound {frac:.3f} (err {err.reshape(-1)[k]:.3e}, bound {bd.reshape(-1)[k]:.3e})")
    assert frac <= 1.0, f"{what}: error {err.reshape(-1)[k]:.3e} is {frac:.2f} of the bound {bd.reshape(-1)[k]:.3e} at {k}"
    return frac


def reach_probe(fn, T, i):
    """Outputs of `fn` (a 1-D float64 array -> array) that a NaN at input i turns NaN: (first, last)."""
    x = np.zeros(T)
    x[i] = np.nan
    bad = np.flatnonzero(np.isnan(fn(x)))
    return int(bad.min()), int(bad.max())
