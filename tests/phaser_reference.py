"""The phaser's definition (include/torchfx_hip.h, tfx_phaser_forward) as a per-sample loop, independent of the product's scan
paths, with a numpy.longdouble twin, and the two bounds the tests hold the product to.

    a[n]   = (g - 1) / (g + 1),  g = tan(w fc),  fc = min_freq exp(Lg (0.5 + 0.5 l)),  l = lfo(frac(n inc) + frac(phase + c spread))
    x_k[n] = a[n] x_{k-1}[n] + x_{k-1}[n-1] - a[n] x_k[n-1],  k = 1..N;      y[n] = dry x_0[n] + wet x_N[n]

The coefficient and the recursion are judged apart, so that neither hides the other.

1. Coefficient: |a - a_ld| <= delta_a, a_ld the track below in long double.  Steps 1 and 2 (off, t = double(n) inc, a_ = (t -
   floor(t)) + off) are IEEE operations the definition fixes, so the long-double track takes their float64 values and goes on
   in long double from a_.  delta_a is derived, not tuned, from the errors of steps 3 to 5, to first order (u = 2^-53):
     l    sine, device: sinpi(2 a_), 2 a_ exact, 2 ulp (ROCm's documented bound for the float64 sinpi) of a value <= 1: 4 u.
          sine, host: fl(fl(2 pi) a_) <= 4 pi < 16 carries 8 u of rounding + 4 u from pi's own error, then 1 ulp of sin: 14 u.
          triangle: a_ + 0.25 < 4 rounds by 2 u, times 4, plus the last subtraction: 9 u.            => delta_l = 16 u = 2^-49
     fc   h = 0.5 + 0.5 l: delta_l / 2 + u / 2;  Lg h: relative u;  exp: 1 ulp = 2 u relative (ROCm's bound for the float64 exp;
          glibc's is below it);  min_freq *: u.  |dfc/dl| = fc Lg / 2, so relatively
          rho_fc = Lg (delta_l / 2 + u / 2 + u) + 3 u
     g    v = w fc: relative u;  tan: 2 ulp = 4 u relative (ROCm's bound for the float64 tan);  |dg/dv| = 1 + g^2, so
          |dg| <= (1 + g^2) v (rho_fc + u) + 4 u g
     a    |da/dg| = 2 / (1 + g)^2 <= 2;  g - 1, g + 1 and the division round by u each of a value below 1: 3 u.  With
          2 (1 + g^2) / (1 + g)^2 <= 2 and 2 g / (1 + g)^2 <= 1/2 for every g > 0:
          delta_a = 2 v_max (rho_fc + u) + 2 u + 3 u,   v_max = w max_freq <= 0.45 pi
   times 1.01 for the second-order terms.  At 48 kHz and a 200-2000 Hz sweep that is 1.3e-15, at 192 kHz and 10 Hz-0.45 fs 2.9e-14.

2. Recursion: the loop below is fed the coefficient bits of the path under test.  E_REF is the largest distance between the float64
   loop and its long-double twin on the same case; the product stays within 16 E_REF of the long-double result (the factor the
   project holds Freeverb's affine scan to), plus 2^-24 |ref| for float32 outputs."""
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def channel_offset(phase, spread, c):
    z = phase + float(c) * spread
    return z - math.floor(z)


def coef_track_ld(T, fs, min_freq, max_freq, rate, phase=0.0, spread=0.0, c=0, shape="sine", position=0):
    """a[n] for n = position .. position + T - 1 of channel index c, in long double from a_ on."""
    inc = rate / fs
    off = channel_offset(phase, spread, c)
    n = position + np.arange(T, dtype=np.int64)
    t = n.astype(np.float64) * inc
    a_ = ((t - np.floor(t)) + off).astype(LD)
    if shape == "sine":
        l = np.sin(_two_pi_ld() * a_)
    else:
        z = a_ + LD(0.25)
        l = LD(1) - LD(4) * np.abs((z - np.floor(z)) - LD(0.5))
    lg, w = LD(math.log(max_freq / min_freq)), LD(math.pi / fs)         # the two host doubles of the definition
    fc = LD(min_freq) * np.exp(lg * (LD(0.5) + LD(0.5) * l))
    g = np.tan(w * fc)
    return (g - LD(1)) / (g + LD(1))


def _two_pi_ld():
    # 2 pi to long-double precision: float64 pi plus its known remainder
    return LD(2) * (LD(math.pi) + LD(1.2246467991473532e-16))


def coef_tolerance(fs, min_freq, max_freq):
    """delta_a of the module docstring."""
    lg = math.log(max_freq / min_freq)
    rho_fc = lg * (8 * U + 0.5 * U + U) + 3 * U
    v_max = math.pi / fs * max_freq
    return 1.01 * (2.0 * v_max * (rho_fc + U) + 2 * U + 3 * U)


def phaser_loop(x, coef, stages, dry, wet, channels=1, state=None, dtype=np.float64):
    """The definition sample by sample in `dtype` (float64 or longdouble): x [rows, T], coef [C or 1, T] (row r uses coef[r mod C],
    or coef[0]), state [rows, N + 1] or None -> (unrounded y [rows, T], new state [rows, N + 1]), both in `dtype`."""
    x = np.asarray(x)
    rows, T = x.shape
    N = stages
    coef = np.asarray(coef)
    idx = (np.arange(rows) % channels) if coef.shape[0] > 1 else np.zeros(rows, dtype=np.int64)
    a = coef.astype(dtype)[idx]                                # [rows, T]
    s = np.zeros((rows, N + 1), dtype) if state is None else np.asarray(state).astype(dtype).copy()
    xd = x.astype(dtype)
    y = np.empty((rows, T), dtype)
    dry, wet = dtype(dry), dtype(wet)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(T):
            an = a[:, n]
            u = xd[:, n]
            x0 = u
            for k in range(1, N + 1):
                v = an * u + s[:, k - 1] - an * s[:, k]
                s[:, k - 1] = u
                u = v
            s[:, N] = u
            y[:, n] = dry * x0 + wet * u
    return y, s


def reference(x, coef, stages, dry, wet, channels=1, state=None):
    """(long-double result, its end state, E_REF) for a case: E_REF = max |float64 loop - long-double loop| over the outputs."""
    y64, _ = phaser_loop(x, coef, stages, dry, wet, channels, state, np.float64)
    yld, sld = phaser_loop(x, coef, stages, dry, wet, channels, state, LD)
    with np.errstate(invalid="ignore"):
        d = np.abs(y64.astype(LD) - yld)
    e_ref = float(np.nanmax(d)) if d.size else 0.0
    return yld, sld, e_ref


RATIOS = {}                                                    # dtype name -> largest |got - ref| / (16 E_REF [+ 2^-24 |ref|]) seen


def check(got, yld, e_ref, what=""):
    """Print the largest deviation in units of the bound; pass only within 16 E_REF (+ 2^-24 |ref| for float32)."""
    got = np.asarray(got)
    assert got.shape == yld.shape, f"{what}: shape {got.shape} != {yld.shape}"
    if got.size == 0:
        return 0.0
    bound = 16.0 * e_ref + (2.0 ** -24 * np.abs(yld).astype(np.float64) if got.dtype == np.float32 else 0.0)
    dev = np.abs(got.astype(LD) - yld).astype(np.float64)
    assert np.all(np.isfinite(dev)), f"{what}: non-finite deviation"
    worst = float(dev.max())
    ratio = float((dev / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{what}: largest deviation {worst:.3e}, E_REF {e_ref:.3e}, largest deviation / bound {ratio:.3f} (<= 1 passes)")
    RATIOS[got.dtype.name] = max(RATIOS.get(got.dtype.name, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: deviation {worst:.3e} is {ratio:.2f} times the bound (E_REF {e_ref:.3e})"
    return ratio


def check_coef(coef, fs, min_freq, max_freq, rate, phase=0.0, spread=0.0, shape="sine", position=0, what=""):
    """coef [C or 1, T] float64 against the long-double track of every channel index it holds."""
    coef = np.asarray(coef)
    assert coef.dtype == np.float64
    tol = coef_tolerance(fs, min_freq, max_freq)
    worst = 0.0
    for c in range(coef.shape[0]):
        ref = coef_track_ld(coef.shape[1], fs, min_freq, max_freq, rate, phase, spread, c, shape, position)
        if coef.shape[1]:
            worst = max(worst, float(np.abs(coef[c].astype(LD) - ref).max()))
        assert np.all(np.abs(coef[c]) < 1.0), f"{what}: |a[n]| >= 1"
    print(f"{what}: largest coefficient deviation {worst:.3e}, delta_a {tol:.3e}")
    assert worst <= tol, f"{what}: coefficient deviation {worst:.3e} exceeds delta_a {tol:.3e}"
    return worst
