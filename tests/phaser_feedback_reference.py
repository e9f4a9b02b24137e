"""The phaser with feedback (include/torchfx_hip.h, tfx_phaser_feedback_forward) as a per-sample loop in float64 and in
numpy.longdouble, independent of the product's blocked paths.  The coefficient track is tests/phaser_reference.py's; the bound is
its rule applied to this loop: within 16 E_REF of the long-double result, E_REF the case's own max |loop64 - loop_ld|, plus
2^-24 |ref| for float32 outputs.

    u[n] = x[n] + feedback x_N[n-1];  x_0[n] = u[n];  x_k[n] = a[n] x_{k-1}[n] + x_{k-1}[n-1] - a[n] x_k[n-1];  y[n] = dry x[n] + wet x_N[n]"""
import numpy as np

from tests.phaser_reference import LD, check, check_coef  # noqa: F401  (the track's check and the bound, shared)


def loop(x, coef, stages, dry, wet, feedback, channels=1, state=None, dtype=np.float64):
    """x [rows, T], coef [C or 1, T], state [rows, N + 1] or None -> (unrounded y [rows, T], end state), both in `dtype`."""
    x = np.asarray(x)
    rows, T = x.shape
    N = stages
    idx = (np.arange(rows) % channels) if coef.shape[0] > 1 else np.zeros(rows, dtype=np.int64)
    a = np.asarray(coef).astype(dtype)[idx]
    s = np.zeros((rows, N + 1), dtype) if state is None else np.asarray(state).astype(dtype).copy()
    xd = x.astype(dtype)
    y = np.empty((rows, T), dtype)
    dry, wet, fb = dtype(dry), dtype(wet), dtype(feedback)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(T):
            an = a[:, n]
            u = xd[:, n] + fb * s[:, N]
            for k in range(1, N + 1):
                v = an * u + s[:, k - 1] - an * s[:, k]
                s[:, k - 1] = u
                u = v
            s[:, N] = u
            y[:, n] = dry * xd[:, n] + wet * u
    return y, s


def reference(x, coef, stages, dry, wet, feedback, channels=1, state=None):
    """(long-double result, its end state, E_REF = max |float64 loop - long-double loop| over the outputs)."""
    y64, _ = loop(x, coef, stages, dry, wet, feedback, channels, state, np.float64)
    yld, sld = loop(x, coef, stages, dry, wet, feedback, channels, state, LD)
    return yld, sld, float(np.abs(y64.astype(LD) - yld).max())
