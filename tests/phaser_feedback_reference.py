"""The phaser with feedback (include/torchfx_hip.h, tfx_phaser_feedback_forward) as a per-sample loop in float64 and in
numpy.longdouble, independent of the product's blocked paths.  The coefficient track is tests/phaser_reference.py's; the bound is
its rule applied to this loop: within 16 E_REF of the long-double result, E_REF the case's own max |loop64 - loop_ld|, plus
2^-24 |ref| for float32 outputs.  The state is held to the same rule with its own figure: within 16 E_REF_S of the long-double
state at the same sample, E_REF_S the largest |state64 - state_ld| over every sample and every component of the case.

    u[n] = x[n] + feedback x_N[n-1];  x_0[n] = u[n];  x_k[n] = a[n] x_{k-1}[n] + x_{k-1}[n-1] - a[n] x_k[n-1];  y[n] = dry x[n] + wet x_N[n]"""
import collections

import numpy as np

from tests.phaser_reference import LD, check, check_coef  # noqa: F401  (the track's check and the bound, shared)

# y [rows, T] and state [rows, N + 1] in long double, E_REF, E_REF_S, states [rows, T, N + 1]: the long-double state after every sample
Ref = collections.namedtuple("Ref", "y state e_ref e_ref_s states")


def loop(x, coef, stages, dry, wet, feedback, channels=1, state=None, dtype=np.float64):
    """x [rows, T], coef [C or 1, T], state [rows, N + 1] or None -> (unrounded y [rows, T], end state, the state after every
    sample [rows, T, N + 1]), all in `dtype`."""
    x = np.asarray(x)
    rows, T = x.shape
    N = stages
    idx = (np.arange(rows) % channels) if coef.shape[0] > 1 else np.zeros(rows, dtype=np.int64)
    a = np.asarray(coef).astype(dtype)[idx]
    s = np.zeros((rows, N + 1), dtype) if state is None else np.asarray(state).astype(dtype).copy()
    xd = x.astype(dtype)
    y = np.empty((rows, T), dtype)
    states = np.empty((rows, T, N + 1), dtype)
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
            states[:, n] = s
    return y, s, states


def reference(x, coef, stages, dry, wet, feedback, channels=1, state=None):
    """Ref(long-double result, its end state, E_REF = max |float64 loop - long-double loop| over the outputs, E_REF_S = the same
    over the states after every sample, those states in long double)."""
    y64, _, s64 = loop(x, coef, stages, dry, wet, feedback, channels, state, np.float64)
    yld, sld, states = loop(x, coef, stages, dry, wet, feedback, channels, state, LD)
    e_ref = float(np.abs(y64.astype(LD) - yld).max()) if yld.size else 0.0
    e_ref_s = float(np.abs(s64.astype(LD) - states).max()) if states.size else 0.0
    return Ref(yld, sld, e_ref, e_ref_s, states)


STATE_RATIOS = {}                                              # label -> largest |state - state_ld| / (16 E_REF_S) seen


def check_state(got, want, e_ref_s, what="", label="state"):
    """The end state [rows, N + 1] (float64) within 16 E_REF_S of the long-double state; prints its share of the bound."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, f"{what}: state {got.dtype} {got.shape} != {want.shape}"
    dev = np.abs(got.astype(LD) - want).astype(np.float64)
    assert np.all(np.isfinite(dev)), f"{what}: non-finite state"
    ratio = float(dev.max()) / max(16.0 * e_ref_s, np.finfo(np.float64).tiny)
    print(f"{what}: largest state deviation {float(dev.max()):.3e}, E_REF_S {e_ref_s:.3e}, largest deviation / bound {ratio:.3f} (<= 1 passes)")
    STATE_RATIOS[label] = max(STATE_RATIOS.get(label, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: the state deviates by {float(dev.max()):.3e}, {ratio:.2f} times the bound (E_REF_S {e_ref_s:.3e})"
    return ratio
