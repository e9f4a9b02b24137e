"""Plain references for the resampler's edge tests (tests/test_gpu_resample_edges.py, tests/test_resample_reference_host.py):
numpy only, no fixtures.  With h the taps the product runs (`design_taps`: already scaled by up) and half = (nh - 1) // 2,

    y[m] = sum_i x[i] * h[m*down + half - i*up]        0 <= i < T, tap index in [0, nh),  m in [0, ceil(T*up/down))

which is scipy.signal.resample_poly's upfirdn with its n_pre_pad and n_pre_remove folded in: n_pre_remove * down =
half + n_pre_pad exactly, so (m + n_pre_remove)*down - n_pre_pad = m*down + half.
"""
import numpy as np

from tests.fir_reference import gamma, staircase  # noqa: F401  (staircase: re-exported for the resampler's tests)

_BLOCK = 1 << 21                      # elements of one gathered [outputs, taps] block


def n_out_of(T, up, down):
    return -(-T * up // down)


def ref(x, h, up, down, wide=False):
    """The definition in float64 (`wide`: numpy's long double, for judging the float64 kernel).  x [C, T] or [T]; returns
    [C, n_out] or [n_out] in the accumulation dtype.  Outputs m and m + up share their taps h[r::up], r = (m*down + half) % up,
    and their newest inputs lie `down` apart: one phase is one strided gather of x times one tap vector."""
    dt = np.longdouble if wide else np.float64
    x = np.asarray(x)
    flat = x.ndim == 1
    x2 = np.atleast_2d(x).astype(dt)
    h = np.asarray(h).reshape(-1).astype(dt)
    C, T = x2.shape
    nh, n_out = len(h), n_out_of(T, up, down)
    half = (nh - 1) // 2
    y = np.zeros((C, n_out), dt)
    if T == 0:
        return y[0] if flat else y
    L = -(-nh // up)                                       # the longest phase
    i_max = ((n_out - 1) * down + half) // up              # newest input any output asks for
    xp = np.zeros((C, L + max(i_max + 1, T)), dt)          # xp[:, L + i] = x[:, i], zeros around
    xp[:, L:L + T] = x2
    s_c, s_t = xp.strides
    for m0 in range(min(up, n_out)):
        c = m0 * down + half
        hr = h[c % up::up]
        if len(hr) == 0:
            continue
        E = (n_out - 1 - m0) // up + 1
        step = max(1, _BLOCK // (len(hr) * C))
        for e0 in range(0, E, step):
            e1 = min(E, e0 + step)
            first = L + c // up + e0 * down                # xp index of the newest input of output m0 + e0*up
            win = np.lib.stride_tricks.as_strided(xp[:, first:], shape=(C, e1 - e0, len(hr)), strides=(s_c, down * s_t, -s_t),
                                                  writeable=False)
            y[:, m0 + e0 * up:m0 + (e1 - 1) * up + 1:up] = win @ hr
    return y[0] if flat else y


def bound(x, h, up, down, Lp):
    """Per-output tolerance for a kernel that forms the Lp products of one phase and their sum in the dtype of `x`, in any
    order, fused or not: gamma(Lp + 1) * (|h| (*) |x|)[m] + Lp * tiny, gamma(n) = n u / (1 - n u) (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., section 3.1).  u = 2^-24, tiny = 2^-126 for float32; 2^-53, 2^-1022 for
    float64.  `Lp` is the per-phase tap count of the plan (resample_plan_info); terms that are exact zeros (bucket padding,
    samples outside the signal) round nothing and need no allowance.  Derived, not measured."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    u, tiny = (2.0 ** -24, 2.0 ** -126) if x.dtype == np.float32 else (2.0 ** -53, 2.0 ** -1022)
    s = ref(np.abs(x), np.abs(np.asarray(h).astype(np.float64)), up, down)
    return gamma(Lp + 1, u) * s + Lp * tiny


def reach_mask(T, n_out, up, down, pre_remove, Lp, bad, rows=None):
    """[rows, n_out] bool: output m of row r is true iff some (r, i) of `bad` has 0 <= (m + pre_remove)*down - i*up < Lp*up --
    the outputs whose Lp-term window x[n // up - j], j < Lp, n = (m + pre_remove)*down, holds input i.  Zero-valued taps and
    the zero padding up to Lp*up taps count (the contract at the top of csrc/resample.hip: every term SciPy adds is added)."""
    rows = 1 + max(r for r, _ in bad) if rows is None else rows
    mask = np.zeros((rows, n_out), bool)
    n = (np.arange(n_out, dtype=np.int64) + pre_remove) * down
    for r, i in bad:
        assert 0 <= i < T, (i, T)
        d = n - i * up
        mask[r] |= (d >= 0) & (d < Lp * up)
    return mask


def impulses(T, positions, amps, dtype=np.float32):
    """[T] zeros with x[p] = a for every (p, a) of zip(positions, amps)."""
    x = np.zeros(T, dtype)
    for p, a in zip(positions, amps):
        assert 0 <= p < T and x[p] == 0, (p, T)
        x[p] = a
    return x


def impulse_response(T, h, up, down, positions, amps):
    """What a row of `impulses` resamples to when no output sees two of them, in the dtype of `h`: amp * h[m*down + half - p*up]
    where that tap exists, else 0 -- one exact product per output (a power-of-two amplitude only shifts a normal tap's
    exponent)."""
    h = np.asarray(h).reshape(-1)
    nh, n_out = len(h), n_out_of(T, up, down)
    half = (nh - 1) // 2
    y = np.zeros(n_out, h.dtype)
    seen = np.zeros(n_out, bool)
    c = np.arange(n_out, dtype=np.int64) * down + half
    for p, a in zip(positions, amps):
        k = c - p * up
        ok = (k >= 0) & (k < nh)
        assert not (seen & ok).any(), "two impulses reach one output"
        seen |= ok
        y[ok] = h[k[ok]] * h.dtype.type(a)
    return y
