"""Plain reference for the multi-tap Delay's edge tests (tests/test_gpu_delay_edges.py, tests/test_delay_reference_host.py):
numpy only, float64, no fixtures.  The definition at the top of csrc/delay.hip, with a_1 = 1, a_i = feedback ** (i - 1):

    wet[n] = sum_{i=1..taps} a_i * src[n - i*D]      taps whose position falls outside [0, T) are not added
    dry[n] = x[n] for n < T, else 0
    y[n]   = dry[n] + mix * (wet[n] - dry[n])        n in [0, L),  L = T + taps*D

Mono: src is the row itself.  Ping-pong (consecutive row pairs): the odd taps of row 0 go to row 1, the even taps of row 1 go
to row 0; nothing else is added.
"""
import numpy as np

from tests.fir_reference import gamma  # noqa: F401  (re-exported: gamma(k, u) = k u / (1 - k u))


def amplitudes(taps, feedback):
    """torchfx_ext.delay_amplitudes' formula: 1.0, then feedback ** (i - 1) as Python computes it."""
    return [1.0 if i == 1 else float(feedback ** (i - 1)) for i in range(1, int(taps) + 1)]


def feeds(row, i, pingpong):
    """The output row that tap i of input row `row` is added to, or None."""
    if not pingpong:
        return row
    return row ^ 1 if (i % 2 == 1) == (row % 2 == 0) else None


def wet_dry(x, D, taps, feedback, pingpong):
    """(dry, wet, S) in float64, each [rows, L]: the zero-padded input, the tap sum, and S[n] = |dry[n]| + sum_i |a_i| |src[n - i*D]|,
    the magnitude every rounding of an output is relative to."""
    x = np.asarray(x)
    assert x.ndim == 2 and (not pingpong or x.shape[0] % 2 == 0), x.shape
    rows, T = x.shape
    L = T + taps * D
    x64 = x.astype(np.float64)
    dry = np.zeros((rows, L))
    dry[:, :T] = x64
    wet = np.zeros((rows, L))
    mag = np.zeros((rows, L))
    ax = np.abs(x64)
    for i, a in enumerate(amplitudes(taps, feedback), start=1):
        for r in range(rows):
            dst = feeds(r, i, pingpong)
            if dst is not None:
                wet[dst, i * D:i * D + T] += a * x64[r]
                mag[dst, i * D:i * D + T] += abs(a) * ax[r]
    return dry, wet, np.abs(dry) + mag


def mix_of(dry, wet, mix):
    return dry + mix * (wet - dry)


def delay_ref(x, D, taps, feedback, mix, pingpong):
    """(y, S): the definition in float64 and the magnitude sum of `wet_dry`."""
    dry, wet, S = wet_dry(x, D, taps, feedback, pingpong)
    return mix_of(dry, wet, mix), S


def bound(S, taps, dtype):
    """Per-output tolerance gamma(taps + 6) * S for a kernel that works in `dtype` (u = 2^-24 / 2^-53): `taps` products and
    `taps` additions of the wet sum (each term passes through at most taps + 1 of them, the product's among them: gamma(taps + 1)
    covers products and additions together), the roundings of (T)a_i and of (T)mix, the difference wet - dry, 1 - w, and the
    fused multiply-add of the lerp: five more.  Where S = 0 the output must be exactly 0.  Derived, not measured."""
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return gamma(taps + 6, u) * S


def reach(p, row, T, D, taps, pingpong):
    """{(row, n)}: the outputs a non-finite sample at (row, p) makes non-finite for 0 < mix < 1 and non-zero amplitudes: p itself
    (the dry path) and p + i*D in the row that tap i feeds."""
    assert 0 <= p < T
    out = {(row, p)}
    for i in range(1, taps + 1):
        dst = feeds(row, i, pingpong)
        if dst is not None:
            out.add((dst, p + i * D))
    return out


def reach_mask(bad, rows, T, D, taps, pingpong):
    """[rows, L] bool: the union of `reach` over the (row, p) of `bad`."""
    m = np.zeros((rows, T + taps * D), bool)
    for r, p in bad:
        for rr, n in reach(p, r, T, D, taps, pingpong):
            m[rr, n] = True
    return m
