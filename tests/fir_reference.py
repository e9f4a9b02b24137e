"""Plain references for the direct FIR tests (tests/test_gpu_fir_edges.py, tests/test_fir_reference_host.py): numpy only,
no fixtures.  Convention of `fir_direct_forward`: `kf` are the FLIPPED taps,

    y[c, n] = sum_{t < K} kf[t] * xp[c, n + t],      xp = [K-1 samples of history (zeros without one) | x]
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def _padded(x, K, hist, dtype):
    x = np.asarray(x)
    C, T = x.shape
    xp = np.zeros((C, T + K - 1), dtype)
    xp[:, K - 1:] = x
    if hist is not None and K > 1:
        hist = np.asarray(hist)
        assert hist.shape == (C, K - 1), hist.shape
        xp[:, :K - 1] = hist
    return xp


def _direct(xp, kf, T):
    """sum_t kf[t] * xp[:, n + t] in xp's dtype: every tap is multiplied with every sample it meets, one tap at a time in tap
    order, so NaN and Inf travel by numpy's own IEEE arithmetic.  Rows are independent: they are spread over a few threads."""
    C = xp.shape[0]
    y = np.zeros((C, T), xp.dtype)

    def rows(sl):
        acc, tmp = y[sl], np.empty_like(y[sl])
        with np.errstate(all="ignore"):                 # (per thread)
            for t in range(len(kf)):
                np.multiply(xp[sl, t:t + T], kf[t], out=tmp)
                acc += tmp

    if C == 1 or C * T * len(kf) < (1 << 22):
        rows(slice(0, C))
    else:
        n = min(8, C)
        with ThreadPoolExecutor(n) as pool:
            list(pool.map(rows, [slice(i * C // n, (i + 1) * C // n) for i in range(n)]))
    return y


def ref64(x, kf, hist=None, wide=False):
    """The direct form in float64 (`wide`: in numpy's long double, for judging float64 kernels: 64 mantissa bits on x86).
    All K taps are always multiplied, zero-valued ones included.  Returns [C, T] in the accumulation dtype."""
    dt = np.longdouble if wide else np.float64
    kf = np.asarray(kf).reshape(-1).astype(dt)
    return _direct(_padded(x, len(kf), hist, dt), kf, np.asarray(x).shape[1])


def gamma(n, u):
    return n * u / (1.0 - n * u)


def bound(x, kf, hist=None):
    """Per-output tolerance for a kernel that forms the K products and their sum in the dtype of `x`, in any order, fused
    or not: gamma(K+1) * (|kf| (*) |x|)[n] + K * tiny, gamma(N) = N u / (1 - N u) (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., section 3.1 and 4.2).  u = 2^-24, tiny = 2^-126 for float32; 2^-53, 2^-1022 for float64.
    The floor of K * tiny leaves subnormal handling out of the assertion.  Derived, not measured."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    u, tiny = (2.0 ** -24, 2.0 ** -126) if x.dtype == np.float32 else (2.0 ** -53, 2.0 ** -1022)
    kf = np.asarray(kf).reshape(-1)
    K = len(kf)
    s = ref64(np.abs(x), np.abs(kf.astype(np.float64)), None if hist is None else np.abs(np.asarray(hist)))
    return gamma(K + 1, u) * s + K * tiny


def reach_mask(C, T, K, bad):
    """[C, T] bool: true on [p, p + K) within [0, T) for every (row, p) of `bad` -- the outputs a causal K-tap filter lets the
    sample at p reach.  p < 0 is a position in the history."""
    m = np.zeros((C, T), bool)
    for row, p in bad:
        lo, hi = max(p, 0), min(p + K, T)
        if lo < hi:
            m[row, lo:hi] = True
    return m


STAIR = (1.0, 2.0 ** -10, 2.0 ** -20, 2.0 ** -30, 2.0 ** -20, 2.0 ** -10)


def staircase(C, T, seed, edges, dtype=np.float32):
    """Gaussian noise whose amplitude steps through 1, 2^-10, 2^-20, 2^-30 and back up (and round again), one step at every
    sample index in `edges`."""
    x = np.random.default_rng(seed).standard_normal((C, T))
    amp = np.empty(T)
    cuts = [0] + sorted(e for e in set(edges) if 0 < e < T) + [T]
    for i in range(len(cuts) - 1):
        amp[cuts[i]:cuts[i + 1]] = STAIR[i % len(STAIR)]
    return (x * amp).astype(dtype)
