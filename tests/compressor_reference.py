"""The compressor's definition (torchfx_amd.dynamics.compress, steps 1-4) as a plain float64 loop over the samples: the reference
of the compressor tests.  For short signals only."""
import math

import numpy as np


def alphas(fs, attack, release):
    return tuple(math.exp(-1.0 / (t * fs)) if t > 0 else 0.0 for t in (attack, release))


def curve(p, th, s, W):
    """Step 2 for one level ``p >= 0``."""
    if not math.isfinite(p):
        return math.nan
    o = 20.0 * math.log10(p) - th if p > 0 else -math.inf
    if 2.0 * o <= -W:
        return 0.0
    if 2.0 * o >= W:
        return s * o
    return s * (o + W / 2.0) ** 2 / (2.0 * W)


def nanmax(a, b):
    return math.nan if (math.isnan(a) or math.isnan(b)) else max(a, b)


def detector(v, aA, aR, state=(0.0, 0.0)):
    """Step 3: ``v [T]`` -> ``(y1 [T], yL [T])`` from ``state = (y1[-1], yL[-1])``."""
    y1, yl = float(state[0]), float(state[1])
    o1, ol = np.empty(len(v)), np.empty(len(v))
    for n, vn in enumerate(v):
        y1 = nanmax(vn, aR * y1 + (1.0 - aR) * vn)
        yl = aA * yl + (1.0 - aA) * y1
        o1[n], ol[n] = y1, yl
    return o1, ol


def compress_ref(x, fs, threshold_db=-20.0, ratio=4.0, attack=5e-3, release=100e-3, knee_db=6.0, makeup_db=0.0, link=True,
                 state=None, alphas_=None, trace=None):
    """``x`` a NumPy array ``[T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64) -> ``(y float64 like x, g float64
    [groups, T], end state float64 [groups, 2])``; ``y`` is the unrounded float64 product ``g * x``.  ``alphas_ = (aA, aR)``
    takes the place of the coefficients of ``attack`` and ``release`` (what the low-level op is given); a dict ``trace``
    receives the loop's ``v`` and ``y1`` as ``[groups, T]`` arrays."""
    x = np.asarray(x)
    T = x.shape[-1]
    rows = int(np.prod(x.shape[:-1], dtype=np.int64))
    channels = x.shape[-2] if (link and x.ndim >= 2) else 1
    groups = rows // channels
    xg = x.reshape(groups, channels, T).astype(np.float64)
    s = 1.0 - 1.0 / ratio
    aA, aR = alphas(fs, attack, release) if alphas_ is None else alphas_
    g = np.empty((groups, T))
    tv, t1 = np.empty((groups, T)), np.empty((groups, T))
    end = np.zeros((groups, 2))
    for k in range(groups):
        with np.errstate(invalid="ignore"):
            p = np.abs(xg[k])
            p = np.where(np.isnan(p).any(0), np.nan, p.max(0))
        v = [curve(float(pn), threshold_db, s, knee_db) for pn in p]
        st = (0.0, 0.0) if state is None else state[k]
        y1, yl = detector(v, aA, aR, st)
        g[k] = 10.0 ** ((makeup_db - yl) / 20.0)
        end[k] = (y1[-1], yl[-1]) if T else st
        tv[k], t1[k] = v, y1
    if trace is not None:
        trace["v"], trace["y1"] = tv, t1
    y = (g[:, None, :] * xg).reshape(x.shape)
    return y, g, end


def bursty(rng, shape, quiet=0.01, loud=0.8, burst=400, gap=900, dtype=np.float64):
    """Noise at ``quiet`` with bursts at ``loud``: ``burst`` samples every ``burst + gap``."""
    T = shape[-1]
    x = rng.standard_normal(shape) * quiet
    n = np.arange(T)
    on = (n % (burst + gap)) < burst
    x[..., on] *= loud / quiet
    return np.clip(x, -4.0, 4.0).astype(dtype)
