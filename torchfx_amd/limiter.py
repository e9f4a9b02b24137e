"""Look-ahead true-peak limiter: :func:`limit` and the parameters behind :class:`torchfx_amd.effect.Limiter`.

``wave | LoudnessNormalize(-14) | Limiter(-1.0)`` is the mastering one-liner: where ``LoudnessNormalize(max_true_peak=...)``
can only lower the whole programme's gain, the limiter takes down the peaks alone.  Gain reduction is a windowed minimum
followed by a short FIR -- no recursion -- so every output depends on a bounded window of inputs.  On ROCm device float32 /
float64 tensors ONE HIP launch (``csrc/limiter.hip``, :func:`torchfx_ext.limiter_forward`) reads the signal once and writes
it once: the detector's oversampled signal, the gain curve and its intermediates never leave the chip.  CPU tensors run
NumPy / SciPy with the same definition in the signal's dtype.  For a chunked stream the bounded window is what makes
:class:`torchfx_amd.realtime.StatefulLimiter` possible: it carries a fixed input history per row and its chunks plus ``flush()``
are this function's result on the whole signal, bit for bit.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.loudness import OVERSAMPLE_FACTORS, _check_fs, _check_signal, _interpolator, default_oversample

MAX_LOOKAHEAD = 512            # samples: the native kernel's limits (tfx_limiter_forward)
MAX_HOLD = 4096
DETECTORS = ("true_peak", "sample")


def default_window(A: int) -> np.ndarray:
    """The default smoothing weights ``sin^2(pi (j + 1) / (A + 1))``, ``j < A``, in float64 (not normalised)."""
    return np.sin(np.pi * (np.arange(A, dtype=np.float64) + 1.0) / (A + 1.0)) ** 2


class LimiterParams:
    """What a limiter call works with, in samples and in the signal's dtype: ``c`` (linear ceiling), ``A`` (look-ahead), ``H``
    (hold), ``up`` (detector oversampling), ``taps`` (host tensor or None for ``up == 1``) and ``w`` (``[A]`` weights, sum 1)."""

    __slots__ = ("c", "A", "H", "up", "taps", "w")

    def __init__(self, fs, dtype: torch.dtype, ceiling_db=-1.0, lookahead=1.5e-3, hold=10e-3, detector="true_peak",
                 oversample=None, taps=None, window=None) -> None:
        fs = _check_fs(fs)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"limit: float32 or float64 signals only, got {dtype}")
        np_dtype = np.float64 if dtype == torch.float64 else np.float32
        if isinstance(ceiling_db, bool) or not isinstance(ceiling_db, numbers.Real) or not math.isfinite(ceiling_db):
            raise ValueError(f"limit: ceiling_db must be a finite level in dB, got {ceiling_db!r}")
        for name, v in (("lookahead", lookahead), ("hold", hold)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
                raise ValueError(f"limit: {name} must be a finite time >= 0 in seconds, got {v!r}")
        if detector not in DETECTORS:
            raise ValueError(f"limit: detector must be one of {DETECTORS}, got {detector!r}")
        self.c = float(np_dtype(10.0 ** (float(ceiling_db) / 20.0)))
        if not (self.c > 0.0 and math.isfinite(self.c)):
            raise ValueError(f"limit: a ceiling of {ceiling_db!r} dB is not a positive finite {np_dtype.__name__} value")
        self.A = max(1, int(round(float(lookahead) * fs)))
        self.H = max(1, int(round(float(hold) * fs)))
        if self.A > MAX_LOOKAHEAD:
            raise ValueError(f"limit: a look-ahead of {self.A} samples exceeds the limit of {MAX_LOOKAHEAD}")
        if self.H > MAX_HOLD:
            raise ValueError(f"limit: a hold of {self.H} samples exceeds the limit of {MAX_HOLD}")
        if oversample is None:
            oversample = default_oversample(fs) if detector == "true_peak" else 1
        if isinstance(oversample, bool) or oversample not in OVERSAMPLE_FACTORS:
            raise ValueError(f"limit: oversample must be one of {OVERSAMPLE_FACTORS}, got {oversample!r}")
        self.up = int(oversample)
        self.taps = None
        if self.up > 1:
            self.taps = _interpolator(taps, self.up, dtype)
            if self.taps is None:
                from torchfx_amd.resample import design_taps

                self.taps = design_taps(self.up, 1, ("kaiser", 5.0), dtype)
        if window is None:
            w = default_window(self.A)
        else:
            w = window.detach().cpu().numpy() if isinstance(window, Tensor) else np.asarray(window)
            w = np.array(w, dtype=np.float64)
            if w.ndim != 1 or w.size != self.A:
                raise ValueError(f"limit: window must hold A = {self.A} weights (lookahead * fs), got shape {w.shape}")
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("limit: window weights must be finite and >= 0")
            if not w.sum() > 0:
                raise ValueError("limit: window weights sum to 0")
        self.w = np.ascontiguousarray((w / w.sum()).astype(np_dtype))

    def key(self) -> tuple:
        return (self.c, self.A, self.H, self.up, None if self.taps is None else self.taps.numpy().tobytes(), self.w.tobytes())


def _grouping(x: Tensor, link: bool) -> tuple[int, int]:
    """(groups, channels per group) of ``x [T]``, ``[C, T]`` or ``[B, C, T]``."""
    rows = 1
    for n in x.shape[:-1]:
        rows *= int(n)
    channels = int(x.shape[-2]) if (link and x.dim() >= 2) else 1
    return (rows // channels if channels else 0), channels


def sliding_min(rp: np.ndarray, W: int) -> np.ndarray:
    """``min(rp[..., a : a + W])`` for every ``a`` (last axis shrinks by ``W - 1``): exact, by doubling; NaN propagates."""
    cur, w = rp, 1
    while 2 * w <= W:
        cur = np.minimum(cur[..., :-w], cur[..., w:])
        w *= 2
    n = rp.shape[-1] - W + 1
    return np.minimum(cur[..., :n], cur[..., W - w:W - w + n])


def _limit_host(x: Tensor, P: LimiterParams, groups: int, channels: int) -> tuple[Tensor, Tensor]:
    a = x.detach().numpy()
    dt = a.dtype.type
    T = a.shape[-1]
    xg = a.reshape(groups, channels, T)
    p = np.abs(xg)
    if P.up > 1:
        from torchfx_amd.resample import resample_poly

        v = resample_poly(torch.from_numpy(np.ascontiguousarray(xg)), P.up, 1, window=(P.taps / P.up).numpy()).numpy()
        q = np.abs(v).reshape(groups, channels, T, P.up).max(-1)              # np.max propagates NaN
        qs = np.concatenate([np.zeros_like(q[..., :1]), q[..., :-1]], -1)
        p = np.maximum(np.maximum(p, q), qs)
    p = p.max(1)                                                              # [groups, T]
    c = dt(P.c)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(p > c, c / p, np.where(np.isnan(p), dt(np.nan), dt(1)))
    A, H = P.A, P.H
    # m[k] for k in [-(A-1), T): r padded with ones, H-1 + A-1 in front and A-1 behind
    rp = np.concatenate([np.ones((groups, H + A - 2), dt), r, np.ones((groups, A - 1), dt)], -1)
    d = dt(1) - sliding_min(rp, A + H - 1)                                    # d[., k + A - 1] = 1 - m[k]
    acc = np.zeros((groups, T), dt)
    for j in range(A - 1, -1, -1):
        acc = P.w[j] * d[:, A - 1 - j:A - 1 - j + T] + acc
    g = np.minimum(np.maximum(dt(1) - acc, dt(0)), r)
    g = np.where(np.isnan(r) | np.isnan(acc), dt(np.nan), g)
    y = (g[:, None, :] * xg).reshape(a.shape)
    return torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(np.ascontiguousarray(g))


@torch.no_grad()
def limit(x: Tensor, fs: int, ceiling_db: float = -1.0, lookahead: float = 1.5e-3, hold: float = 10e-3,
          detector: str = "true_peak", link: bool = True, oversample: int | None = None, taps=None, window=None,
          return_gain: bool = False):
    """Look-ahead limiter: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64) -> the same shape, dtype and device;
    with ``return_gain`` also the gain curve ``g [groups, T]`` (the gain-reduction meter).

    A *group* shares one gain curve: with ``link=True`` a ``[C, T]`` signal or each batch item is one group of ``C``
    channels, with ``link=False`` every row is its own.  In the signal's dtype, with ``c = 10^(ceiling_db / 20)``,
    ``A = max(1, round(lookahead * fs))``, ``H = max(1, round(hold * fs))`` (at most 512 and 4096 samples), ``up`` the
    detector's oversampling (``detector="true_peak"``: :func:`torchfx_amd.loudness.default_oversample`, ``"sample"``: 1, or
    ``oversample``) and ``w`` the ``A`` smoothing weights (default ``sin^2(pi (j + 1) / (A + 1))``, or ``window``; normalised
    to sum 1 in float64, then rounded):

    1. ``q[ch, i] = max_ph |v[ch, i up + ph]|``, ``v = resample_poly(x[ch], up, 1)`` with the library's interpolator or
       ``taps`` (as :func:`torchfx_amd.loudness.true_peak`); ``q[ch, -1] = 0``
    2. ``p[i] = max_ch max(|x[ch, i]|, q[ch, i], q[ch, i - 1])`` -- with ``up = 1`` there is nothing between the samples and
       ``p[i] = max_ch |x[ch, i]|``
    3. ``r[i] = c / p[i]`` where ``p[i] > c``, else 1; 1 outside ``[0, T)``
    4. ``m[k] = min r[k - H + 1 ... k + A - 1]``
    5. ``s[n]``: ``acc = 0``, then ``acc = fma(w[j], 1 - m[n - j], acc)`` for ``j = A - 1`` down to 0
    6. ``g[n] = min(max(1 - s[n], 0), r[n])``
    7. ``y[ch, n] = g[n] x[ch, n]``

    What follows from it:

    * **Transparent.**  A group whose ``p`` never passes ``c`` comes back bit-identical (the FIR smooths the reduction
      ``1 - m``, which is then exactly 0).
    * **Sample ceiling.**  ``|y| <= c (1 + u)^2``, ``u`` = 2^-24 / 2^-53: ``g <= r``, ``p >= |x|``, one rounded division and
      one rounded product.
    * **Time course.**  A lone sample peak at ``n0`` (``detector="sample"``) starts the gain falling at ``n0 - A + 1``; the gain
      is ``r[n0]`` (to the rounding of the ``A``-term sum; at ``n0`` itself never above it) from ``n0`` through ``n0 + H - 1``
      and is back at exactly 1 from ``n0 + H + A - 1`` on.
    * **True peak: measured, not guaranteed.**  A gain curve does not commute with the interpolator, so the true peak of the
      result is not bounded by a theorem.  It stays within a margin that shrinks as ``A`` grows: at 48 kHz and a -1 dBTP
      ceiling a float64 prototype read +0.000 dB over the ceiling for tones and integrated noise and +0.00015 dB for stereo
      uniform noise 8 dB over it at ``A, H = 72, 480``; +0.0065 dB at 24 / 24; +0.27 dB at 8 / 2.  Do not rely on a hard
      true-peak ceiling with a short look-ahead.

    On the device the work is cut into tiles fixed by ``(T, A, H, up, taps, dtype)``: a tile whose input window holds a NaN or an
    Inf in any channel of the group gives NaN on all its outputs in every channel of that group; other tiles and groups are
    unaffected, and a group's bits do not depend on the batch.  An empty ``T`` returns an empty tensor.  ``ValueError`` /
    ``TypeError`` for a non-finite ``ceiling_db``, a negative time, a look-ahead or hold beyond the limits, a ``window`` of the
    wrong length, with a negative or non-finite weight or summing to 0, and a non-float dtype."""
    _check_signal(x, "limit")
    P = LimiterParams(fs, x.dtype, ceiling_db, lookahead, hold, detector, oversample, taps, window)
    groups, channels = _grouping(x, bool(link))
    T = int(x.shape[-1])
    if T == 0 or x.numel() == 0:
        y, g = torch.empty_like(x), torch.empty((groups, T), dtype=x.dtype, device=x.device)
    elif x.is_cuda:
        from torchfx_amd import torchfx_ext

        with torch.cuda.device(x.device):
            y, g = torchfx_ext.limiter_forward(x, P.c, P.A, P.H, torch.from_numpy(P.w), P.up, P.taps, channels, bool(return_gain))
    else:
        y, g = _limit_host(x, P, groups, channels)
    return (y, g) if return_gain else y
