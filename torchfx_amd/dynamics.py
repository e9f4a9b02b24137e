"""Feed-forward compressor: :func:`compress` and the parameters behind :class:`torchfx_amd.effect.Compressor`.

``wave | LoudnessNormalize(-14) | Compressor(-18, 3) | Limiter(-1.0)`` is the mastering chain: the compressor narrows the
dynamic range, the limiter then takes down what peaks are left.  The gain computer works in the log domain (threshold, ratio,
soft knee) and the level detector is the *smooth decoupled* peak detector of Giannoulis, Massberg & Reiss, "Digital Dynamic
Range Compressor Design -- A Tutorial and Analysis" (JAES 60(6), 2012): a release stage with a ``max`` in it followed by a
one-pole attack stage.  Both stages are scans over a monoid -- ``y -> max(M, a^k y + B)`` and ``y -> a^k y + S`` are closed under
composition -- so a row is cut into tiles and segments that run in parallel: on ROCm device float32 / float64 tensors the HIP
kernels of ``csrc/compressor.hip`` (:func:`torchfx_ext.compressor_forward`; one launch, or three for long rows of few
groups), on CPU tensors the same scan over NumPy arrays.  The detector runs in float64 for both signal dtypes.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.limiter import _grouping
from torchfx_amd.loudness import _check_fs, _check_signal

_HOST_BLOCK = 1 << 16          # samples the host path scans at a time (the state carries over; bounds its temporaries)


def _level(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"compress: {name} must be a finite level in dB, got {v!r}")
    return float(v)


class CompressorParams:
    """What a compressor call works with: ``th`` (threshold, dB), ``s = 1 - 1 / ratio``, ``w`` (knee width, dB), ``alpha_a`` /
    ``alpha_r`` (``exp(-1 / (time fs))``, 0 for a time of 0) and ``makeup`` (dB), all float64."""

    __slots__ = ("th", "s", "w", "alpha_a", "alpha_r", "makeup")

    def __init__(self, fs, dtype: torch.dtype, threshold_db=-20.0, ratio=4.0, attack=5e-3, release=100e-3, knee_db=6.0,
                 makeup_db=0.0) -> None:
        fs = _check_fs(fs)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"compress: float32 or float64 signals only, got {dtype}")
        self.th = _level("threshold_db", threshold_db)
        self.makeup = _level("makeup_db", makeup_db)
        if isinstance(ratio, bool) or not isinstance(ratio, numbers.Real) or not ratio >= 1:      # NaN fails the comparison
            raise ValueError(f"compress: ratio must be >= 1 (inf for a limiter's slope), got {ratio!r}")
        self.s = 1.0 - 1.0 / float(ratio)
        if isinstance(knee_db, bool) or not isinstance(knee_db, numbers.Real) or not math.isfinite(knee_db) or knee_db < 0:
            raise ValueError(f"compress: knee_db must be a finite width >= 0 in dB, got {knee_db!r}")
        self.w = float(knee_db)
        alphas = []
        for name, v in (("attack", attack), ("release", release)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
                raise ValueError(f"compress: {name} must be a finite time >= 0 in seconds, got {v!r}")
            alphas.append(math.exp(-1.0 / (float(v) * fs)) if v > 0 else 0.0)
        self.alpha_a, self.alpha_r = alphas

    def key(self) -> tuple:
        return (self.th, self.s, self.w, self.alpha_a, self.alpha_r, self.makeup)


def gain_reduction_db(p: np.ndarray, P: CompressorParams) -> np.ndarray:
    """Step 2 of :func:`compress`: the static curve's gain reduction ``v >= 0`` in dB for linear levels ``p >= 0`` (float64)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        o = 20.0 * np.log10(p) - P.th
        v = np.where(2.0 * o >= P.w, P.s * o, 0.0)
        if P.w > 0:
            v = np.where(np.abs(2.0 * o) < P.w, P.s * (o + 0.5 * P.w) ** 2 / (2.0 * P.w), v)
    return np.where(np.isfinite(p), v, np.nan)


def _release_scan(v: np.ndarray, a: float, y0: np.ndarray) -> np.ndarray:
    """``y1[n] = max(v[n], a y1[n-1] + (1 - a) v[n])`` along the last axis from ``y1[-1] = y0``: the maps
    ``y -> max(M, a^k y + B)`` of the single samples, composed by log-step doubling."""
    M, B = v.copy(), (1.0 - a) * v
    n, d = v.shape[-1], 1
    while d < n:
        ad = a ** d
        Mn = np.maximum(M[..., d:], ad * M[..., :-d] + B[..., d:])
        B[..., d:] = ad * B[..., :-d] + B[..., d:]
        M[..., d:] = Mn
        d *= 2
    return np.maximum(M, a ** np.arange(1.0, n + 1.0) * y0[..., None] + B)


def _attack_scan(u: np.ndarray, a: float, y0: np.ndarray) -> np.ndarray:
    """``yL[n] = a yL[n-1] + (1 - a) u[n]`` along the last axis from ``yL[-1] = y0``, by the same doubling."""
    S = (1.0 - a) * u
    n, d = u.shape[-1], 1
    while d < n:
        S[..., d:] = a ** d * S[..., :-d] + S[..., d:]
        d *= 2
    return a ** np.arange(1.0, n + 1.0) * y0[..., None] + S


def _compress_host(x: Tensor, P: CompressorParams, groups: int, channels: int, state: np.ndarray) -> tuple[Tensor, Tensor, Tensor]:
    a = x.detach().numpy()
    T = a.shape[-1]
    xg = a.reshape(groups, channels, T)
    y = np.empty_like(xg)
    g = np.empty((groups, T), a.dtype)
    y1, yl = state[:, 0].copy(), state[:, 1].copy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for n0 in range(0, T, _HOST_BLOCK):
            blk = xg[..., n0:n0 + _HOST_BLOCK]
            v = gain_reduction_db(np.abs(blk).astype(np.float64).max(1), P)           # np.max propagates NaN
            r = _release_scan(v, P.alpha_r, y1)
            l = _attack_scan(r, P.alpha_a, yl)
            y1, yl = r[:, -1], l[:, -1]
            gb = 10.0 ** ((P.makeup - l) / 20.0)
            y[..., n0:n0 + _HOST_BLOCK] = gb[:, None, :] * blk
            g[:, n0:n0 + _HOST_BLOCK] = gb
    return (torch.from_numpy(y.reshape(a.shape)), torch.from_numpy(g), torch.from_numpy(np.stack([y1, yl], -1)))


def _check_state(state, groups: int, device) -> Tensor | None:
    if state is None:
        return None
    if not isinstance(state, Tensor):
        raise TypeError(f"compress: state must be a torch.Tensor, got {type(state).__name__}")
    if tuple(state.shape) != (groups, 2):
        raise ValueError(f"compress: state must have shape [groups, 2] = [{groups}, 2], got {list(state.shape)}")
    return state.detach().to(device=device, dtype=torch.float64)


@torch.no_grad()
def compress(x: Tensor, fs: int, threshold_db: float = -20.0, ratio: float = 4.0, attack: float = 5e-3, release: float = 100e-3,
             knee_db: float = 6.0, makeup_db: float = 0.0, link: bool = True, return_gain: bool = False, state: Tensor | None = None,
             return_state: bool = False):
    """Feed-forward compressor: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64) -> the same shape, dtype and device;
    with ``return_gain`` also the gain curve ``g [groups, T]`` in ``x``'s dtype, with ``return_state`` also the detector's end
    state ``[groups, 2]`` float64, in that order.

    A *group* shares one gain curve: with ``link=True`` a ``[C, T]`` signal or each batch item is one group of ``C`` channels,
    with ``link=False`` every row is its own.  With ``s = 1 - 1 / ratio`` (``ratio >= 1``, ``inf`` allowed), ``W = knee_db``,
    ``Th = threshold_db``, ``aA = exp(-1 / (attack fs))`` (0 for ``attack = 0``) and ``aR`` likewise from ``release``, all
    detector arithmetic in float64 for both signal dtypes:

    1. ``p[n] = max_ch |x[ch, n]|``
    2. the wanted gain reduction in dB, with ``o = 20 log10(p[n]) - Th`` (``p = 0``: ``-inf``): ``v[n] = 0`` where
       ``2 o <= -W``, ``s o`` where ``2 o >= W``, else ``s (o + W / 2)^2 / (2 W)``; a non-finite ``p[n]`` gives NaN
    3. ``y1[n] = max(v[n], aR y1[n-1] + (1 - aR) v[n])``, ``yL[n] = aA yL[n-1] + (1 - aA) y1[n]``, from
       ``(y1[-1], yL[-1]) = state[group]`` (silence without a state); ``max`` propagates NaN
    4. ``g[n] = 10^((makeup_db - yL[n]) / 20)``, ``y[ch, n] = dtype(g[n] x[ch, n])``

    What follows from it:

    * **Transparent.**  With ``makeup_db = 0`` and no state a group whose level never passes ``Th - W / 2`` comes back
      bit-identical: ``v = 0`` gives ``yL = 0`` exactly, however the row is cut.
    * **Static curve.**  A constant level ``L`` above the knee settles to the output level ``Th + (L - Th) / ratio``.
    * **Attack.**  After a step of ``v`` from 0 to ``v0``, ``yL[n] = v0 (1 - aA^(n+1))``.
    * **Release.**  After ``v`` drops to 0, ``y1`` decays as ``aR^n``.
    * **Hold.**  A release so long that ``aR`` rounds to 1 (``release = 1e300``) holds the peak: ``y1`` is the running maximum
      of ``v``, without any rounding.
    * **Chunks.**  Feeding the returned state into the next call continues the curve: chunks equal the one-shot result to
      float64 round-off of the detector (the scan's association follows the cut), not bit for bit.
    * **Non-finite input.**  From the first NaN / Inf sample of a group to the end of its rows every output, the gain and the
      end state of that group are NaN; earlier samples and other groups are unaffected.

    RMS, feedback and branching detectors, a side-chain input, automatic make-up gain, look-ahead, downward expansion (gating
    is :func:`torchfx_amd.gate.gate`), autograd and axes other than the last are not provided.  An empty ``T`` returns an empty tensor and the state unchanged.
    ``ValueError`` / ``TypeError`` for ``ratio < 1`` or NaN, a negative or non-finite time, ``knee_db < 0``, a non-finite level,
    a non-float dtype and a state of the wrong shape."""
    _check_signal(x, "compress")
    P = CompressorParams(fs, x.dtype, threshold_db, ratio, attack, release, knee_db, makeup_db)
    groups, channels = _grouping(x, bool(link))
    T = int(x.shape[-1])
    st = _check_state(state, groups, x.device)
    if T == 0 or x.numel() == 0:
        y, g = torch.empty_like(x), torch.empty((groups, T), dtype=x.dtype, device=x.device)
        st = st.clone() if st is not None else torch.zeros((groups, 2), dtype=torch.float64, device=x.device)
    elif x.is_cuda:
        from torchfx_amd import torchfx_ext

        with torch.cuda.device(x.device):
            y, g, st = torchfx_ext.compressor_forward(x, P.th, P.s, P.w, P.alpha_a, P.alpha_r, P.makeup, channels, st,
                                                      bool(return_gain))
    else:
        y, g, st = _compress_host(x, P, groups, channels, np.zeros((groups, 2)) if st is None else st.numpy())
    out = (y,) + ((g,) if return_gain else ()) + ((st,) if return_state else ())
    return out if len(out) > 1 else y
