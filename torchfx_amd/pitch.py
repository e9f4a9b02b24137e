"""What pitch a signal has: the YIN fundamental-frequency estimator (de Cheveigne & Kawahara, JASA 2002, steps 2 to 5).

:func:`yin` cuts the last axis into frames and returns one frequency per frame, with the aperiodicity that says whether the frame
is voiced at all.  It is an analysis: it returns tensors, there is no ``FX`` class, nothing in the planner and nothing in the
stream processors; ``Wave.pitch`` calls it on a wave's samples.

The difference function is summed as it is written, ``sum (x[j] - x[j + tau])^2`` in the signal's dtype.  Every term is a square,
so nothing cancels; the autocorrelation form ``E(0) + E(tau) - 2 r(tau)`` loses in float32 exactly the digits the decision is
made on.  On a ROCm device that is one launch of ``torchfx_amd/csrc/yin.hip`` (``torchfx_ext.yin_forward``): a workgroup stages
the span of its frames in LDS once, the partial sums of a block of samples are computed once and shared by the frames that
overlap in it, and the cumulative-mean normalisation, the threshold walk and the parabola run on the chip, so that without
``return_cmndf`` only two numbers per frame are written.  CPU tensors run the same definition over NumPy in the signal's dtype.
There is no other route: a ``frame_length`` above 8192 (float32) or 4096 (float64) is an error on the device.

Not here: pYIN / Viterbi smoothing, median smoothing of the track, NCCF (``detect_pitch_frequency``) semantics, several pitches
at once, a streaming tracker, autograd, axes other than the last.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import Tensor

from torchfx_amd import torchfx_ext as E

__all__ = ["yin"]


def _number(v, name: str, positive: bool = True) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"yin: {name} must be a finite number{' > 0' if positive else ''}, got {v!r}")
    return float(v)


def _count(v, name: str, least: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError(f"yin: {name} must be an integer >= {least}, got {v!r}")
    return int(v)


def _geometry(x, fs, fmin, fmax, frame_length, win_length, hop_length, threshold, center, pad_mode):
    """Every check of :func:`yin`; returns ``(fs, frame_length, W, hop, tau_min, tau_max, threshold, pad)``."""
    if not isinstance(x, Tensor) or x.dtype not in (torch.float32, torch.float64) or x.dim() not in (1, 2, 3) or x.shape[-1] < 1:
        got = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, Tensor) else type(x).__name__
        raise ValueError(f"yin: x must be a float32 / float64 tensor [T], [C, T] or [B, C, T] with T >= 1, got {got}")
    fs, fmin, fmax = _number(fs, "fs"), _number(fmin, "fmin"), _number(fmax, "fmax")
    threshold = _number(threshold, "threshold", positive=False)
    n = _count(frame_length, "frame_length", 2)
    W = n // 2 if win_length is None else _count(win_length, "win_length", 1)
    hop = max(1, n // 4) if hop_length is None else _count(hop_length, "hop_length", 1)
    if W > n:
        raise ValueError(f"yin: win_length {W} must not exceed frame_length {n}")
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"yin: pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    tau_min, tau_max = E.yin_lags(fs, fmin, fmax)
    if tau_min > tau_max:
        raise ValueError(f"yin: fmin {fmin} gives lags up to {tau_max}, below the shortest lag {tau_min} of fmax {fmax}")
    if W + tau_max + 1 > n:
        raise ValueError(f"yin: fmin {fmin} needs lags up to {tau_max + 1}: win_length {W} + {tau_max + 1} exceed frame_length {n}")
    T, pad = int(x.shape[-1]), n // 2 if center else 0
    if pad and pad_mode == "reflect" and pad >= T:
        raise ValueError(f"yin: pad_mode 'reflect' needs more than frame_length // 2 = {pad} samples, got {T}")
    if T + 2 * pad < n:
        raise ValueError(f"yin: frame_length {n} exceeds the {T + 2 * pad} samples of a row (with padding)")
    return fs, n, W, hop, tau_min, tau_max, threshold, pad


def _pick_host(cm: np.ndarray, fs: float, tau_min: int, tau_max: int, threshold: float):
    """Steps 4 and 5 on one frame's ``d'`` in its dtype: ``(f0, aperiodicity)``."""
    R = cm.dtype.type
    under = np.flatnonzero(cm[tau_min:tau_max + 1] < R(threshold))
    if under.size:
        tau = tau_min + int(under[0])
        while tau < tau_max and cm[tau + 1] < cm[tau]:
            tau += 1
    else:
        tau = tau_min + int(np.argmin(cm[tau_min:tau_max + 1]))
    a, b, c = cm[tau - 1], cm[tau], cm[tau + 1]
    den = a - R(2) * b + c
    delta = R(0.5) * (a - c) / den if den > 0 and b <= a and b <= c else R(0)
    return R(fs) / (R(tau) + delta), b


def _yin_host(x: np.ndarray, fs, n, W, hop, tau_min, tau_max, threshold, pad, pad_mode):
    """The definition of :func:`yin` on a host array ``[rows, T]``, in its dtype."""
    R = x.dtype.type
    Lmax = tau_max + 1
    xp = np.pad(x, ((0, 0), (pad, pad)), mode=pad_mode) if pad else x
    frames = 1 + (xp.shape[-1] - n) // hop
    fr = np.lib.stride_tricks.sliding_window_view(xp, W + Lmax, axis=-1)[:, ::hop][:, :frames]          # [rows, frames, W + Lmax]
    head = fr[..., :W]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.stack([np.square(head - fr[..., t:t + W]).sum(axis=-1, dtype=x.dtype) for t in range(Lmax + 1)], axis=-1)
        S = np.cumsum(d[..., 1:], axis=-1, dtype=x.dtype)
        cm = np.ones_like(d)
        lag = np.arange(1, Lmax + 1).astype(x.dtype)
        cm[..., 1:] = np.where(S == 0, R(1), lag * d[..., 1:] / np.where(S == 0, R(1), S))
    f0 = np.empty(d.shape[:-1], dtype=x.dtype)
    ap = np.empty_like(f0)
    bad = ~np.isfinite(fr).all(axis=-1)
    for i in np.ndindex(*f0.shape):
        if bad[i]:
            f0[i] = ap[i] = cm[i] = np.nan
        else:
            f0[i], ap[i] = _pick_host(cm[i], fs, tau_min, tau_max, threshold)
    return f0, ap, cm


@torch.no_grad()
def yin(x: Tensor, fs: float, fmin: float = 65.0, fmax: float = 2093.0, frame_length: int = 2048, win_length: int | None = None,
        hop_length: int | None = None, threshold: float = 0.1, center: bool = True, pad_mode: str = "constant",
        return_aperiodicity: bool = False, return_cmndf: bool = False):
    """The fundamental frequency of ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64) along the last axis by YIN:
    ``f0 [..., frames]`` in Hz, in the signal's dtype.  With ``return_aperiodicity`` also ``[..., frames]``, the normalised
    difference at the chosen lag -- a frame is voiced where it is ``< threshold``; masking is the caller's -- and with
    ``return_cmndf`` also the normalised difference function ``[..., frames, Lmax + 1]`` (a tuple in that order).

    ``win_length`` defaults to ``frame_length // 2`` and ``hop_length`` to ``frame_length // 4``.  The lags searched are
    ``tau_min = max(1, floor(fs / fmax))`` to ``tau_max = ceil(fs / fmin)``, and ``Lmax = tau_max + 1``; ``win_length + Lmax`` must
    fit ``frame_length`` (``ValueError`` naming ``fmin``; nothing is clamped).  ``frames = 1 + (T + 2 pad - frame_length) //
    hop_length`` with ``pad = frame_length // 2`` for ``center=True`` (zeros for ``pad_mode="constant"``, one reflection for
    ``"reflect"``) and 0 without; frame ``f`` starts at ``s = f hop_length - pad`` and reads its first ``W + Lmax`` samples
    (``W = win_length``).  Per frame, in the signal's dtype:

    * ``d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2`` for ``tau = 0 .. Lmax``;
    * ``S(tau) = sum_{k = 1 .. tau} d(k)``, ``d'(0) = 1``, ``d'(tau) = tau d(tau) / S(tau)``, and 1 where ``S(tau) = 0``;
    * ``tau``: the smallest lag in ``[tau_min, tau_max]`` with ``d' < threshold``, advanced while ``tau < tau_max`` and
      ``d'(tau + 1) < d'(tau)``; with none, the first arg-min of ``d'`` over ``[tau_min, tau_max]``;
    * ``a, b, c = d'(tau - 1), d'(tau), d'(tau + 1)``; ``delta = 0.5 (a - c) / (a - 2 b + c)`` when ``a - 2 b + c > 0``,
      ``b <= a`` and ``b <= c``, else 0; ``f0 = fs / (tau + delta)`` and the aperiodicity is ``b``.

    A frame whose ``W + Lmax`` samples (through the reflected edge too) hold a NaN or an Inf is NaN in every output; every other
    frame keeps its bits.  On the device a frame's bits depend on its own samples and on ``(W, hop_length, Lmax, threshold, fs)``
    alone -- not on its index, its row, the batch or its place in a workgroup.

    Device tensors take one launch of ``torchfx_amd/csrc/yin.hip`` (``torchfx_ext.yin_forward``; ``torchfx_ext.yin_plan_info``
    shows its geometry), which serves ``frame_length <= 8192`` (float32) / ``4096`` (float64) and raises ``ValueError`` naming
    ``frame_length`` beyond; CPU tensors run the same definition over NumPy.  ``ValueError`` names a bad argument."""
    fs, n, W, hop, tau_min, tau_max, threshold, pad = _geometry(x, fs, fmin, fmax, frame_length, win_length, hop_length, threshold,
                                                                 center, pad_mode)
    if x.is_cuda:
        cap = 8192 if x.dtype == torch.float32 else 4096
        if n > cap:
            raise ValueError(f"yin: frame_length {n} exceeds {cap}, the longest frame the device kernel serves for {x.dtype}")
        with torch.cuda.device(x.device):
            f0, ap, cm = E.yin_forward(x, fs, n, W, hop, tau_min, tau_max, threshold, pad, pad_mode, return_cmndf)
    else:
        rows = x.detach().reshape(-1, x.shape[-1]).numpy()
        f0, ap, cm = (torch.from_numpy(np.ascontiguousarray(v)) for v in _yin_host(rows, fs, n, W, hop, tau_min, tau_max, threshold, pad,
                                                                                   pad_mode))
        f0, ap = f0.reshape(x.shape[:-1] + f0.shape[-1:]), ap.reshape(x.shape[:-1] + ap.shape[-1:])
        cm = cm.reshape(x.shape[:-1] + cm.shape[-2:])
    out = (f0,) + ((ap,) if return_aperiodicity else ()) + ((cm,) if return_cmndf else ())
    return out[0] if len(out) == 1 else out
