"""Noise gate: :func:`gate` and the parameters behind :class:`torchfx_amd.effect.Gate`.

``wave | Gate(-45) | Compressor(-18, 3) | Limiter(-1.0)``: the gate is the first stage of a practical chain.  It takes hum, bleed
and room noise between phrases down before a compressor's make-up gain or ``LoudnessNormalize`` can lift them.  The decision has
hysteresis (it opens at ``threshold_db`` and closes ``hysteresis_db`` below it) and a hold counter; a one-pole smoother with
separate attack and release turns it into a gain between ``range`` and 1.  Both parts look serial and both are scans over small
monoids: a run of samples acts on the decision state through four values (where it ends when entered closed, where it ends when
entered open, how long its leading quiet stretch is, whether it is all quiet), and on the gain as an affine map.  On ROCm device
float32 / float64 tensors the HIP kernels of ``csrc/gate.hip`` cut a row into tiles and segments that run in parallel
(:func:`torchfx_ext.gate_forward`; one launch, or three for long rows of few groups); CPU tensors take the same definition over
NumPy arrays.  The detector runs in float64 for both signal dtypes.
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


class GateParams:
    """What a gate call works with, all linear and float64: ``p_open = 10^(threshold_db / 20)``, ``p_close = 10^((threshold_db -
    hysteresis_db) / 20)``, ``r = 10^(-range_db / 20)`` (exactly 0 for ``range_db = inf``), ``H = floor(hold fs + 0.5)`` samples,
    ``aA`` / ``aR`` (``exp(-1 / (time fs))``, 0 for a time of 0), ``bA = 1 - aA`` and ``bR = (1 - aR) r``."""

    __slots__ = ("p_open", "p_close", "r", "H", "aA", "aR", "bA", "bR")

    def __init__(self, fs, dtype: torch.dtype, threshold_db=-40.0, hysteresis_db=6.0, range_db=math.inf, attack=1e-3, hold=50e-3,
                 release=100e-3) -> None:
        fs = _check_fs(fs)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"gate: float32 or float64 signals only, got {dtype}")
        if isinstance(threshold_db, bool) or not isinstance(threshold_db, numbers.Real) or not math.isfinite(threshold_db):
            raise ValueError(f"gate: threshold_db must be a finite level in dB, got {threshold_db!r}")
        if (isinstance(hysteresis_db, bool) or not isinstance(hysteresis_db, numbers.Real) or not math.isfinite(hysteresis_db)
                or hysteresis_db < 0):
            raise ValueError(f"gate: hysteresis_db must be a finite width >= 0 in dB, got {hysteresis_db!r}")
        if isinstance(range_db, bool) or not isinstance(range_db, numbers.Real) or not range_db >= 0:     # NaN fails the comparison
            raise ValueError(f"gate: range_db must be >= 0 in dB (inf closes the gate fully), got {range_db!r}")
        times = []
        for name, v in (("attack", attack), ("hold", hold), ("release", release)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
                raise ValueError(f"gate: {name} must be a finite time >= 0 in seconds, got {v!r}")
            times.append(float(v))
        self.p_open = 10.0 ** (float(threshold_db) / 20.0)
        self.p_close = 10.0 ** ((float(threshold_db) - float(hysteresis_db)) / 20.0)
        if not (self.p_open > 0.0 and math.isfinite(self.p_open)):
            raise ValueError(f"gate: a threshold of {threshold_db!r} dB is not a positive finite linear level")
        self.r = 0.0 if math.isinf(range_db) else 10.0 ** (-float(range_db) / 20.0)
        H = math.floor(times[1] * fs + 0.5)
        if H >= 2 ** 31:
            raise ValueError(f"gate: a hold of {H} samples exceeds the limit of 2^31 - 1")
        self.H = int(H)
        self.aA = math.exp(-1.0 / (times[0] * fs)) if times[0] > 0 else 0.0
        self.aR = math.exp(-1.0 / (times[2] * fs)) if times[2] > 0 else 0.0
        self.bA = 1.0 - self.aA
        self.bR = (1.0 - self.aR) * self.r

    def key(self) -> tuple:
        return (self.p_open, self.p_close, self.r, self.H, self.aA, self.aR)


def _decision_block(p: np.ndarray, P: GateParams, op: np.ndarray, c: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Step 2 of :func:`gate` on a block ``p [groups, n]`` from the states ``(op, c)`` (int64 each): the open track and the end
    states.  Inside a stretch of samples below ``p_close`` an open gate's counter is the stretch's length so far (plus the
    incoming counter for the stretch the block starts in), so the gate closes where that count reaches ``H + 1``; the track is
    whichever of "opened" (``p >= p_open``) and "closed" came last."""
    n = p.shape[-1]
    idx = np.arange(n, dtype=np.int64)
    loud = p >= P.p_close                                            # NaN: False, as in the per-sample comparisons
    last_loud = np.maximum.accumulate(np.where(loud, idx, -1), axis=-1)
    count = np.where(loud, 0, idx - last_loud + np.where(last_loud < 0, c[:, None], 0))
    last_open = np.maximum.accumulate(np.where(p >= P.p_open, idx, -1), axis=-1)
    last_close = np.maximum.accumulate(np.where(count == P.H + 1, idx, -1), axis=-1)
    track = np.where(last_open == last_close, op[:, None], last_open > last_close).astype(np.int64)
    op_end = track[:, -1]
    return track, op_end, np.where(op_end == 1, count[:, -1], 0)


def _gain_scan(a: np.ndarray, b: np.ndarray, g0: np.ndarray) -> np.ndarray:
    """``g[n] = a[n] g[n-1] + b[n]`` along the last axis from ``g[-1] = g0``: the affine maps of the single samples, composed
    by log-step doubling with the coefficient product carried."""
    A, S = a.copy(), b.copy()
    n, d = a.shape[-1], 1
    while d < n:
        S[..., d:] = A[..., d:] * S[..., :-d] + S[..., d:]
        A[..., d:] = A[..., d:] * A[..., :-d]
        d *= 2
    return A * g0[..., None] + S


def _gate_host(x: Tensor, P: GateParams, groups: int, channels: int, state: np.ndarray) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    a = x.detach().numpy()
    T = a.shape[-1]
    xg = a.reshape(groups, channels, T)
    y = np.empty_like(xg)
    g = np.empty((groups, T), a.dtype)
    o = np.empty((groups, T), np.uint8)
    clean = np.isfinite(state).all(-1)
    gl = np.where(clean, state[:, 0], np.nan)
    op = np.where(clean & (state[:, 1] > 0), 1, 0).astype(np.int64)
    c = np.where(op == 1, np.clip(np.nan_to_num(state[:, 2]), 0, P.H), 0).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for n0 in range(0, T, _HOST_BLOCK):
            blk = xg[..., n0:n0 + _HOST_BLOCK]
            p = np.abs(blk).astype(np.float64).max(1)                                 # np.max propagates NaN
            track, op, c = _decision_block(p, P, op, c)
            bad = ~np.isfinite(p)
            gb = _gain_scan(np.where(track == 1, P.aA, P.aR), np.where(bad, np.nan, np.where(track == 1, P.bA, P.bR)), gl)
            gl = gb[:, -1]
            y[..., n0:n0 + _HOST_BLOCK] = gb[:, None, :] * blk
            g[:, n0:n0 + _HOST_BLOCK] = gb
            o[:, n0:n0 + _HOST_BLOCK] = np.where(np.isnan(gb), 0, track)
    ok = ~np.isnan(gl)
    st = np.stack([gl, np.where(ok, op, np.nan), np.where(ok, c, np.nan)], -1)
    return torch.from_numpy(y.reshape(a.shape)), torch.from_numpy(g), torch.from_numpy(o), torch.from_numpy(st)


def _check_state(state, groups: int, device) -> Tensor | None:
    if state is None:
        return None
    if not isinstance(state, Tensor):
        raise TypeError(f"gate: state must be a torch.Tensor, got {type(state).__name__}")
    if tuple(state.shape) != (groups, 3):
        raise ValueError(f"gate: state must have shape [groups, 3] = [{groups}, 3], got {list(state.shape)}")
    return state.detach().to(device=device, dtype=torch.float64)


def start_state(P: GateParams, groups: int, device) -> Tensor:
    """The state a call without ``state`` starts from: ``(r, closed, 0)`` per group."""
    st = torch.zeros((groups, 3), dtype=torch.float64, device=device)
    st[:, 0] = P.r
    return st


@torch.no_grad()
def gate(x: Tensor, fs: int, threshold_db: float = -40.0, hysteresis_db: float = 6.0, range_db: float = math.inf,
         attack: float = 1e-3, hold: float = 50e-3, release: float = 100e-3, link: bool = True, return_gain: bool = False,
         return_open: bool = False, state: Tensor | None = None, return_state: bool = False, segments: int = 0):
    """Noise gate with hysteresis, hold and range: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64, CPU or device) ->
    the same shape, dtype and device; with ``return_gain`` also the gain curve ``g [groups, T]`` in ``x``'s dtype, with
    ``return_open`` also the decision track ``[groups, T]`` ``torch.uint8``, with ``return_state`` also the end state
    ``[groups, 3]`` float64 ``(g, open, c)`` (``c = 0`` whenever closed), in the order ``y, gain, open, state``.

    A *group* shares one gain curve: with ``link=True`` a ``[C, T]`` signal or each batch item is one group of ``C`` channels,
    with ``link=False`` every row is its own.  The constants are computed once on the host and passed down as linear values:
    ``P_open = 10^(threshold_db / 20)``, ``P_close = 10^((threshold_db - hysteresis_db) / 20)``, ``r = 10^(-range_db / 20)``
    (exactly 0 for ``range_db = inf``), ``H = floor(hold fs + 0.5)`` samples (``0 <= H < 2^31``), ``aA = exp(-1 / (attack fs))``
    (0 for ``attack = 0``) and ``aR`` likewise from ``release``, ``bA = 1 - aA``, ``bR = (1 - aR) r``.  All detector arithmetic
    is float64 for both signal dtypes:

    1. ``p[n] = max_ch |x[ch, n]|``; the max propagates NaN
    2. the state ``(open, c)`` starts from ``state[group]`` or ``(closed, 0)``; per sample: if ``p >= P_open``: ``open = 1,
       c = 0``; else if open and ``p >= P_close``: ``c = 0``; else if open: ``c += 1``, and if ``c > H`` then ``open = 0,
       c = 0``; else it stays closed.  ``open[n]`` is the value after sample ``n``
    3. ``g[n] = aA g[n-1] + bA`` where ``open[n]``, else ``aR g[n-1] + bR``, from ``g[-1] = state[group][0]`` or ``r``
    4. ``y[ch, n] = dtype(g[n] x[ch, n])``
    5. a non-finite ``p[n]`` (NaN or Inf) poisons its group: from that sample to the end of its rows ``y``, ``g`` and the end
       state are NaN and ``open`` is 0; earlier samples and other groups are untouched

    What follows from it:

    * **Hard gate.**  With ``attack = release = 0`` the gain is exactly 1 or ``r``: ``y`` equals ``x`` where open and
      ``dtype(r x)`` where closed, bit for bit.
    * **Transparent.**  A group that is open from its first sample with ``attack = 0`` and never closes comes back bit-identical.
    * **Decision.**  The open track and the ``(open, c)`` of the state are the per-sample loop's bit for bit, on any device,
      under any tiling, segment count or chunking.
    * **Gain.**  Accurate to ``8 * 2^-53 * min(T, 1 / (1 - max(aA, aR)))`` against the exact recursion, not bit for bit: the
      scan's association follows the cut.
    * **Chunks.**  Feeding the returned state into the next call continues both the decision and the gain.

    ``segments`` (device tensors only) forces the cut of a row for the scans; 0 leaves it to the plan.  Finite-ratio downward
    expansion, an envelope or RMS detector, a side-chain key input, look-ahead, autograd and axes other than the last are not
    provided.  An empty ``T`` returns empty tensors and the state unchanged.  ``ValueError`` / ``TypeError`` for a non-finite
    threshold, ``hysteresis_db < 0`` or non-finite, ``range_db < 0`` or NaN, a negative or non-finite time, a hold of ``2^31``
    samples or more, a non-float dtype and a state of the wrong shape."""
    _check_signal(x, "gate")
    P = GateParams(fs, x.dtype, threshold_db, hysteresis_db, range_db, attack, hold, release)
    groups, channels = _grouping(x, bool(link))
    T = int(x.shape[-1])
    st = _check_state(state, groups, x.device)
    if T == 0 or x.numel() == 0:
        y, g = torch.empty_like(x), torch.empty((groups, T), dtype=x.dtype, device=x.device)
        o = torch.empty((groups, T), dtype=torch.uint8, device=x.device)
        st = st.clone() if st is not None else start_state(P, groups, x.device)
    elif x.is_cuda:
        from torchfx_amd import torchfx_ext

        with torch.cuda.device(x.device):
            y, g, o, st = torchfx_ext.gate_forward(x, P.p_open, P.p_close, P.r, P.H, P.aA, P.aR, channels, st, bool(return_gain),
                                                   bool(return_open), int(segments))
    else:
        y, g, o, st = _gate_host(x, P, groups, channels, start_state(P, groups, "cpu").numpy() if st is None else st.numpy())
    out = (y,) + ((g,) if return_gain else ()) + ((o,) if return_open else ()) + ((st,) if return_state else ())
    return out if len(out) > 1 else y
