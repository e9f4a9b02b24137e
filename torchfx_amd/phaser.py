"""The phaser: :func:`phase_shift` and the parameters behind :class:`torchfx_amd.effect.Phaser`.

A phaser is a chain of first-order all-pass sections whose one coefficient a low-frequency oscillator (LFO) sweeps every sample;
mixed with the dry signal the moving phase shift cuts moving notches.  The recursion ``x_k[n] = a[n] x_{k-1}[n] + x_{k-1}[n-1] -
a[n] x_k[n-1]`` is an affine map per sample, ``y -> c[n] y + b[n]`` with ``c[n] = -a[n]``, so it is a scan: on ROCm device float32 /
float64 tensors the launches of ``csrc/phaser.hip`` (:func:`torchfx_ext.phaser_forward`), on CPU tensors the same expressions over
NumPy arrays with a blocked scan per stage.  Every intermediate is float64 for both signal dtypes.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.loudness import _check_fs, _check_signal

SHAPES = ("sine", "triangle")
MAX_STAGES = 12
MAX_POSITION = 1 << 52
MIN_FREQ = 10.0                # Hz
MAX_FREQ_OVER_FS = 0.45
_HOST_BLOCK = 1 << 14          # samples the host path scans at a time (bounds its temporaries)


def _real(name: str, v, what: str = "a finite number") -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"phase_shift: {name} must be {what}, got {v!r}")
    return float(v)


class PhaserParams:
    """What a phaser call works with, checked and reduced: ``fs``, ``stages``, ``min_freq``, ``max_freq``, ``rate``, ``phase``,
    ``dry``, ``wet``, ``spread``, ``shape`` as given, and the three numbers the coefficient track is built from, each computed
    once as a float64: ``inc = rate / fs`` (cycles per sample), ``lg = ln(max_freq / min_freq)`` and ``w = pi / fs``."""

    __slots__ = ("fs", "stages", "min_freq", "max_freq", "rate", "phase", "dry", "wet", "spread", "shape", "inc", "lg", "w")

    def __init__(self, fs, dtype: torch.dtype, stages=4, min_freq=200.0, max_freq=2000.0, rate=0.5, phase=0.0, dry=0.5, wet=0.5,
                 spread=0.0, shape="sine") -> None:
        fs = _check_fs(fs)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"phase_shift: float32 or float64 signals only, got {dtype}")
        if shape not in SHAPES:
            raise ValueError(f"phase_shift: shape must be one of {SHAPES}, got {shape!r}")
        if isinstance(stages, bool) or not isinstance(stages, numbers.Integral) or not 1 <= stages <= MAX_STAGES:
            raise ValueError(f"phase_shift: stages must be an integer in [1, {MAX_STAGES}], got {stages!r}")
        lo = _real("min_freq", min_freq, "a finite frequency in Hz")
        hi = _real("max_freq", max_freq, "a finite frequency in Hz")
        if not MIN_FREQ <= lo <= hi <= MAX_FREQ_OVER_FS * fs:
            raise ValueError(f"phase_shift: need {MIN_FREQ:g} Hz <= min_freq <= max_freq <= {MAX_FREQ_OVER_FS} fs = "
                             f"{MAX_FREQ_OVER_FS * fs:g} Hz, got {lo!r} and {hi!r}")
        rate = _real("rate", rate, "a finite rate in Hz")
        if not 0 < rate < fs / 2:
            raise ValueError(f"phase_shift: rate must be in (0, fs / 2) = (0, {fs / 2:g}) Hz, got {rate!r}")
        self.fs, self.stages, self.min_freq, self.max_freq, self.rate = fs, int(stages), lo, hi, rate
        self.phase = _real("phase", phase, "a finite phase in cycles")
        self.dry, self.wet = _real("dry", dry), _real("wet", wet)
        self.spread = _real("spread", spread, "a finite phase in cycles per channel")
        self.shape = shape
        self.inc, self.lg, self.w = rate / fs, math.log(hi / lo), math.pi / fs


def _check_position(position) -> int:
    if isinstance(position, bool) or not isinstance(position, numbers.Integral) or not 0 <= position <= MAX_POSITION:
        raise ValueError(f"phase_shift: position must be an integer in [0, 2^52], got {position!r}")
    return int(position)


def _channels(x: Tensor) -> int:
    return int(x.shape[-2]) if x.dim() >= 2 else 1


def _rows(x: Tensor) -> int:
    return max(1, math.prod(x.shape[:-1]))


def coef_rows(channels: int, spread: float) -> int:
    """Rows of the coefficient track: one per channel index, one in all when the channels share the sweep."""
    return 1 if (spread == 0.0 or channels == 1) else channels


def coefficient_track(n: np.ndarray, P: PhaserParams, c: int = 0) -> np.ndarray:
    """Steps 1 to 5 of :func:`phase_shift` for the absolute samples ``n`` (int64) of channel index ``c``: ``a[n]`` (float64)."""
    z = P.phase + float(c) * P.spread
    off = z - math.floor(z)
    t = n.astype(np.float64) * P.inc
    a_ = (t - np.floor(t)) + off
    if P.shape == "sine":
        l = np.sin(2.0 * np.pi * a_)
    else:
        q = a_ + 0.25
        l = 1.0 - 4.0 * np.abs((q - np.floor(q)) - 0.5)
    fc = P.min_freq * np.exp(P.lg * (0.5 + 0.5 * l))
    g = np.tan(P.w * fc)
    return (g - 1.0) / (g + 1.0)


def _stage_scan(b: np.ndarray, levels: list, cinc: np.ndarray, y0: np.ndarray) -> np.ndarray:
    """``y[n] = c[n] y[n-1] + b[n]`` along the last axis from ``y[-1] = y0``: the maps ``y -> C y + B`` of the single samples
    composed by log-step doubling.  ``levels[i]`` holds the products of ``c`` over the ``2^i`` samples that end at each sample
    and ``cinc`` the products from the block's first sample on; every stage shares them."""
    B = b.copy()
    d = 1
    for cd in levels:
        B[..., d:] = cd[d:] * B[..., :-d] + B[..., d:]
        d *= 2
    return cinc * y0[..., None] + B


def _phase_shift_host(xr: np.ndarray, P: PhaserParams, channels: int, position: int, state: np.ndarray,
                      want_coef: bool) -> tuple[np.ndarray, np.ndarray | None, np.ndarray]:
    """``xr [rows, T]`` (rows are ``[batch, channels]`` flattened), ``state [rows, N + 1]`` -> the float64-computed output in
    ``xr``'s dtype, the coefficient track (or None) and the new state.  A coefficient is computed once per (sample, channel
    index) and applied to every batch item."""
    rows, T = xr.shape
    N = P.stages
    xb = xr.reshape(rows // channels, channels, T)
    st = state.reshape(rows // channels, channels, N + 1).copy()
    y = np.empty_like(xb)
    crow = coef_rows(channels, P.spread)
    coef = np.empty((crow, T), np.float64) if want_coef else None
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for n0 in range(0, T, _HOST_BLOCK):
            n1 = min(T, n0 + _HOST_BLOCK)
            n = position + np.arange(n0, n1, dtype=np.int64)
            shared = None
            for c in range(channels):
                if crow == 1 and shared is not None:
                    a, levels, cinc = shared
                else:
                    a = coefficient_track(n, P, c)
                    cinc, levels, d = -a, [], 1
                    while d < n1 - n0:                               # the products the scan strides need, once for all stages
                        levels.append(cinc)
                        nxt = cinc.copy()
                        nxt[d:] = cinc[d:] * cinc[:-d]
                        cinc, d = nxt, d * 2
                    shared = (a, levels, cinc)
                if coef is not None and c < crow:
                    coef[c, n0:n1] = a
                x0 = xb[:, c, n0:n1].astype(np.float64)
                u = x0
                for k in range(1, N + 1):
                    b = a * u
                    b[:, 1:] += u[:, :-1]
                    b[:, 0] += st[:, c, k - 1]
                    st[:, c, k - 1] = u[:, -1]
                    u = _stage_scan(b, levels, cinc, st[:, c, k])
                st[:, c, N] = u[:, -1]
                y[:, c, n0:n1] = (P.dry * x0 + P.wet * u).astype(xr.dtype)
    return y.reshape(rows, T), coef, st.reshape(rows, N + 1)


def _check_state(state, rows: int, stages: int, device) -> Tensor | None:
    if state is None:
        return None
    if not isinstance(state, Tensor):
        raise TypeError(f"phase_shift: state must be a torch.Tensor, got {type(state).__name__}")
    if tuple(state.shape) != (rows, stages + 1):
        raise ValueError(f"phase_shift: state must have shape [rows, stages + 1] = [{rows}, {stages + 1}], got {list(state.shape)}")
    return state.detach().to(device=device, dtype=torch.float64)


@torch.no_grad()
def phase_shift_run(x: Tensor, P: PhaserParams, position: int = 0, state: Tensor | None = None, want_coef: bool = False,
                    pos: Tensor | None = None, segments: int = 0) -> tuple[Tensor, Tensor | None, Tensor, Tensor | None]:
    """:func:`phase_shift` with the parameters already checked and reduced (the effects' entry): ``(y, coef | None, new state,
    new position | None)``.  ``pos`` is a stream's position as an int64 ``[1]`` tensor on ``x``'s device; it takes the place of
    ``position`` and comes back advanced by ``T`` in a new tensor."""
    _check_signal(x, "phase_shift")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"phase_shift: float32 or float64 signals only, got {x.dtype}")
    position = _check_position(position)
    rows, channels, T = _rows(x), _channels(x), int(x.shape[-1])
    st = _check_state(state, rows, P.stages, x.device)
    if T == 0 or x.numel() == 0:
        st = st.clone() if st is not None else torch.zeros((rows, P.stages + 1), dtype=torch.float64, device=x.device)
        coef = torch.empty((coef_rows(channels, P.spread), T), dtype=torch.float64, device=x.device) if want_coef else None
        return torch.empty_like(x), coef, st, (pos.clone() if pos is not None else None)
    if x.is_cuda:
        from torchfx_amd import torchfx_ext

        with torch.cuda.device(x.device):
            return torchfx_ext.phaser_forward(x, P.stages, P.fs, P.rate, P.min_freq, P.max_freq, P.phase, P.spread, P.dry, P.wet, P.shape,
                                              position, pos, st, want_coef, segments)
    if pos is not None:
        position = _check_position(int(pos))
    a = x.detach().contiguous().numpy()
    y, coef, new = _phase_shift_host(a.reshape(rows, T), P, channels, position,
                                     np.zeros((rows, P.stages + 1)) if st is None else st.numpy(), want_coef)
    return (torch.from_numpy(y.reshape(a.shape)), None if coef is None else torch.from_numpy(coef), torch.from_numpy(new),
            None if pos is None else torch.tensor([position + T], dtype=torch.int64))


@torch.no_grad()
def phase_shift(x: Tensor, fs: int, stages: int = 4, min_freq: float = 200.0, max_freq: float = 2000.0, rate: float = 0.5,
                phase: float = 0.0, dry: float = 0.5, wet: float = 0.5, spread: float = 0.0, shape: str = "sine", position: int = 0,
                state: Tensor | None = None, return_state: bool = False, return_coef: bool = False):
    """Phaser: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64) -> the same shape, dtype and device, computed along
    the last axis; with ``return_coef`` also the coefficient track ``a[n]`` (float64 ``[C, T]``, or ``[1, T]`` when ``spread ==
    0`` or ``C == 1``), with ``return_state`` also the end state (float64 ``[rows, stages + 1]``), in that order.

    The channel index ``c`` of a row is ``row mod C`` (``C = 1`` for ``[T]``).  Every intermediate is float64 for both signal
    dtypes.  The coefficient track, for the absolute sample ``n = position + j``:

    1. ``off = frac(phase + c spread)``
    2. ``t = double(n) (rate / fs)``, one multiplication that is never fused; ``a_ = (t - floor(t)) + off``
    3. ``l = sin(2 pi a_)`` (``shape="sine"``) or ``1 - 4 |frac(a_ + 0.25) - 0.5|`` (``"triangle"``) -- steps 1 to 3 are
       :func:`~torchfx_amd.modulation.modulated_delay`'s
    4. ``fc = min_freq exp(Lg (0.5 + 0.5 l))`` with ``Lg = ln(max_freq / min_freq)``: an exponential sweep (``min_freq ==
       max_freq`` gives a constant filter)
    5. ``g = tan(w fc)`` with ``w = pi / fs``; ``a[n] = (g - 1) / (g + 1)``: ``|a| < 1``, negative while ``fc < fs / 4``

    The filter is ``stages = N`` first-order all-pass sections in series, every one with the same ``a[n]``: ``x_0 = double(x)``,
    ``x_k[n] = a[n] x_{k-1}[n] + x_{k-1}[n-1] - a[n] x_k[n-1]`` for ``k = 1..N``, and ``y[n] = dtype(dry x_0[n] + wet x_N[n])``,
    rounded once.  ``state`` holds ``(x_0[-1], x_1[-1], .., x_N[-1])`` per row; None means silence.

    What follows from it:

    * **Dry path.**  With ``wet = 0`` and ``dry = 1`` a finite input comes back unchanged.
    * **Independence.**  A row's bits depend on its own samples, its channel index and ``position`` alone; equal rows give equal
      rows.  The coefficient track depends on neither the signal nor how the row is cut, bit for bit.
    * **Causality.**  A sample's bits do not depend on values after it.
    * **Chunks.**  Feeding the returned state and ``position + T`` into the next call continues the sweep and the filter: chunks
      equal the one-shot result to float64 round-off (the scan's association follows the cut), not bit for bit.
    * **Non-finite input.**  From a NaN / Inf ``x[m]`` on, every output of its row is non-finite; earlier samples and other rows
      are unaffected.

    Rules: ``1 <= stages <= 12``; ``10 Hz <= min_freq <= max_freq <= 0.45 fs``; ``0 < rate < fs / 2``; ``0 <= position <= 2^52``;
    finite ``dry``, ``wet``, ``phase`` and ``spread``.  ``ValueError`` / ``TypeError`` otherwise.  Feedback (regeneration) around
    the chain, per-stage sweeps, an externally supplied coefficient track, tempo-synced rates, autograd and axes other than the
    last are not provided."""
    _check_signal(x, "phase_shift")
    P = PhaserParams(fs, x.dtype, stages, min_freq, max_freq, rate, phase, dry, wet, spread, shape)
    y, coef, st, _ = phase_shift_run(x, P, position, state, bool(return_coef))
    out = (y,) + ((coef,) if return_coef else ()) + ((st,) if return_state else ())
    return out if len(out) > 1 else y
