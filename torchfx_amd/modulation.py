"""The modulated delay line: :func:`modulated_delay` and the parameters behind :class:`torchfx_amd.effect.Chorus`,
:class:`~torchfx_amd.effect.Flanger` and :class:`~torchfx_amd.effect.Vibrato`.

The three effects are one formula, ``y[n] = dry x[n] + sum_v g_v x(n - d_v[n])``: a few *voices* read the signal at a fractional
position that a low-frequency oscillator (LFO) moves.  It is feed-forward, so tiles, batch items and the chunks of a stream are
exact: on ROCm device float32 / float64 tensors one launch of ``csrc/modulation.hip``
(:func:`torchfx_ext.modulated_delay_forward`), on CPU tensors the same expressions over NumPy arrays.  Every intermediate is
float64 for both signal dtypes.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.loudness import _check_fs, _check_signal

SHAPES = ("sine", "triangle")
INTERPOLATIONS = ("linear", "cubic")
MAX_VOICES = 8
MAX_REACH = 1 << 24
MAX_POSITION = 1 << 52
_HOST_BLOCK = 1 << 16          # samples the host path works on at a time (bounds its temporaries)


def _real(name: str, v, what: str = "a finite number") -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"modulated_delay: {name} must be {what}, got {v!r}")
    return float(v)


class ModulationParams:
    """What a modulated-delay call works with: ``table`` (float64 ``[V, 5]`` rows ``(base, depth, inc, phase, gain)``: delay
    and depth in samples, ``inc = rate / fs`` in cycles per sample, phase in cycles), ``dry``, ``spread``, ``shape``,
    ``interpolation`` and ``history`` (``H = max_v floor(base_v + depth_v) + 2``, what a stream carries per row).

    ``voices`` is a sequence of ``(delay, depth, rate, phase, gain)`` rows with delay and depth in samples (need not be
    integers) and rate in Hz."""

    __slots__ = ("table", "dry", "spread", "shape", "interpolation", "history")

    def __init__(self, fs, dtype: torch.dtype, voices, dry=1.0, spread=0.0, shape="sine", interpolation="linear") -> None:
        fs = _check_fs(fs)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"modulated_delay: float32 or float64 signals only, got {dtype}")
        if shape not in SHAPES:
            raise ValueError(f"modulated_delay: shape must be one of {SHAPES}, got {shape!r}")
        if interpolation not in INTERPOLATIONS:
            raise ValueError(f"modulated_delay: interpolation must be one of {INTERPOLATIONS}, got {interpolation!r}")
        try:
            rows = [tuple(v) for v in voices]
        except TypeError:
            raise TypeError(f"modulated_delay: voices must be a sequence of (delay, depth, rate, phase, gain) rows, got {voices!r}") from None
        if not 1 <= len(rows) <= MAX_VOICES:
            raise ValueError(f"modulated_delay: the number of voices must be in [1, {MAX_VOICES}], got {len(rows)}")
        lowest = 1.0 if interpolation == "cubic" else 0.0
        table = np.empty((len(rows), 5), np.float64)
        for i, row in enumerate(rows):
            if len(row) != 5:
                raise ValueError(f"modulated_delay: voice {i} must be (delay, depth, rate, phase, gain), got {row!r}")
            base = _real(f"voice {i}: delay", row[0], "a finite number of samples >= 0")
            depth = _real(f"voice {i}: depth", row[1], "a finite number of samples >= 0")
            rate = _real(f"voice {i}: rate", row[2], "a finite rate in Hz")
            phase = _real(f"voice {i}: phase", row[3], "a finite phase in cycles")
            gain = _real(f"voice {i}: gain", row[4], "a finite gain")
            if base < 0 or depth < 0:
                raise ValueError(f"modulated_delay: voice {i}: delay and depth must be >= 0 samples, got {base!r} and {depth!r}")
            if base - depth < lowest:
                raise ValueError(f"modulated_delay: voice {i}: delay - depth must be >= {lowest:g} sample(s) for {interpolation} "
                                 f"interpolation, got {base!r} - {depth!r}")
            if math.floor(base + depth) + 3 > MAX_REACH:
                raise ValueError(f"modulated_delay: voice {i}: delay + depth must stay below 2^24 - 3 samples, got {base + depth!r}")
            if not 0 < rate < fs / 2:
                raise ValueError(f"modulated_delay: voice {i}: rate must be in (0, fs / 2) = (0, {fs / 2:g}) Hz, got {rate!r}")
            table[i] = (base, depth, rate / fs, phase, gain)
        self.table = table
        self.dry = _real("dry", dry)
        self.spread = _real("spread", spread, "a finite phase in cycles per channel")
        self.shape, self.interpolation = shape, interpolation
        self.history = int(np.floor(table[:, 0] + table[:, 1]).max()) + 2


def _check_position(position) -> int:
    if isinstance(position, bool) or not isinstance(position, numbers.Integral) or not 0 <= position <= MAX_POSITION:
        raise ValueError(f"modulated_delay: position must be an integer in [0, 2^52], got {position!r}")
    return int(position)


def lfo_delay(n: np.ndarray, voice: np.ndarray, off: float, shape: str) -> tuple[np.ndarray, np.ndarray]:
    """Steps 2 to 4 of :func:`modulated_delay` for the absolute samples ``n`` (int64) of one voice and channel offset: the
    delay's whole part ``i`` (int64) and fraction ``f`` (float64)."""
    base, depth, inc = voice[0], voice[1], voice[2]
    t = n.astype(np.float64) * inc
    a = (t - np.floor(t)) + off
    if shape == "sine":
        l = np.sin(2.0 * np.pi * a)
    else:
        z = a + 0.25
        l = 1.0 - 4.0 * np.abs((z - np.floor(z)) - 0.5)
    d = base + depth * l
    i = np.floor(d)
    return i.astype(np.int64), d - i


def _modulate_host(xh: np.ndarray, H: int, P: ModulationParams, channels: int, position: int) -> np.ndarray:
    """``xh [rows, H + T]`` (the ``H`` samples before the call, then the call's) -> float64-computed ``[rows, T]`` in ``xh``'s
    dtype.  Rows are ``[batch, channels]`` flattened; a delay is computed once per (sample, voice, channel index) and applied
    to every batch item."""
    rows, T = xh.shape[0], xh.shape[1] - H
    xb = xh.reshape(rows // channels, channels, H + T)
    y = np.empty((rows // channels, channels, T), xh.dtype)
    cubic = P.interpolation == "cubic"
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(channels):
            xc = xb[:, c, :]
            for n0 in range(0, T, _HOST_BLOCK):
                j = np.arange(n0, min(T, n0 + _HOST_BLOCK), dtype=np.int64)
                acc = P.dry * xc[:, H + j].astype(np.float64)
                for voice in P.table:
                    z = voice[3] + float(c) * P.spread
                    i, f = lfo_delay(position + j, voice, z - math.floor(z), P.shape)
                    m = H + j - i                                    # index of x[n - i] in [history | x]

                    def at(k):
                        ok = (k >= 0) & (k < H + T)
                        return np.where(ok, xc[:, np.clip(k, 0, H + T - 1)].astype(np.float64), 0.0)

                    x0, x1 = at(m), at(m - 1)
                    if cubic:
                        xd = ((-f * (f - 1.0) * (f - 2.0) / 6.0) * at(m + 1) + ((f + 1.0) * (f - 1.0) * (f - 2.0) / 2.0) * x0
                              + (-(f + 1.0) * f * (f - 2.0) / 2.0) * x1 + ((f + 1.0) * f * (f - 1.0) / 6.0) * at(m - 2))
                    else:
                        xd = x0 + f * (x1 - x0)
                    acc = acc + voice[4] * xd
                y[:, c, j] = acc.astype(xh.dtype)
    return y.reshape(rows, T)


def _channels(x: Tensor) -> int:
    return int(x.shape[-2]) if x.dim() >= 2 else 1


def modulate_stream_host(x: Tensor, hist: Tensor | None, P: ModulationParams, position: int) -> tuple[Tensor, Tensor]:
    """One chunk of a stream on the host: ``x`` continues ``hist [rows, H]`` (None = silence) at ``position``.  Returns the
    chunk's output and the new history (the newest ``H`` samples of ``[hist | x]``)."""
    H, T = P.history, int(x.shape[-1])
    rows = max(1, math.prod(x.shape[:-1]))
    h = torch.zeros(rows, H, dtype=x.dtype) if hist is None else hist
    v = torch.cat([h, x.detach().reshape(rows, T)], dim=-1)
    y = _modulate_host(v.numpy(), H, P, _channels(x), position) if T and x.numel() else np.empty((rows, T), v.numpy().dtype)
    return torch.from_numpy(y).reshape(x.shape), v[:, T:].clone()


@torch.no_grad()
def modulated_delay(x: Tensor, fs: int, voices, dry: float = 1.0, spread: float = 0.0, shape: str = "sine",
                    interpolation: str = "linear", position: int = 0) -> Tensor:
    """Modulated delay line: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64) -> the same shape, dtype and device,
    ``y[n] = dry x[n] + sum_v g_v x(n - d_v[n])`` along the last axis.  The delayed tail past the end is dropped.

    ``voices`` holds 1 to 8 rows ``(delay, depth, rate, phase, gain)``: delay and depth in samples (``>= 0``, need not be
    integers), rate in Hz, phase in cycles.  The channel index ``c`` of a row is ``row mod C`` (``C = 1`` for ``[T]``).  For the
    absolute sample ``n = position + j``, voice ``v`` and channel ``c``, every intermediate in float64 for both signal dtypes:

    1. ``off = frac(phase_v + c spread)``
    2. ``t = double(n) (rate_v / fs)``, one multiplication that is never fused; ``a = (t - floor(t)) + off``
    3. ``l = sin(2 pi a)`` (``shape="sine"``) or ``1 - 4 |frac(a + 0.25) - 0.5|`` (``"triangle"``)
    4. ``d = delay_v + depth_v l``, ``i = floor(d)``, ``f = d - i``
    5. ``"linear"``: ``xd = x[n-i] + f (x[n-i-1] - x[n-i])``; ``"cubic"``: the 4-point third-order Lagrange interpolant through
       ``x[n-i+1], x[n-i], x[n-i-1], x[n-i-2]`` at ``f``.  Samples before the first give 0.
    6. ``y[n] = dtype(dry x[n] + sum_v g_v xd_v)``, summed in voice order and rounded once

    What follows from it:

    * **Integer delay.**  Both interpolants return ``x[n-i]`` exactly at ``f = 0``: ``depth = 0`` with an integer delay,
      ``dry = 0`` and ``g = 1`` is the input delayed, bit for bit.
    * **Silent wet part.**  With every ``g_v = 0`` and ``dry = 1`` the result equals ``x``.
    * **Independence.**  A row's bits depend on its own samples, its channel index and ``position`` alone -- not on the
      tiling or the other rows; batch items with equal rows give equal rows.
    * **Chunks.**  A stream that carries the last ``H = max_v floor(delay_v + depth_v) + 2`` samples and the position
      (:class:`torchfx_amd.realtime.StatefulChorus` and its siblings) is bit-identical to the one-shot call.
    * **Non-finite input.**  A NaN / Inf ``x[m]`` reaches no output outside ``[m, m + H]`` of its own row.

    Rules: ``delay_v - depth_v >= 0`` (linear) or ``>= 1`` (cubic, which reads ``x[n-i+1]``); ``floor(delay_v + depth_v) + 3 <=
    2^24``; ``0 < rate_v < fs / 2``; ``0 <= position <= 2^52``.  ``ValueError`` / ``TypeError`` otherwise.  Feedback
    (regeneration), autograd and axes other than the last are not provided."""
    _check_signal(x, "modulated_delay")
    return modulate(x, ModulationParams(fs, x.dtype, voices, dry, spread, shape, interpolation), position)


@torch.no_grad()
def modulate(x: Tensor, P: ModulationParams, position: int = 0) -> Tensor:
    """:func:`modulated_delay` with the parameters already checked and reduced (the effects' entry)."""
    _check_signal(x, "modulated_delay")
    position = _check_position(position)
    if x.shape[-1] == 0 or x.numel() == 0:
        return torch.empty_like(x)
    if x.is_cuda:
        from torchfx_amd import torchfx_ext

        with torch.cuda.device(x.device):
            return torchfx_ext.modulated_delay_forward(x, P.table, P.spread, P.dry, P.shape, P.interpolation, position)
    a = x.detach().contiguous().numpy()
    rows = max(1, math.prod(x.shape[:-1]))
    return torch.from_numpy(_modulate_host(a.reshape(rows, -1), 0, P, _channels(x), position).reshape(a.shape))
