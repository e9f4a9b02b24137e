"""Chunked (streaming) execution with carried state -- SURVEY.md 8(f) rank 1.

Reference: ``StreamProcessor`` (``src/torchfx/realtime/stream.py:164-347``) reads a file in
chunks of ``chunk_size`` frames with ``overlap``, runs every effect's ``forward`` per chunk and
relies on the IIR modules' carried DF1 state for continuity; FIR modules are stateless there, so
seams are only right with ``overlap >= K-1``.  This mirror keeps the same chunk / overlap arithmetic
on tensors (``process_chunks`` / ``process_tensor``) and on files (``process_file`` /
``process_file_chunks``: ``soundfile`` stays the codec, as in the reference, but each decoded chunk
goes to the device interleaved -- pinned staging, de-interleave kernel, ``torchfx_amd.io`` -- and comes
back interleaved, so the host never transposes), plus what the reference lacks: :class:`StatefulFIR`,
an FIR that carries its last K-1 input samples so that ``overlap = 0`` streaming is exact for FIR
stages too; its kernels read the history and the chunk from two buffers (``tfx_fir_stream_forward``),
there is no concatenated copy of the chunk.  :class:`StatefulDelay` and :class:`StatefulReverb` do the same for the two
time-based effects: they carry the last ``taps * delay_samples`` (``delay``) input samples of every row, return chunks of the
chunk's shape, and one launch per chunk (``tfx_delay_stream_forward`` / ``tfx_delay_line_stream_forward``) gives the
one-shot effect's bits.  :class:`StatefulResample` converts the rate of a stream: it carries the last ``Lp_s - 1`` inputs of
every row, returns the outputs each chunk completes (``tfx_resample_stream_forward``), and its chunks plus ``flush()`` are
``resample_poly`` on the whole signal.  :class:`StatefulLimiter` is the look-ahead limiter of a stream: it carries the last
``D + A + H - 2`` (+ the detector interpolator's reach) inputs of every row, holds the last ``D = A - 1 + i_lo`` outputs back
(``tfx_limiter_stream_forward``, one launch per chunk), and its chunks plus ``flush()`` are ``limit`` on the whole signal;
``aligned=False`` gives the constant-latency form a sound card needs.  :class:`StatefulCompressor` is the compressor of a
stream: causal, no latency, it carries the detector's ``(y1, yL)`` per group (``tfx_compressor_forward``'s state), and its chunks
equal ``compress`` on the whole signal to float64 round-off of the detector (not bit for bit).  :class:`StatefulGate` is the noise
gate of a stream: causal, no latency, it carries ``(g, open, c)`` per group (``tfx_gate_forward``'s state); its decision is the
one-shot call's bit for bit and its gain equals it to float64 round-off.  :class:`StatefulChorus`,
:class:`StatefulFlanger` and :class:`StatefulVibrato` are the modulation effects of a stream: causal, no latency, they carry the
delay line's reach in ``_hist`` and the LFO's position in ``_pos`` (a device counter, ``tfx_modulated_delay_stream_forward``), and
their chunks are bit-identical to the one-shot effect on the whole signal.  :class:`StatefulPhaser` is the phaser of a stream:
causal, no latency, it carries the all-pass sections' states in ``_hist`` and the sweep's position in ``_pos``
(``tfx_phaser_forward``'s state and device counter); its coefficient track is bit-identical to the one-shot call's and its chunks
equal it to float64 round-off (not bit for bit).  :class:`StatefulFreeverb` is the room reverb of a
stream: causal, no latency, it carries every delay line in time order (``tfx_freeverb_forward``'s state), its chunks equal
``freeverb`` on the whole signal to float64 round-off (not bit for bit) and ``flush()`` returns the ring-out.
:class:`StatefulWaveshaper` and :class:`StatefulDistortion` are the oversampled waveshaper of a stream: they carry the last
``reach_before + reach_after`` inputs of every row, hold the last ``D = reach_before`` outputs back
(``tfx_waveshaper_stream_forward``, one launch per chunk), and their chunks plus ``flush()`` are bit-identical to ``waveshape`` on
the whole signal; ``aligned=False`` gives the constant-latency form.  The limiter and the waveshapers share their state machine,
:class:`_HoldBackStream`; the effects that cannot run chunk by chunk at all are one table, ``_REFUSALS``.

Small chunks are launch-bound (a 2 x 4096 step is ~60 us of host + launch overhead for a few us of
GPU work), so ``StreamProcessor(..., use_graph=True)`` captures one full-size chunk step -- every
effect's kernels plus the copies that carry the IIR states / FIR histories into persistent buffers --
into a HIP graph and replays it per chunk (the ragged last chunk runs eagerly).
"""
from __future__ import annotations

import abc
import dataclasses
import enum
import gc
import math
import os
import threading
import typing as tp
from collections.abc import Generator, Sequence

import torch
from torch import Tensor, nn

from torchfx_amd.effect import (FX, Chorus, Compressor, Delay, Distortion, Flanger, Freeverb, Gate, Limiter, LoudnessNormalize, ModulatedDelay,
                                MonoDelayStrategy, Phaser, PingPongDelayStrategy, Reverb, Vibrato, Waveshaper, _ext)
from torchfx_amd.filter._base import AbstractFilter
from torchfx_amd.filter.fir import FIR
from torchfx_amd.filter.zerophase import ZeroPhase
from torchfx_amd.resample import Resample, design_taps, window_key


def _rows(x: Tensor) -> int:
    if x.ndim not in (1, 2, 3):
        raise ValueError("Input must be of shape [T], [C, T], or [B, C, T]")
    return math.prod(x.shape[:-1])


class StatefulFIR(FIR):
    """FIR whose K-1 sample input history survives between calls (``reset_state()`` clears it):
    filtering a signal chunk by chunk equals filtering it in one piece."""

    DIRECT_BELOW_MACS = 1 << 31          # rows x samples x taps of a chunk below which the direct kernel is used

    def __init__(self, b, conv_mode: str = "fft") -> None:
        super().__init__(b, conv_mode)
        self._hist: Tensor | None = None

    def reset_state(self) -> None:
        self._hist = None

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        from torchfx_amd import torchfx_ext

        rows = _rows(x)
        xr = x.reshape(-1, x.shape[-1])
        taps = self.kernel.reshape(-1)
        k = taps.numel()
        if k == 1:
            return super().forward(x)
        # history and chunk stay in their own buffers (tfx_fir_stream_forward reads both); no torch.cat.
        # Small chunks take the one-launch direct kernel whatever the mode (a 2 x 512 chunk through the FFT path is
        # half a dozen launches for a microsecond of arithmetic); both paths meet the same 1e-5 bar.
        direct = self._conv_mode == "direct" or x.numel() * k <= self.DIRECT_BELOW_MACS
        y, self._hist = torchfx_ext.fir_stream_forward(xr, taps, _carried(self._hist, rows, k - 1, x), direct)
        return y.reshape(x.shape)


def _carried(hist: Tensor | None, rows: int, H: int, x: Tensor) -> Tensor | None:
    """The history a stateful effect carries into this chunk: None (silence) when there is none or the row count, dtype or
    device changed; when only its length ``H`` changed, the newest ``min(H_old, H)`` samples, zero-filled at the front."""
    if hist is None or hist.shape[0] != rows or hist.dtype != x.dtype or hist.device != x.device:
        return None
    old = hist.shape[1]
    if old == H:
        return hist
    out = torch.zeros(rows, H, dtype=x.dtype, device=x.device)
    k = min(old, H)
    if k:
        out[:, H - k:] = hist[:, old - k:]
    return out


def _native_stream(x: Tensor) -> bool:
    return x.is_cuda and x.dtype in (torch.float32, torch.float64)


class _RingOut:
    """The stream's last chunk as ``flush()`` needs it: ``_note(x)`` keeps its leading shape, dtype and device in ``_last``
    (``reset_state`` sets it to None) and ``_zeros(n)`` is a chunk of ``n`` zero samples shaped like it."""

    def _note(self, x: Tensor) -> None:
        self._last = (tuple(x.shape[:-1]), x.dtype, x.device)

    def _zeros(self, n: int) -> Tensor:
        lead, dtype, device = self._last
        return torch.zeros(*lead, n, dtype=dtype, device=device)


class StatefulDelay(_RingOut, Delay):
    """:class:`~torchfx_amd.effect.Delay` over a continuous stream: every chunk's output has the chunk's shape, the last
    ``H = taps * delay_samples`` input samples of every row are carried in ``_hist`` (``[rows, H]``) and :meth:`flush`
    returns the ring-out (``[..., H]``).  The chunks' outputs followed by the ring-out are bit-identical to ``Delay`` on
    the whole signal, on the same device and in the same dtype, whatever the chunk sizes (``csrc/delay.hip``).

    Device float32 / float64 chunks run one launch each (:func:`torchfx_ext.delay_stream_forward`); other chunks run the
    one-shot effect on ``[history | chunk]`` and keep the chunk's part.  The history restarts from silence when the row
    count, dtype or device changes; when ``H`` changes between chunks (``delay_samples``, ``taps``, or ``bpm`` /
    ``delay_time`` / ``fs`` of a BPM-synced instance) the newest samples are kept.  Only the stock strategies stream."""

    def __init__(self, delay_samples: int | None = None, bpm: float | None = None, delay_time: str = "1/8",
                 fs: int | None = None, feedback: float = 0.3, mix: float = 0.2, taps: int = 3,
                 strategy=None) -> None:
        super().__init__(delay_samples, bpm, delay_time, fs, feedback, mix, taps, strategy)
        if type(self.strategy) not in (MonoDelayStrategy, PingPongDelayStrategy):
            raise TypeError(f"StatefulDelay streams MonoDelayStrategy and PingPongDelayStrategy only, got {type(self.strategy).__name__}")
        self._bpm_synced = delay_samples is None
        self._bpm_key = (bpm, delay_time, fs) if self.delay_samples is not None else None
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None
        self._last: tuple | None = None

    def _delay(self) -> int:
        """The delay of this chunk: a BPM-synced instance follows ``bpm``, ``delay_time`` and ``fs``."""
        if self._bpm_synced and (self.bpm, self.delay_time, self.fs) != self._bpm_key:
            self._needs_calculation = True
            self._resolve()
            self._bpm_key = (self.bpm, self.delay_time, self.fs)
        self._resolve()
        return int(self.delay_samples)

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in (``StreamProcessor._graph_step`` recaptures when it changes)."""
        return self._delay(), int(self.taps), float(self.feedback), float(self.mix), type(self.strategy)

    def _sync_history(self) -> None:
        """Bring the carried history to the current ``H`` (newest samples kept) before a capture takes it as a home."""
        if self._hist is not None:
            self._hist = _carried(self._hist, self._hist.shape[0], int(self.taps) * self._delay(), self._hist)

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        rows = _rows(x)
        D = self._delay()
        taps = int(self.taps)
        H, T = taps * D, x.shape[-1]
        h = _carried(self._hist, rows, H, x)
        self._note(x)
        if _native_stream(x):
            y, self._hist = _ext().delay_stream_forward(x, h, D, taps, self.feedback, self.mix, self.pingpong(x))
            return y
        if h is None:
            h = torch.zeros(rows, H, dtype=x.dtype, device=x.device)
        v = torch.cat([h, x.reshape(rows, T)], dim=-1)
        self._hist = v[:, T:].clone()
        return Delay.forward(self, v.reshape(*x.shape[:-1], H + T))[..., H:H + T]

    @torch.no_grad()
    def flush(self) -> Tensor:
        """The ring-out of the stream (the last ``taps * delay_samples`` samples of the one-shot output), shaped like the
        last chunk; then the state is reset.  Without a chunk since the last reset: an empty tensor."""
        if self._last is None:
            return torch.zeros(0)
        tail = self.forward(self._zeros(int(self.taps) * self._delay()))
        self.reset_state()
        return tail


class StatefulReverb(Reverb):
    """:class:`~torchfx_amd.effect.Reverb` (``y[n] = x[n] + mix * decay * x[n - delay]``) over a continuous stream: the last
    ``delay`` input samples of every row are carried in ``_hist``, so a chunk's first ``delay`` outputs get the previous
    chunk's echo and chunks shorter than the delay are not passed through unchanged.  Output has the chunk's shape (no
    tail).  Chunked output equals ``Reverb`` on the whole signal (``torch.equal``).  Device float32 / float64 chunks run
    one launch each (:func:`torchfx_ext.delay_line_stream_forward`); other chunks run the one-shot effect on
    ``[history | chunk]`` -- which, like ``Reverb`` itself, needs a device: the library's delay line has no CPU path, so a CPU
    chunk longer than the history raises as ``Reverb`` does on a CPU signal longer than the delay."""

    def __init__(self, delay: int = 4410, decay: float = 0.5, mix: float = 0.5) -> None:
        super().__init__(delay, decay, mix)
        self._hist: Tensor | None = None

    def reset_state(self) -> None:
        self._hist = None

    def _capture_key(self) -> tuple:
        return int(self.delay), float(self.decay), float(self.mix)

    def _sync_history(self) -> None:
        if self._hist is not None:
            self._hist = _carried(self._hist, self._hist.shape[0], int(self.delay), self._hist)

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        rows = _rows(x)
        D, T = int(self.delay), x.shape[-1]
        h = _carried(self._hist, rows, D, x)
        if _native_stream(x):
            y, self._hist = _ext().delay_line_stream_forward(x, h, D, self.decay, self.mix)
            return y
        xr = x.reshape(rows, T)
        if h is None:                                   # the stream starts here: the one-shot effect on the chunk itself
            self._hist = torch.cat([torch.zeros(rows, D, dtype=x.dtype, device=x.device), xr], dim=-1)[:, T:].clone()
            return Reverb.forward(self, x)
        v = torch.cat([h, xr], dim=-1)
        self._hist = v[:, T:].clone()
        return Reverb.forward(self, v.reshape(*x.shape[:-1], D + T))[..., D:]


class StatefulResample(_RingOut, Resample):
    """:class:`~torchfx_amd.resample.Resample` over a continuous stream: chunks go in, the converted signal comes out in
    pieces with no seam.  After chunks of ``N`` input samples per row in all the stream has returned exactly
    ``M(N) = max(0, ceil(N * up / down) - latency)`` outputs, each final; :meth:`flush` returns the ``latency`` (at most)
    outputs still held back.  All chunk outputs followed by ``flush()`` are :func:`~torchfx_amd.resample.resample_poly` on the
    whole signal, ``ceil(N * up / down)`` samples: on the device ``torch.equal`` to it for finite float32 / float64 input,
    whatever the chunk sizes.  A chunk may return zero samples.

    Every row carries its last ``history_length`` input samples in ``_hist``, and the stream two host integers: the inputs
    consumed and the outputs emitted (so no chunk waits on the device).  Device float32 / float64 chunks run one launch each
    (:func:`torchfx_ext.resample_stream_forward`); CPU chunks run ``scipy.signal.upfirdn`` on ``[history | chunk]``.  The
    stream restarts from silence when the row count, dtype or device changes, and when ``new_fs``, ``fs`` or ``window``
    changes between chunks -- the outputs still held back are then dropped.  A ``Wave`` is a whole signal: pipe it through
    ``Resample`` or use ``Wave.resample`` instead."""

    holds_back = True                               # chunks may return fewer samples than they take; flush() hands out the rest
    _hold_rank = 0                                  # see _held_back
    _wave_refusal = ("StatefulResample is for chunked streams (StreamProcessor): a Wave is a whole signal, and a stream's forward "
                     "holds back its last outputs; pipe it through Resample or call Wave.resample instead")

    def __init__(self, new_fs: int, fs: int | None = None, window=("kaiser", 5.0)) -> None:
        super().__init__(new_fs, fs, window)
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None
        self._consumed = 0                          # N: input samples per row so far
        self._emitted = 0                           # M(N): output samples per row so far
        self._key: tuple | None = None              # (rows, dtype, device, new_fs, fs, window) of the running stream
        self._geo: tuple[int, int] = (0, 0)         # its (n_pre_remove, history length)
        self._last: tuple | None = None

    def _geometry(self, up: int, down: int) -> tuple[int, int]:
        """``(n_pre_remove, Lp_s - 1)`` of the designed filter: the outputs held back and the history length."""
        if up == down:
            return 0, 0
        nh = int(design_taps(up, down, self.window, torch.float32).numel())
        half_len = (nh - 1) // 2
        pre_pad = down - half_len % down
        return (half_len + pre_pad) // down, -(-(nh + pre_pad) // up) - 1

    @property
    def latency(self) -> int:
        """The outputs a stream holds back (``n_pre_remove``): what :meth:`flush` returns at most."""
        return self._geometry(*self._ratio())[0]

    @property
    def history_length(self) -> int:
        """The input samples every row carries between chunks (``Lp_s - 1``)."""
        return self._geometry(*self._ratio())[1]

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (<kernel>)`` for the next chunk of ``x`` (``length`` samples, default x's), or the host / refusal route."""
        if not x.is_cuda or x.dtype not in (torch.float32, torch.float64):
            return super().route(x, length)
        from torchfx_amd import torchfx_ext

        up, down = self._ratio()
        if up == down:
            return "native (copy)"
        n = int(x.shape[-1]) if length is None else int(length)
        taps = int(design_taps(up, down, self.window, x.dtype).numel())
        return f"native ({torchfx_ext.resample_stream_plan_info(self._consumed, n, up, down, taps, x.dtype)['kernel']})"

    def _emit_count(self, n: int, up: int, down: int, pre: int) -> int:
        return max(0, -(-n * up // down) - pre)

    def _graph_ready(self, x: Tensor) -> bool:
        """Never: a replay skips :meth:`forward`, which counts the samples of every chunk."""
        return False

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        rows = _rows(x)
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"StatefulResample: float32 or float64 signals only, got {x.dtype}")
        up, down = self._ratio()
        key = (rows, x.dtype, x.device, self.new_fs, self.fs, window_key(self.window))
        if key != self._key:                        # a new stream: from silence
            self.reset_state()
            self._key, self._geo = key, self._geometry(up, down)
        self._note(x)
        T = x.shape[-1]
        if up == down:
            y = x.clone()
        else:
            h = design_taps(up, down, self.window, x.dtype)
            if x.is_cuda:
                from torchfx_amd import torchfx_ext

                with torch.cuda.device(x.device):
                    y, self._hist = torchfx_ext.resample_stream_forward(x, h, self._hist, up, down, self._consumed)
            else:
                y = self._host_chunk(x, rows, up, down, h)
        self._consumed += T
        self._emitted = self._consumed if up == down else self._emit_count(self._consumed, up, down, self._geo[0])
        return y

    def _host_chunk(self, x: Tensor, rows: int, up: int, down: int, h: Tensor) -> Tensor:
        """One chunk on the host: ``scipy.signal.upfirdn`` over ``[history | chunk]``, from a window start that is a multiple
        of ``down`` so the phases are the whole signal's."""
        import numpy as np
        from scipy.signal import upfirdn

        pre, H = self._geo
        N, T = self._consumed, x.shape[-1]
        xr = x.detach().reshape(rows, T)
        hist = self._hist if self._hist is not None else torch.zeros(rows, H, dtype=x.dtype)
        v = torch.cat([hist, xr], dim=-1)                   # absolute inputs [N - H, N + T), zeros before 0
        self._hist = v[:, v.shape[-1] - H:].clone()
        m0, m1 = self._emit_count(N, up, down, pre), self._emit_count(N + T, up, down, pre)
        lead = tuple(x.shape[:-1])
        if m1 == m0:
            return torch.zeros(*lead, 0, dtype=x.dtype)
        s = (N - H) // down * down                           # window start, <= N - H; inputs before N - H meet no tap
        hn = h.numpy()
        half_len = (hn.size - 1) // 2
        hp = np.concatenate([np.zeros(down - half_len % down, dtype=hn.dtype), hn])
        vv = np.concatenate([np.zeros((rows, N - H - s), dtype=hn.dtype), v.numpy()], axis=-1)
        yu = upfirdn(hp, vv, up, down, axis=-1)
        r0 = m0 + pre - up * (s // down)                      # upfirdn output r is output r + up*s/down - pre of the whole
        out = np.zeros((rows, m1 - m0), dtype=yu.dtype)
        got = yu[:, r0:r0 + m1 - m0]
        out[:, :got.shape[-1]] = got
        return torch.from_numpy(out.astype(hn.dtype, copy=False)).reshape(*lead, m1 - m0)

    @torch.no_grad()
    def flush(self) -> Tensor:
        """The outputs still held back (``ceil(N * up / down) - M(N)``, at most :attr:`latency`), computed with zeros past
        the end and shaped like the last chunk; then the state is reset.  Without a chunk since the last reset: an empty
        tensor."""
        if self._last is None:
            return torch.zeros(0)
        up, down = self._ratio()
        pre = self._geometry(up, down)[0]
        N = self._consumed
        rem = -(-N * up // down) - self._emitted
        if rem <= 0:
            tail = self._zeros(0)
        else:
            Z = -(-pre * down // up)                       # zeros that complete every held-back output
            while self._emit_count(N + Z, up, down, pre) - self._emitted < rem:
                Z += 1
            tail = self.forward(self._zeros(Z))[..., :rem].contiguous()
        self.reset_state()
        return tail


class _HoldBackStream(_RingOut):
    """The state machine of a stream whose outputs read ``D`` input samples ahead (:class:`StatefulLimiter`,
    :class:`_ShaperStream`); mixed in in front of the effect class.  After ``N`` input samples per row the stream has returned the
    first ``max(0, N - D)`` samples of the one-shot result, and :meth:`flush` returns the remaining ``min(N, D)``.  Every row
    carries its last ``Hs`` input samples in ``_hist`` (``[rows, Hs]``) and the stream one host integer, ``_pos = min(N, Hs + D)``;
    ``aligned`` chooses between the outputs a chunk completes and the chunk's shape, delayed by ``D``.  A subclass says what its
    stream is made of in three hooks:

    * ``_stream(lead, dtype, device) -> (ctx, key, (D, Hs))`` for chunks of leading shape ``lead``: ``ctx`` is what the other two
      hooks need, a stream lives while ``key`` stays, and ``(D, Hs)`` comes from :meth:`_geometry`;
    * ``_launch(x, ctx, n_in=None) -> y``: one native launch on the chunk ``x`` behind ``_hist`` at position ``_pos``; it stores
      the new history unless ``n_in`` (the number of real inputs in ``x``) is given;
    * ``_one_shot_host(v, ctx) -> [rows, n]``: the effect's host definition on the whole signal ``v [rows, n]``."""

    holds_back = True                               # chunks may return fewer samples than they take; flush() hands out the rest
    _aligned_refusal = ("{name}(aligned=True) cannot run in RealtimeProcessor: it returns the outputs a block completes, fewer for "
                        "the first block, and a sound card's output block has the input block's length; construct it with "
                        "aligned=False (constant latency: the result delayed by its `latency` samples)")

    def __init__(self, *args, aligned: bool = True, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.aligned = bool(aligned)
        self._geos: dict = {}
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None
        self._pos = 0                               # min(N, Hs + D): input samples per row so far, as far as it matters
        self._key: tuple | None = None              # what the running stream is bound to (see _stream)
        self._geo: tuple[int, int] = (0, 0)         # its (D, Hs)
        self._last: tuple | None = None

    def _geometry(self, query: str, *key) -> tuple[int, int]:
        """``(D, Hs)`` of the stream: the latency and history that the effect's stream plan query (``torchfx_ext.<query>``,
        host-only) gives for ``key``, the sizes they depend on; asked once per key."""
        geo = self._geos.get(key)
        if geo is None:
            info = getattr(_ext(), query)(0, *key)
            geo = self._geos[key] = (info["latency"], info["history"])
        return geo

    @property
    def latency(self) -> int:
        """The samples the stream holds back (``D``): what :meth:`flush` returns at most, and the delay of ``aligned=False``."""
        return self._stream((), torch.float32, None)[2][0]

    @property
    def history_length(self) -> int:
        """The input samples every row carries between chunks (``Hs``; the class says what it is made of)."""
        return self._stream((), torch.float32, None)[2][1]

    def _sync_history(self) -> None:
        """Nothing to resize: a parameter that changes the history's length restarts the stream (``_graph_ready``)."""

    def _graph_ready(self, x: Tensor) -> bool:
        """A replay skips :meth:`forward`: it leaves nothing stale once the position counter has saturated, for the stream
        that is running."""
        if self._key is None or self._pos != sum(self._geo):
            return False
        return self._stream(tuple(x.shape[:-1]), x.dtype, x.device)[1] == self._key

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        _rows(x)
        ctx, key, geo = self._stream(tuple(x.shape[:-1]), x.dtype, x.device)
        if key != self._key:                        # a new stream: from silence
            self.reset_state()
            self._key, self._geo = key, geo
        self._note(x)
        (D, Hs), N, T = geo, self._pos, x.shape[-1]
        if T == 0:
            return torch.zeros_like(x)
        y = self._launch(x, ctx) if _native_stream(x) else self._host_chunk(x, ctx)
        self._pos = min(N + T, Hs + D)
        k = min(T, max(0, D - N)) if self.aligned else 0         # outputs in front of position 0
        return y[..., k:] if k else y

    def _window(self, rows: int, dtype: torch.dtype) -> tuple[Tensor, Tensor]:
        """``(history [rows, Hs], its valid part)``: the part starts at position 0 while the stream is younger than ``Hs``."""
        Hs = self._geo[1]
        hist = self._hist.cpu() if self._hist is not None else torch.zeros(rows, Hs, dtype=dtype)
        return hist, hist[:, Hs - min(self._pos, Hs):]

    def _host_chunk(self, x: Tensor, ctx) -> Tensor:
        """One chunk on the host: the one-shot definition on ``[history | chunk]`` -- its start is position 0 or a sample no
        output of the chunk reads behind, its end a sample none reads past, so no output that is cut out of it reads a truncated
        edge -- and the chunk's outputs cut from it."""
        (D, Hs), N, T = self._geo, self._pos, x.shape[-1]
        rows = math.prod(x.shape[:-1])
        hist, valid = self._window(rows, x.dtype)
        xr = x.detach().reshape(rows, T).cpu()
        v = torch.cat([valid, xr], dim=-1)                   # positions [N - valid, N + T)
        self._hist = torch.cat([hist, xr], dim=-1)[:, T:].to(x.device)
        out = torch.zeros(rows, T, dtype=x.dtype)
        lo = max(0, N - D)
        n = N + T - D - lo
        if n > 0:
            s = lo - (N - valid.shape[-1])
            out[:, T - n:] = self._one_shot_host(v, ctx)[:, s:s + n]
        return out.reshape(x.shape).to(x.device)

    @torch.no_grad()
    def flush(self) -> Tensor:
        """The outputs still held back (the last ``min(N, latency)`` samples of the one-shot result), computed with the stream
        ending here and shaped like the last chunk; then the state is reset.  Without a chunk since the last reset, or after a
        parameter change that restarts the stream: an empty tensor."""
        if self._last is None:
            return torch.zeros(0)
        lead, dtype, device = self._last
        ctx, key, _ = self._stream(lead, dtype, device)
        D, N = self._geo[0], self._pos
        n = min(N, D) if key == self._key else 0
        if n == 0:
            tail = self._zeros(0)
        elif device.type == "cuda":                   # a chunk of D samples with no input in it: the stream ends at N
            tail = self._launch(self._zeros(D), ctx, 0)[..., D - n:].contiguous()
        else:
            v = self._window(math.prod(lead), dtype)[1]
            tail = self._one_shot_host(v, ctx)[:, v.shape[-1] - n:].reshape(*lead, n).to(device)
        self.reset_state()
        return tail


class StatefulLimiter(_HoldBackStream, Limiter):
    """:class:`~torchfx_amd.effect.Limiter` over a continuous stream: chunks go in, the limited signal comes out with no seam.
    The gain at a sample reads ``latency`` = ``D = A - 1 + i_lo`` samples ahead (``A`` the look-ahead in samples, ``i_lo`` the
    detector interpolator's forward reach: 0 for ``detector="sample"``, 10 for the library's filters), so after ``N`` input
    samples per row the stream has returned the first ``max(0, N - D)`` samples of :func:`~torchfx_amd.limiter.limit` on the
    whole signal, each final, and :meth:`flush` returns the remaining ``min(N, D)``, computed with the stream ending at ``N``.

    * ``aligned=True``: a chunk returns the outputs it completes -- ``max(0, N + T - D) - max(0, N - D)`` samples, possibly
      none.  All chunk outputs followed by ``flush()`` are ``limit`` on the whole signal: ``torch.equal``, on the same device
      and in the same dtype, whatever the chunk sizes.
    * ``aligned=False`` (constant latency, what a sound card needs): every chunk returns the chunk's shape, the one-shot result
      delayed by ``D`` samples with zeros first; ``flush()`` still returns the last ``min(N, D)``.

    Every row carries its last ``history_length`` input samples in ``_hist`` (``[rows, Hs]``) and the stream one host integer,
    ``min(N, Hs + D)``: no chunk waits on the device.  Device float32 / float64 chunks run one launch each
    (:func:`torchfx_ext.limiter_stream_forward`, which reads the history and the chunk from their two buffers and sweeps only the
    positions the chunk's outputs depend on); CPU chunks run the host definition on ``[history | chunk]``.  The stream restarts
    from silence -- and what is held back is dropped -- when the row count, dtype, device or ``link`` grouping changes and when
    ``lookahead``, ``hold``, ``detector``, ``oversample``, ``taps`` or ``fs`` changes.  A changed ``ceiling_db`` or ``window`` (of
    the same length) applies from the next chunk on without a restart; such a run equals no one-shot call.  A NaN or Inf makes
    the outputs of the chunks whose ``[history | chunk]`` still holds it NaN (all channels of the group); after that the stream
    is the clean stream's again, bit for bit.  A ``Wave`` is a whole signal: pipe it through ``Limiter`` instead."""

    _hold_rank = 1                                  # see _held_back
    _wave_refusal = ("StatefulLimiter is for chunked streams (StreamProcessor, RealtimeProcessor): a Wave is a whole signal, and a "
                     "stream's forward holds back its last outputs; pipe it through Limiter instead")
    _aligned_refusal = ("{name}(aligned=True) cannot run in RealtimeProcessor: it returns the outputs a block completes, none for "
                        "the first blocks, and a sound card's output block has the input block's length; construct it with "
                        "aligned=False (constant latency: the result delayed by {name}.latency samples)")

    def __init__(self, ceiling_db: float = -1.0, lookahead: float = 1.5e-3, hold: float = 10e-3, detector: str = "true_peak",
                 link: bool = True, oversample: int | None = None, taps=None, window=None, fs: int | None = None,
                 aligned: bool = True) -> None:
        super().__init__(ceiling_db, lookahead, hold, detector, link, oversample, taps, window, fs, aligned=aligned)
        self._pcache: tuple | None = None

    def _params(self, dtype: torch.dtype):
        """``self.params(dtype)``, kept while the attributes it is made from stay what they were."""
        ver = tuple((id(v), getattr(v, "_version", None)) for v in (self.taps, self.window))
        key = (dtype, self.fs, self.ceiling_db, self.lookahead, self.hold, self.detector, self.oversample, ver)
        if self._pcache is None or self._pcache[0] != key:
            self._pcache = (key, self.params(dtype), (self.taps, self.window))
        return self._pcache[1]

    def _stream(self, lead: tuple, dtype: torch.dtype, device) -> tuple:
        """``((P, groups, channels), key, (D, Hs))`` for chunks of leading shape ``lead``: a stream lives while ``key`` stays.
        ``Hs = D + A + H - 2`` plus the interpolator's backward reach (``tfx_limiter_stream_plan_info``)."""
        P = self._params(dtype)
        channels = int(lead[-1]) if (self.link and lead) else 1        # limiter._grouping, from the leading shape
        groups = math.prod(lead) // channels if channels else 0
        ntaps = 0 if P.taps is None else int(P.taps.numel())
        key = (groups, channels, dtype, device, P.A, P.H, P.up, None if P.taps is None else P.taps.numpy().tobytes())
        return (P, groups, channels), key, self._geometry("limiter_stream_plan_info", P.A, P.H, P.up, ntaps)

    def _launch(self, x: Tensor, ctx, n_in: int | None = None) -> Tensor:
        P, _, channels = ctx
        with torch.cuda.device(x.device):
            y, _, hist = _ext().limiter_stream_forward(x, self._hist, self._pos, P.c, P.A, P.H, torch.from_numpy(P.w), P.up, P.taps,
                                                       channels, False, n_in)
        if n_in is None:
            self._hist = hist
        return y

    def _one_shot_host(self, v: Tensor, ctx) -> Tensor:
        from torchfx_amd.limiter import _limit_host

        return _limit_host(v, *ctx)[0]

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (limiter_stream_kernel, ...)`` for the next chunk of ``x``, or the host / refusal route."""
        if not _native_stream(x):
            return super().route(x, length)
        try:
            P = self.params(x.dtype)
            n = int(x.shape[-1]) if length is None else int(length)
            info = _ext().limiter_stream_plan_info(n, P.A, P.H, P.up, 0 if P.taps is None else int(P.taps.numel()), x.dtype)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        det = f"{P.up}x oversampled detector" if P.up > 1 else "sample-peak detector"
        return (f"native (limiter_stream_kernel, {det}, look-ahead {P.A} / hold {P.H} samples, latency {info['latency']}, history "
                f"{info['history']}, {info['tiles']} tile(s), {info['positions']} of 8192 positions swept; one launch)")

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in (the ceiling and the window among it)."""
        dtype = self._last[1] if self._last is not None else torch.float32
        return self._params(dtype).key(), self.link, self.aligned


class StatefulCompressor(Compressor):
    """:class:`~torchfx_amd.effect.Compressor` over a continuous stream: the detector's state ``(y1, yL)`` per group goes from
    chunk to chunk, so the gain curve has no seam.  The compressor is causal with no latency: every chunk returns the chunk's
    shape and there is nothing to flush.

    The state lives in ``_hist`` (``[groups, 2]`` float64 on the chunks' device) and is rebuilt from silence when the row
    count, the ``link`` grouping or the device changes; :meth:`reset_state` does the same on request.  A changed parameter
    applies from the next chunk on.  All chunks together equal :func:`~torchfx_amd.dynamics.compress` on the whole signal to
    float64 round-off of the detector -- within 1e-10 dB of gain -- and not bit for bit: the scan's association follows the
    cut.  After a NaN or Inf the state of its group is NaN and stays so until :meth:`reset_state`.  Device float32 / float64
    chunks run :func:`torchfx_ext.compressor_forward` (one launch for a chunk of up to 2048 samples), CPU chunks the host
    path."""

    def __init__(self, threshold_db: float = -20.0, ratio: float = 4.0, attack: float = 5e-3, release: float = 100e-3,
                 knee_db: float = 6.0, makeup_db: float = 0.0, link: bool = True, fs: int | None = None) -> None:
        super().__init__(threshold_db, ratio, attack, release, knee_db, makeup_db, link, fs)
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None            # [groups, 2] float64 (y1, yL); None = silence
        self._key: tuple | None = None              # what the running stream is bound to

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in."""
        return (self.threshold_db, self.ratio, self.attack, self.release, self.knee_db, self.makeup_db, self.link, self.fs)

    def _sync_history(self) -> None:
        """Nothing to resize: the state's shape follows the rows alone."""

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        _rows(x)
        if self.fs is None:
            raise ValueError("StatefulCompressor needs the sample rate: pass fs or let the processor configure it")
        from torchfx_amd.dynamics import compress

        key = (tuple(x.shape[:-1]), self.link, x.device)
        if key != self._key:                        # a new stream: from silence
            self.reset_state()
            self._key = key
        y, self._hist = compress(x, self.fs, self.threshold_db, self.ratio, self.attack, self.release, self.knee_db, self.makeup_db,
                                 self.link, state=self._hist, return_state=True)
        return y


class StatefulGate(Gate):
    """:class:`~torchfx_amd.effect.Gate` over a continuous stream: the state ``(g, open, c)`` per group -- the smoothed gain, the
    decision and the hold counter -- goes from chunk to chunk, so neither the gain curve nor the hold has a seam.  The gate is
    causal with no latency: every chunk returns the chunk's shape and there is nothing to flush.

    The state lives in ``_hist`` (``[groups, 3]`` float64 on the chunks' device) and is rebuilt from the closed gate when the
    row count, the ``link`` grouping or the device changes; :meth:`reset_state` does the same on request.  A changed parameter
    applies from the next chunk on.  The decision of all chunks together is :func:`~torchfx_amd.gate.gate`'s on the whole
    signal bit for bit; the gain equals it to float64 round-off (the scan's association follows the cut).  After a NaN or Inf
    the state of its group is NaN and stays so until :meth:`reset_state`.  Device float32 / float64 chunks run
    :func:`torchfx_ext.gate_forward` (one launch for a chunk of up to 2048 samples), CPU chunks the host path."""

    def __init__(self, threshold_db: float = -40.0, hysteresis_db: float = 6.0, range_db: float = math.inf, attack: float = 1e-3,
                 hold: float = 50e-3, release: float = 100e-3, link: bool = True, fs: int | None = None) -> None:
        super().__init__(threshold_db, hysteresis_db, range_db, attack, hold, release, link, fs)
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None            # [groups, 3] float64 (g, open, c); None = closed, g = r
        self._key: tuple | None = None              # what the running stream is bound to

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in."""
        return (self.threshold_db, self.hysteresis_db, self.range_db, self.attack, self.hold, self.release, self.link, self.fs)

    def _sync_history(self) -> None:
        """Nothing to resize: the state's shape follows the rows alone."""

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        _rows(x)
        if self.fs is None:
            raise ValueError("StatefulGate needs the sample rate: pass fs or let the processor configure it")
        from torchfx_amd.gate import gate

        key = (tuple(x.shape[:-1]), self.link, x.device)
        if key != self._key:                        # a new stream: from the closed gate
            self.reset_state()
            self._key = key
        y, self._hist = gate(x, self.fs, self.threshold_db, self.hysteresis_db, self.range_db, self.attack, self.hold, self.release,
                             self.link, state=self._hist, return_state=True)
        return y


class StatefulFreeverb(_RingOut, Freeverb):
    """:class:`~torchfx_amd.effect.Freeverb` over a continuous stream: the delay lines go from chunk to chunk, so the room's
    tail has no seam.  The reverb is causal with no latency: every chunk returns the chunk's shape; with ``tail > 0``
    :meth:`flush` returns the ring-out (``[..., floor(tail fs + 0.5)]``) and resets the state.

    The state lives in ``_hist`` (``[banks, state_len]`` float64 on the chunks' device: per bank every comb's last ``D`` values
    and its low-pass state, then every all-pass's last ``D`` values, oldest first -- :func:`~torchfx_amd.reverb.freeverb_bank`)
    and is rebuilt from silence when the leading shape, the device or the sample rate changes; :meth:`reset_state` does the
    same on request.  ``room_size``, ``damping``, ``wet``, ``dry`` and ``width`` may change between chunks.  The state is in time
    order, so chunks shorter than a delay work and the state does not depend on the chunk sizes; all chunks together (then
    ``flush()``) equal :func:`~torchfx_amd.reverb.freeverb` on the whole signal to float64 round-off and not bit for bit: the
    damping scan's association follows the cut.  After a NaN or Inf the state of its item is not finite and stays so until
    :meth:`reset_state`.  Device float32 / float64 chunks run :func:`torchfx_ext.freeverb_forward`, CPU chunks the host path."""

    def __init__(self, room_size: float = 0.5, damping: float = 0.5, wet: float = 1.0 / 3.0, dry: float = 0.5, width: float = 1.0,
                 tail: float = 0.0, fs: int | None = None) -> None:
        super().__init__(room_size, damping, wet, dry, width, tail, fs)
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None            # [banks, state_len] float64; None = silence
        self._key: tuple | None = None              # what the running stream is bound to
        self._last: tuple | None = None

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in."""
        return (self.room_size, self.damping, self.wet, self.dry, self.width, self.fs)

    def _sync_history(self) -> None:
        """Nothing to resize: the state's shape follows the rows and the rate alone, and a change of either restarts the stream."""

    def _call_tail(self, F) -> int:
        return 0                                    # a chunk returns the chunk's shape; the ring-out is flush()'s

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        _rows(x)
        if self.fs is None:
            raise ValueError("StatefulFreeverb needs the sample rate: pass fs or let the processor configure it")
        from torchfx_amd.reverb import _shape, freeverb_bank

        key = (tuple(x.shape[:-1]), x.device, self.fs)
        if key != self._key:                        # a new stream: from silence
            self.reset_state()
            self._key = key
        self._note(x)
        P = self.params().bank(_shape(x)[1])
        y, self._hist = freeverb_bank(x, P.comb, P.allpass, P.fb, P.d1, P.g, P.input_gain, P.dry, P.wet1, P.wet2, 0, self._hist, True)
        return y

    @torch.no_grad()
    def flush(self) -> Tensor:
        """The ring-out of the stream (the ``floor(tail fs + 0.5)`` samples the one-shot effect appends), shaped like the last
        chunk; then the state is reset.  Without a chunk since the last reset, or with ``tail = 0``: an empty tensor."""
        if self._last is None:
            return torch.zeros(0)
        n = self.params().tail_samples
        out = self.forward(self._zeros(n)) if n else self._zeros(0)
        self.reset_state()
        return out


class _ShaperStream(_HoldBackStream):
    """An oversampled waveshaper (:class:`~torchfx_amd.effect.Waveshaper`) over a continuous stream; mixed in in front of the
    effect class.  An output reads ``latency`` = ``D = reach_before`` samples ahead and ``reach_after`` behind
    (:func:`torchfx_ext.waveshaper_plan_info`: 21 and 20 for the default window at every ``oversample > 1``), so after ``N``
    input samples per row the stream has returned the first ``max(0, N - D)`` samples of
    :func:`~torchfx_amd.waveshaper.waveshape` on the whole signal, each final, and :meth:`flush` returns the remaining
    ``min(N, D)``, computed with the stream ending at ``N``.  ``oversample=1`` is memoryless: no history, no latency, nothing to
    flush.

    * ``aligned=True``: a chunk returns the outputs it completes -- ``max(0, N + T - D) - max(0, N - D)`` samples, possibly
      none.  All chunk outputs followed by ``flush()`` are ``waveshape`` on the whole signal: ``torch.equal``, on the same device
      and in the same dtype, whatever the chunk sizes, a NaN's or an Inf's reach included.
    * ``aligned=False`` (constant latency, what a sound card needs): every chunk returns the chunk's shape, the one-shot result
      delayed by ``D`` samples with zeros first; ``flush()`` still returns the last ``min(N, D)``.

    Every row carries its last ``history_length`` = ``Hs = reach_before + reach_after`` input samples in ``_hist``
    (``[rows, Hs]``) and the stream one host integer, ``min(N, Hs + D)``: no chunk waits on the device.  Device float32 / float64
    chunks run one launch each (:func:`torchfx_ext.waveshaper_stream_forward`, which reads the history and the chunk from their
    two buffers); CPU chunks run the host definition on ``[history | chunk]``.  ``drive_db``, ``bias``, ``mix``, ``output_db``,
    ``shape`` and ``curve`` may change between chunks without a restart; such a run equals no one-shot call.  The stream restarts
    from silence -- and what is held back is dropped -- when ``oversample`` or the taps of ``window`` change and when the row count,
    dtype or device changes.  A ``Wave`` is a whole signal: pipe it through ``Waveshaper`` / ``Distortion`` instead."""

    _hold_rank = 2                                  # see _held_back
    _wave_refusal = ("StatefulWaveshaper / StatefulDistortion are for chunked streams (StreamProcessor, RealtimeProcessor): a Wave is "
                     "a whole signal, and a stream's forward holds back its last outputs; pipe it through Waveshaper or Distortion "
                     "instead")

    def _stream(self, lead: tuple, dtype: torch.dtype, device) -> tuple:
        """``((P, taps up, taps down), key, (D, Hs))`` for chunks of leading shape ``lead``: a stream lives while ``key`` stays.
        ``Hs = reach_before + reach_after`` (``tfx_waveshaper_stream_plan_info``)."""
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{type(self).__name__}: float32 or float64 signals only, got {dtype}")
        from torchfx_amd.waveshaper import check_gains

        P = self.params()
        check_gains(P, dtype)
        up, dn = P.taps(dtype)
        taps = None if up is None else (up.numpy().tobytes(), dn.numpy().tobytes())
        geo = self._geometry("waveshaper_stream_plan_info", P.oversample, 0 if up is None else int(up.numel()),
                             0 if dn is None else int(dn.numel()))
        return (P, up, dn), (math.prod(lead), dtype, device, P.oversample, taps), geo

    def _launch(self, x: Tensor, ctx, n_in: int | None = None) -> Tensor:
        P, up, dn = ctx
        curve = None if P.curve is None else torch.from_numpy(P.curve).to(x.dtype)
        with torch.cuda.device(x.device):
            y, hist = _ext().waveshaper_stream_forward(x, self._hist, self._pos, P.oversample, P.shape, curve, P.drive, P.bias, P.dry,
                                                       P.wet, up, dn, n_in)
        if n_in is None:
            self._hist = hist
        return y

    def _one_shot_host(self, v: Tensor, ctx) -> Tensor:
        from torchfx_amd.waveshaper import _waveshape_host

        return _waveshape_host(v, ctx[0])

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (waveshaper_stream_kernel, ...)`` for the next chunk of ``x``, or the host / refusal route."""
        if not _native_stream(x):
            return super().route(x, length)
        try:
            P = self.params()
            up, dn = P.taps(x.dtype)
            n = int(x.shape[-1]) if length is None else int(length)
            info = _ext().waveshaper_stream_plan_info(n, P.oversample, 0 if up is None else up.numel(), 0 if dn is None else dn.numel(),
                                                      0 if P.curve is None else P.curve.size, x.dtype)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        return (f"native (waveshaper_stream_kernel, L = {P.oversample}, {P.shape}, latency {info['latency']}, history {info['history']}, "
                f"{info['tiles']} tile(s) of {info['tile']}, {info['positions']} positions up-sampled and shaped; one launch)")

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in: every parameter of the launch."""
        P = self.params()
        return (P.shape, None if P.curve is None else P.curve.tobytes(), P.drive, P.bias, P.oversample, P.dry, P.wet,
                window_key(P.window), self.aligned)


class StatefulWaveshaper(_ShaperStream, Waveshaper):
    """:class:`~torchfx_amd.effect.Waveshaper` over a continuous stream, with its constructor arguments plus ``aligned``
    (see :class:`_ShaperStream`)."""


class StatefulDistortion(_ShaperStream, Distortion):
    """:class:`~torchfx_amd.effect.Distortion` over a continuous stream, with its constructor arguments plus ``aligned``
    (see :class:`_ShaperStream`)."""


class _ModulationStream:
    """A modulated delay line (:class:`~torchfx_amd.effect.ModulatedDelay`) over a continuous stream; mixed in in front of the
    effect class.  Every row carries its last ``H = max_v floor(delay_v + depth_v) + 2`` input samples in ``_hist``
    (``[rows, H]``, the stream-history contract, :func:`_carried`) and the stream the absolute position of its next sample in
    ``_pos`` (int64 ``[1]`` on the chunks' device: a replayed HIP graph bakes host scalars in, a device counter moves on with
    every replay).  The stream is causal with no latency: every chunk returns the chunk's shape and there is nothing to flush.
    All chunks together are ``torch.equal`` to the one-shot effect on the whole signal, whatever the chunk sizes.

    The stream restarts from silence and position 0 when the row count, dtype or device changes; :meth:`reset_state` does the
    same on request.  When a changed parameter changes ``H`` the newest samples are kept.  Device float32 / float64 chunks run
    one launch each (:func:`torchfx_ext.modulated_delay_stream_forward`), CPU chunks the host path on ``[history | chunk]``
    with the absolute position."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None            # [rows, H]; None = silence
        self._pos: Tensor | None = None             # int64 [1] on the chunks' device; None = 0

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in: every parameter of the launch."""
        return (tuple(self.voices), self.dry, self.spread, self.shape, self.interpolation, self.pad, self.fs)

    def _sync_history(self) -> None:
        """Bring the carried history to the current ``H`` (newest samples kept) before a capture takes it as a home."""
        if self._hist is not None and self.fs is not None:
            self._hist = _carried(self._hist, self._hist.shape[0], self.params(self._hist.dtype).history, self._hist)

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        rows = _rows(x)
        if self.fs is None:
            raise ValueError(f"{type(self).__name__} needs the sample rate: pass fs or let the processor configure it")
        P = self.params(x.dtype)
        h = _carried(self._hist, rows, P.history, x)
        if h is None or self._pos is None or self._pos.device != x.device:      # a new stream: silence, position 0
            h, self._pos = None, None
        if _native_stream(x):
            with torch.cuda.device(x.device):
                y, self._hist, self._pos = _ext().modulated_delay_stream_forward(x, h, self._pos, P.table, P.spread, P.dry, P.shape,
                                                                                 P.interpolation)
            return y
        from torchfx_amd.modulation import modulate_stream_host

        pos = 0 if self._pos is None else int(self._pos)
        y, self._hist = modulate_stream_host(x, h, P, pos)
        self._pos = torch.tensor([pos + x.shape[-1]], dtype=torch.int64, device=x.device)
        return y


class StatefulChorus(_ModulationStream, Chorus):
    """:class:`~torchfx_amd.effect.Chorus` over a continuous stream (see :class:`_ModulationStream`)."""


class StatefulFlanger(_ModulationStream, Flanger):
    """:class:`~torchfx_amd.effect.Flanger` over a continuous stream (see :class:`_ModulationStream`)."""


class StatefulVibrato(_ModulationStream, Vibrato):
    """:class:`~torchfx_amd.effect.Vibrato` over a continuous stream (see :class:`_ModulationStream`)."""


class StatefulPhaser(Phaser):
    """:class:`~torchfx_amd.effect.Phaser` over a continuous stream: every row carries ``(x_0[-1], .., x_N[-1])``, the last
    sample of the input and of each all-pass section, in ``_hist`` (``[rows, stages + 1]`` float64) and the stream the absolute
    position of its next sample in ``_pos`` (int64 ``[1]`` on the chunks' device: a replayed HIP graph bakes host scalars in, a
    device counter moves on with every replay).  The phaser is causal with no latency: every chunk returns the chunk's shape
    and there is nothing to flush.

    The stream restarts from silence and position 0 when the row count, ``stages`` or the device changes; :meth:`reset_state`
    does the same on request.  Any other parameter applies from the next chunk on.  The coefficient track of the chunks is
    bit-identical to the one-shot call's; the outputs equal :func:`~torchfx_amd.phaser.phase_shift` on the whole signal to
    float64 round-off and not bit for bit: the scan's association follows the cut.  After a NaN or Inf the state of its row is
    non-finite and stays so until :meth:`reset_state`.  Device float32 / float64 chunks run :func:`torchfx_ext.phaser_forward`
    (one launch for a chunk of up to 2048 samples), CPU chunks the host path."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.reset_state()

    def reset_state(self) -> None:
        self._hist: Tensor | None = None            # [rows, stages + 1] float64; None = silence
        self._pos: Tensor | None = None             # int64 [1] on the chunks' device; None = 0

    def _capture_key(self) -> tuple:
        """What a captured HIP graph of this effect bakes in: every parameter of the launch."""
        return (self.rate, self.min_freq, self.max_freq, self.stages, self.mix, self.invert, self.spread, self.shape, self.fs)

    def _sync_history(self) -> None:
        """Nothing to resize: a changed ``stages`` restarts the stream in :meth:`forward`."""

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        rows = _rows(x)
        if self.fs is None:
            raise ValueError(f"{type(self).__name__} needs the sample rate: pass fs or let the processor configure it")
        from torchfx_amd.phaser import phase_shift_run

        P = self.params(x.dtype)
        h = self._hist
        if (h is None or self._pos is None or tuple(h.shape) != (rows, P.stages + 1) or h.device != x.device
                or self._pos.device != x.device):                   # a new stream: silence, position 0
            h, self._pos = None, torch.zeros(1, dtype=torch.int64, device=x.device)
        y, _, self._hist, self._pos = phase_shift_run(x, P, 0, h, False, self._pos)
        return y


def _members(e) -> list:
    """``e`` and every module inside it."""
    return list(e.modules() if isinstance(e, nn.Module) else [e])


def _holds_back(e) -> bool:
    """Effects whose chunks may return fewer samples than they take and that hand the rest out in ``flush()``: their class says
    ``holds_back = True``."""
    return getattr(type(e), "holds_back", False)


def _held_back(members):
    """The member that holds outputs back, or None.  Of several, the one a message names: a resampler before a limiter before a
    shaper (``_hold_rank``), the first of its kind."""
    return min((m for m in members if _holds_back(m)), key=lambda m: m._hold_rank, default=None)


class _Refusal(tp.NamedTuple):
    """One family of effects that cannot run chunk by chunk.  A member that is a ``plain`` but no ``stream`` instance (and meets
    ``when``) raises ``text``, with ``{who}``, ``{name}`` (the member's class), ``{m}`` (the member) and ``{stateful}``
    (``stateful(m)``) filled in; where ``stream`` holds outputs back, an instance of it below the top level raises ``nested``.
    ``who`` names the one processor that makes the check (None: both)."""
    plain: type
    stream: type | tuple
    text: str
    when: tp.Callable | None = None
    stateful: tp.Callable | None = None
    nested: str | None = None
    who: str | None = None


_TOP_LEVEL = "{} must be a top-level effect of the chain in {{who}}: the processor flushes what it holds back at the end of the stream"
_NO_RESAMPLE = ("Resample cannot run in StreamProcessor: resampling each chunk on its own leaves a seam at every chunk boundary; use "
                "StatefulResample as a top-level effect of the chain, or resample the whole signal (Wave.resample) before or after "
                "streaming")
# in the order the refusals fire for an effect that would meet several of them
_REFUSALS = (
    _Refusal(ZeroPhase, (),
             "ZeroPhase cannot run in {who}: zero-phase filtering is non-causal -- its backward pass starts at the end of the signal, "
             "which a chunked stream has not seen yet; filter the whole signal (wave | ZeroPhase(...) or sosfiltfilt) before or after "
             "streaming"),
    _Refusal(LoudnessNormalize, (),
             "LoudnessNormalize cannot run in {who}: integrated loudness is a measurement of the whole signal (its relative gate "
             "depends on every block), which a chunked stream has not seen yet; normalise the whole signal "
             "(wave | LoudnessNormalize(...)) before or after streaming"),
    _Refusal(Limiter, StatefulLimiter,
             "Limiter cannot run in {who}: its gain looks A - 1 samples ahead (the look-ahead), which a chunked stream has not seen "
             "yet; a streaming limiter that carries that history is not provided by Limiter itself -- use StatefulLimiter(...) in its "
             "place, or limit the whole signal (wave | Limiter(...)) before or after streaming",
             nested=_TOP_LEVEL.format("StatefulLimiter")),
    _Refusal(Compressor, StatefulCompressor,
             "Compressor cannot run in {who}: every call starts its level detector from silence, so a chunked stream would drop the "
             "envelope at every chunk start; use StatefulCompressor(...) in its place, or compress the whole signal "
             "(wave | Compressor(...)) before or after streaming"),
    _Refusal(ModulatedDelay, _ModulationStream,
             "{name} cannot run in {who}: every call starts its LFO at position 0 and its delay line from silence, so a chunked stream "
             "would restart the sweep and drop the delayed samples at every chunk start; use {stateful} in its place, or run the "
             "whole signal (wave | {name}(...)) before or after streaming",
             stateful=lambda m: (f"Stateful{type(m).__name__}(...)" if isinstance(m, (Chorus, Flanger, Vibrato))
                                 else "a stateful class (StatefulChorus, StatefulFlanger, StatefulVibrato)")),
    _Refusal(Freeverb, StatefulFreeverb,
             "Freeverb cannot run in {who}: every call starts from silent delay lines, so a chunked stream would cut the room's tail "
             "at every chunk start; use StatefulFreeverb(...) in its place, or run the whole signal (wave | Freeverb(...)) before or "
             "after streaming"),
    _Refusal(Waveshaper, _ShaperStream,
             "{name} with oversample={m.oversample} cannot run in {who}: every call zero-pads the edges of its resampling filters, so "
             "a chunked stream would click at every chunk seam; use {stateful}(...) in its place, oversample=1 (memoryless), or run "
             "the whole signal (wave | {name}(...)) before or after streaming",
             when=lambda m: m.oversample != 1,
             stateful=lambda m: f"Stateful{type(m).__name__ if type(m) in (Waveshaper, Distortion) else 'Waveshaper'}",
             nested=_TOP_LEVEL.format("StatefulWaveshaper / StatefulDistortion")),
    # RealtimeProcessor has no text of its own for a plain Resample: it meets this one in the StreamProcessor it runs its blocks through
    _Refusal(Resample, StatefulResample, _NO_RESAMPLE, nested=_NO_RESAMPLE, who="StreamProcessor"),
    # new families go in here, in front of the phaser, which stays the table's last entry (tests/test_stream_phaser_host.py)
    _Refusal(Gate, StatefulGate,
             "Gate cannot run in {who}: every call starts closed with its hold counter at zero, so a chunked stream would shut the "
             "gate at every chunk start; use StatefulGate(...) in its place, or gate the whole signal (wave | Gate(...)) before or "
             "after streaming"),
    _Refusal(Phaser, StatefulPhaser,
             "Phaser cannot run in {who}: every call starts its sweep at position 0 and its all-pass sections from silence, so a "
             "chunked stream would restart the sweep and the filter states at every chunk start; use StatefulPhaser(...) in its "
             "place, or run the whole signal (wave | Phaser(...)) before or after streaming"),
)


def _check_streamable(e, who: str) -> None:
    """Raise the TypeError of the first family in ``_REFUSALS`` that ``e``, a top-level effect of ``who``'s chain, or a module
    inside it belongs to."""
    members = _members(e)
    for r in _REFUSALS:
        if r.who not in (None, who):
            continue
        for m in members:
            if isinstance(m, r.plain) and not isinstance(m, r.stream) and (r.when is None or r.when(m)):
                raise TypeError(r.text.format(who=who, name=type(m).__name__, m=m, stateful=r.stateful and r.stateful(m)))
        if getattr(r.stream, "holds_back", False) and not isinstance(e, r.stream) and any(isinstance(m, r.stream) for m in members):
            raise TypeError(r.nested.format(who=who))


class _ChunkRun:
    """``IIR ... | StatefulFIR | Gain`` (any non-empty sub-pattern of at least two effects) as ONE launch per small chunk
    (``torchfx_ext.chunk_forward``): the chain of a 2 x 512 block is launch-bound, not arithmetic-bound.  Consecutive
    IIR members run as one float64 cascade rounded to float32 once -- what the ``Wave`` planner does with them
    (``wave.py:207-239``); member by member they would round to float32 in between, so the two agree to a float32 ulp.

    The members stay the owners of their state as far as a caller can see: after every chunk each IIR member's
    ``_state_x`` / ``_state_y`` are row-block views of the combined ``[sum K, C, 2]`` tensors the kernel wrote and the FIR's
    ``_hist`` is the kernel's new history, so a member that is reset, redesigned or run on its own in between is
    picked up on the next chunk (the combined state is then rebuilt from what the members hold).  Chunks the fused
    kernel does not take (too long, float64) run member by member, exactly as before."""

    def __init__(self, iirs: list, fir, gain) -> None:
        self.iirs, self.fir, self.gain = iirs, fir, gain
        self.members = [*iirs, *([fir] if fir is not None else []), *([gain] if gain is not None else [])]
        self._sos_key = None
        self._sos = None
        self._sx = self._sy = None
        self._views: list = []
        self._one = torch.ones(1)                     # "no FIR": one unit tap
        self._geom: dict = {}

    def _table(self) -> Tensor:
        for m in self.iirs:
            if m._sos is None:
                m.compute_coefficients()
        key = tuple((id(m._sos), m._sos._version) for m in self.iirs)
        if key != self._sos_key:
            self._sos = (torch.cat([m._sos for m in self.iirs]).contiguous() if self.iirs else torch.zeros(0, 6, dtype=torch.float64))
            self._sos_key = key
            self._keep = [m._sos for m in self.iirs]             # the ids in the key stay unique
        return self._sos

    def _states(self, rows: int, device) -> tuple[Tensor | None, Tensor | None]:
        if not self.iirs:
            return None, None
        if (self._sx is not None and self._sx.shape[1] == rows and self._sx.device == device
                and len(self._views) == len(self.iirs) and all(
                    m._state_x is vx and m._state_y is vy for m, (vx, vy) in zip(self.iirs, self._views))):
            return self._sx, self._sy                           # untouched since the last chunk, same rows, same device
        # (a chunk with another channel count or on another device takes the rebuild below, which zero-fills the members
        # whose state does not fit -- what _sos_cascade_forward and the reference do, iir.py:136-138)
        if all(m._state_x is None for m in self.iirs):
            return None, None                                   # fresh: the kernel treats None as zeros
        xs, ys = [], []
        for m in self.iirs:
            k = int(m._sos.shape[0])
            ok = m._state_x is not None and m._state_y is not None and tuple(m._state_x.shape) == (k, rows, 2)
            xs.append(m._state_x.to(device) if ok else torch.zeros(k, rows, 2, dtype=torch.float64, device=device))
            ys.append(m._state_y.to(device) if ok else torch.zeros(k, rows, 2, dtype=torch.float64, device=device))
        return torch.cat(xs), torch.cat(ys)

    def fuses(self, w: Tensor) -> bool:
        """Whether this chunk goes through the one-launch kernel (geometry answers are cached: one ctypes call each)."""
        if w.dtype != torch.float32 or w.dim() != 2 or w.shape[-1] == 0:
            return False
        from torchfx_amd import torchfx_ext

        taps = self.fir.kernel.numel() if self.fir is not None else 1
        key = (w.shape[0], w.shape[1], int(self._table().shape[0]), taps)
        ok = self._geom.get(key)
        if ok is None:
            ok = self._geom[key] = torchfx_ext.chunk_supported(*key)
        return ok

    def __call__(self, w: Tensor) -> Tensor:
        from torchfx_amd import torchfx_ext

        taps = self.fir.kernel.reshape(-1) if self.fir is not None else self._one
        sos = self._table()
        if not self.fuses(w):
            for m in self.members:
                w = m(w)
            return w
        rows = w.shape[0]
        sx, sy = self._states(rows, w.device)
        hist = _carried(self.fir._hist, rows, taps.numel() - 1, w) if self.fir is not None else None
        g = self.gain.linear_gain() if self.gain is not None else None
        y, nsx, nsy, nh = torchfx_ext.chunk_forward(w, sos, sx, sy, taps, hist, g,
                                                    bool(self.gain is not None and self.gain.clamp))
        self._sx, self._sy, self._views = nsx, nsy, []
        k0 = 0
        for m in self.iirs:
            k1 = k0 + int(m._sos.shape[0])
            m._state_x, m._state_y = nsx[k0:k1], nsy[k0:k1]
            self._views.append((m._state_x, m._state_y))
            k0 = k1
        if self.fir is not None and taps.numel() > 1:
            self.fir._hist = nh
        return y


def _chunk_segments(effects: list) -> list:
    """Group the effect list into fused per-chunk runs (``_ChunkRun``) and single effects."""
    from torchfx_amd.effect import Gain
    from torchfx_amd.filter.biquad import Biquad
    from torchfx_amd.filter.iir import IIR

    out, i, n = [], 0, len(effects)
    while i < n:
        j = i
        iirs = []
        while j < n and isinstance(effects[j], (IIR, Biquad)):
            iirs.append(effects[j])
            j += 1
        fir = None
        if j < n and isinstance(effects[j], StatefulFIR) and type(effects[j]).forward is StatefulFIR.forward:
            fir = effects[j]
            j += 1
        gain = None
        if (iirs or fir is not None) and j < n and type(effects[j]) is Gain:
            gain = effects[j]
            j += 1
        if len(iirs) + (fir is not None) + (gain is not None) >= 2:
            out.append(_ChunkRun(iirs, fir, gain))
            i = j
        else:
            out.append(effects[i])
            i += 1
    return out


class StreamProcessor:
    """Run a list of effects over a long ``[C, T]`` tensor chunk by chunk."""

    def __init__(self, effects: Sequence[FX] | nn.Sequential, chunk_size: int = 65536, overlap: int = 0,
                 device: str = "cuda", use_graph: bool = False) -> None:
        if chunk_size <= 0:
            raise ValueError(f"chunk_size must be positive, got {chunk_size}")
        if overlap < 0:
            raise ValueError(f"Overlap must be non-negative, got {overlap}")
        if overlap >= chunk_size:
            raise ValueError(f"Overlap ({overlap}) must be less than chunk_size ({chunk_size})")
        self._effects = list(effects)
        for e in self._effects:
            if not isinstance(e, FX):
                raise TypeError("All effects must inherit from FX when used in StreamProcessor")
            _check_streamable(e, "StreamProcessor")
        self._resamplers = [e for e in self._effects if isinstance(e, StatefulResample)]
        held = _held_back(self._effects)
        if held is not None and overlap != 0:
            raise ValueError(f"A chain with a {type(held).__name__} needs overlap = 0, got {overlap}: the effect holds outputs back, so "
                             "a chunk's dropped overlap samples have no counterpart in its output")
        self._chunk_size, self._overlap, self._device = chunk_size, overlap, device
        self._use_graph = use_graph
        self._graph = None            # (CUDAGraph, static in, static out, stream, signature, state slots, homes)
        # small chunks: runs of IIR ... | StatefulFIR | Gain go through one fused launch (TORCHFX_AMD_FUSE_CHUNK=0: never)
        self._segments = _chunk_segments(self._effects) if os.environ.get("TORCHFX_AMD_FUSE_CHUNK", "1") != "0" else list(self._effects)

    chunk_size = property(lambda self: self._chunk_size)
    overlap = property(lambda self: self._overlap)
    effects = property(lambda self: self._effects)

    def __enter__(self) -> "StreamProcessor":
        return self

    def __exit__(self, *exc) -> None:
        return None

    def _configure_effects(self, fs: int) -> None:
        """fs propagation, redesign on change, Nyquist check (``stream.py:119-162``).  The effects are walked in order with
        a running rate: a ``StatefulResample`` gets the rate it receives and the effects after it get its ``new_fs``."""
        for e in self._effects:
            nyquist = fs / 2.0
            cutoff = getattr(e, "cutoff", None)
            if isinstance(e, AbstractFilter) and isinstance(cutoff, (int, float)) and cutoff >= nyquist:
                raise ValueError(
                    f"{type(e).__name__} cutoff ({cutoff} Hz) must be below the Nyquist frequency "
                    f"({nyquist} Hz) for sample rate {fs} Hz. Reduce the cutoff or use a higher sample rate file.")
            if hasattr(e, "fs") and e.fs != fs:
                e.fs = fs
                if isinstance(e, AbstractFilter):
                    e.compute_coefficients()
                    if callable(getattr(e, "reset_state", None)):
                        e.reset_state()
            if isinstance(e, AbstractFilter) and not e._has_computed_coeff:
                e.compute_coefficients()
            if isinstance(e, StatefulResample):
                fs = e.new_fs

    def output_rate(self, fs: int) -> int:
        """The sample rate of the chain's output for an input at ``fs``."""
        for e in self._resamplers:
            fs = e.new_fs
        return fs

    # ---- HIP-graph replay of the per-chunk step ------------------------------------------------
    _STATE_ATTRS = ("_state_x", "_state_y", "_hist", "_pos")

    def _stateful_slots(self) -> list[tuple[object, str]]:
        """(module, attribute) of every carried-state tensor reachable from the effects."""
        slots = []
        for e in self._effects:
            for m in _members(e):
                for a in self._STATE_ATTRS:
                    if isinstance(getattr(m, a, None), Tensor):
                        slots.append((m, a))
                for f in getattr(m, "filters", ()) or ():       # combinations / banks hold plain lists
                    for a in self._STATE_ATTRS:
                        if isinstance(getattr(f, a, None), Tensor):
                            slots.append((f, a))
        return slots

    def _fused(self, w: Tensor) -> bool:
        """The whole chain is one fused launch for this chunk: nothing for a HIP graph to save (one kernel node against
        the copy-in / replay / copy-out of a graph step)."""
        return len(self._segments) == 1 and isinstance(self._segments[0], _ChunkRun) and self._segments[0].fuses(w)

    def _run(self, w: Tensor, start: int = 0) -> Tensor | None:
        """The chain from segment ``start`` on; None when an effect that holds outputs back (``holds_back``) completes no output
        for this chunk (the effects after it are not called)."""
        for e in self._segments[start:]:
            w = e(w)
            if _holds_back(e) and w.shape[-1] == 0:
                return None
        return w

    def _tails(self) -> Generator[Tensor, None, None]:
        """The end of the stream: the held-back outputs of every resampler and limiter, left to right, each through the effects
        after it (so a limiter behind a resampler limits the resampler's tail before it hands out its own)."""
        for i, e in enumerate(self._segments):
            if _holds_back(e):
                t = e.flush()
                if t.dim() > 0 and t.shape[-1] > 0:
                    t = self._run(t, i + 1)
                    if t is not None:
                        yield t

    def _graphable(self, w: Tensor) -> bool:
        """Whether a replayed step leaves the host side of every effect right: a resampler counts samples per chunk (never),
        a limiter or an oversampled waveshaper only until its position counter has saturated (chunks run eagerly until then).
        Every member that has ``_graph_ready`` is asked."""
        return all(m._graph_ready(w) for e in self._effects for m in _members(e) if hasattr(m, "_graph_ready"))

    def _capture_members(self) -> list:
        """Members whose parameters a captured step bakes in and whose carried state can change length (StatefulDelay,
        StatefulReverb): they name their parameters in ``_capture_key`` and resize their history in ``_sync_history``."""
        return [m for e in self._effects for m in _members(e) if hasattr(m, "_capture_key")]

    def _graph_step(self, w: Tensor) -> Tensor:
        """Replay the captured step on ``w`` (capturing it first; the carried states must exist)."""
        members = self._capture_members()
        for m in members:                             # a parameter change since the last chunk: history at its new length
            m._sync_history()
        sig = (tuple(w.shape), w.dtype, tuple(tuple(getattr(m, a).shape) for m, a in self._stateful_slots()),
               tuple(m._capture_key() for m in members))
        if self._graph is None or self._graph[4] != sig:
            dev = w.device
            slots = self._stateful_slots()
            # persistent homes for the carried state: the captured step reads them and its last nodes
            # copy the new state back, so consecutive replays chain exactly like eager calls do
            homes = [getattr(m, a).clone() for m, a in slots]
            saved = [h.clone() for h in homes]
            static_in = w.clone()

            def rehome() -> None:
                for (m, a), h in zip(slots, homes):
                    setattr(m, a, h)

            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                rehome()
                self._run(static_in)                      # warms this stream's workspaces; not captured
                for h, s0 in zip(homes, saved):           # undo what it did to the state
                    h.copy_(s0)
                rehome()
                graph = torch.cuda.CUDAGraph()
                # No cyclic collection may fall into the capture: a dead cycle can hold an earlier processor's CUDAGraph and
                # its pool (a RealtimeProcessor and its backend refer to each other), and destroying those while a stream
                # captures aborts the process.  torch.cuda.graph no longer collects on entry, so collect here, then hold the
                # collector off until the capture has ended.
                gc.collect()
                gc_was_on = gc.isenabled()
                gc.disable()
                try:
                    with torch.cuda.graph(graph, stream=side):
                        static_out = self._run(static_in)
                        for (m, a), h in zip(slots, homes):
                            new = getattr(m, a)
                            if new is not h:
                                h.copy_(new)
                        rehome()
                finally:
                    if gc_was_on:
                        gc.enable()
            torch.cuda.current_stream(dev).wait_stream(side)
            self._graph = (graph, static_in, static_out, side, sig, slots, homes)
        graph, static_in, static_out, _, _, slots, homes = self._graph
        for (m, a), h in zip(slots, homes):           # an eager step in between left the state elsewhere
            cur = getattr(m, a)
            if cur is not h:
                h.copy_(cur)
                setattr(m, a, h)
        static_in.copy_(w)
        graph.replay()
        return static_out.clone()

    def _steps(self, chunks) -> Generator[Tensor, None, None]:
        """The chain over ``(offset, device chunk)`` pairs, then the resamplers' tails; with overlap the first ``overlap``
        samples of every chunk but the first are dropped (``stream.py:327-331``)."""
        primed = False
        for offset, w in chunks:
            if (self._use_graph and primed and w.is_cuda and w.shape[-1] == self._chunk_size and not self._fused(w)
                    and self._graphable(w)):
                w = self._graph_step(w)
            else:
                w = self._run(w)            # first chunk creates the states; ragged tail runs eagerly
                primed = True
            if w is not None:
                yield w[..., self._overlap:] if (self._overlap > 0 and offset > 0) else w
        yield from self._tails()

    @torch.no_grad()
    def process_chunks(self, x: Tensor, fs: int) -> Generator[Tensor, None, None]:
        """Yield processed chunks of ``x`` (see :meth:`_steps`)."""
        self._configure_effects(fs)
        hop = self._chunk_size - self._overlap
        yield from self._steps((o, x[..., o:o + self._chunk_size].to(self._device)) for o in range(0, x.shape[-1], hop))

    @torch.no_grad()
    def process_tensor(self, x: Tensor, fs: int) -> Tensor:
        """The whole processed signal; after a ``StatefulResample`` at the chain's output rate (:meth:`output_rate`)."""
        return torch.cat(list(self.process_chunks(x, fs)), dim=-1)

    # ---- files (``stream.py:164-347``) -------------------------------------------------------------
    def _file_chunks(self, input_path) -> Generator[tuple[int, Tensor], None, None]:
        """Decode ``chunk_size`` frames at a time and yield ``(offset, planar [C, n] chunk on the device)``."""
        import soundfile as sf

        from torchfx_amd import io as _io

        info = sf.info(str(input_path))
        self._configure_effects(info.samplerate)
        on_gpu = torch.device(self._device).type == "cuda"
        for offset in range(0, info.frames, self._chunk_size - self._overlap):
            n = min(self._chunk_size, info.frames - offset)
            frames, _ = sf.read(str(input_path), start=offset, stop=offset + n, dtype="float32", always_2d=True)
            # interleaved [n, C] -> planar [C, n] on the device (reference: data_np.T.copy() on the host)
            yield offset, (_io.upload_interleaved(frames, self._device) if on_gpu else torch.from_numpy(frames.T.copy()))

    @torch.no_grad()
    def process_file_chunks(self, input_path) -> Generator[Tensor, None, None]:
        """Generator over processed chunks of a file, as host tensors ``[channels, frames]`` like the
        reference's ``process_chunks(path)`` (``stream.py:278-347``)."""
        for w in self._steps(self._file_chunks(input_path)):
            yield w.cpu()

    @torch.no_grad()
    def process_file(self, input_path, output_path, format: str | None = None,  # noqa: A002
                     subtype: str | None = None) -> None:
        """Process an audio file chunk by chunk into ``output_path`` (``stream.py:164-276``): output format
        from the extension (WAV when unknown), subtype FLOAT for WAV unless given, parent directories
        created.  Chunks travel interleaved in both directions; the transposes run on the GPU.  The file is written at
        the chain's output rate (:meth:`output_rate`)."""
        import pathlib

        import soundfile as sf

        from torchfx_amd import io as _io

        out = pathlib.Path(output_path)
        out.parent.mkdir(parents=True, exist_ok=True)
        info = sf.info(str(input_path))
        if format is None:
            format = {".wav": "WAV", ".flac": "FLAC", ".ogg": "OGG"}.get(out.suffix.lower(), "WAV")  # noqa: A001
        if subtype is None:
            subtype = "FLOAT" if format == "WAV" else None
        with sf.SoundFile(str(out), mode="w", samplerate=self.output_rate(info.samplerate), channels=info.channels, format=format,
                          subtype=subtype) as sink:
            hostbuf = None                                            # one host buffer for every chunk on its way out
            for w in self._steps(self._file_chunks(input_path)):
                if w.is_cuda and w.dim() == 2 and w.dtype == torch.float32:
                    if hostbuf is None or hostbuf.shape[0] < w.shape[1] or hostbuf.shape[1] != w.shape[0]:
                        import numpy as np
                        hostbuf = np.empty((max(self._chunk_size, w.shape[1]), w.shape[0]), dtype=np.float32)
                    sink.write(_io.download_interleaved(w, out=hostbuf))   # [n, C], interleaved on the device
                else:
                    sink.write(w.cpu().numpy().T)


# ---------------------------------------------------------------------------------------------------
# The sound-card side of the same hot path: RealtimeProcessor (``src/torchfx/realtime/processor.py:46-325``)
# ---------------------------------------------------------------------------------------------------
class RealtimeError(RuntimeError):
    """``realtime/exceptions.py``: message plus an optional suggestion."""

    def __init__(self, message: str, suggestion: str | None = None) -> None:
        self.suggestion = suggestion
        super().__init__(message if suggestion is None else f"{message} ({suggestion})")


class StreamDirection(enum.Enum):
    INPUT = "input"
    OUTPUT = "output"
    DUPLEX = "duplex"


@dataclasses.dataclass(frozen=True)
class StreamConfig:
    """``realtime/backend.py:67-137``: the stream a backend opens."""

    sample_rate: int = 48000
    buffer_size: int = 512
    channels_in: int = 0
    channels_out: int = 2
    dtype: str = "float32"
    device_in: int | str | None = None
    device_out: int | str | None = None
    latency: str | float = "low"

    @property
    def direction(self) -> StreamDirection:
        if self.channels_in > 0 and self.channels_out > 0:
            return StreamDirection.DUPLEX
        return StreamDirection.INPUT if self.channels_in > 0 else StreamDirection.OUTPUT

    @property
    def latency_ms(self) -> float:
        return self.buffer_size / self.sample_rate * 1000.0


class AudioBackend(abc.ABC):
    """What the processor needs from an audio I/O backend (``realtime/backend.py:140-268``, reduced to the four calls
    the processor makes).  A backend calls ``callback(input [channels_in, frames], output [channels_out, frames],
    frames)`` once per buffer; the sound-device backends themselves are out of scope here."""

    @abc.abstractmethod
    def open_stream(self, config: StreamConfig, callback=None) -> None: ...

    @abc.abstractmethod
    def start(self) -> None: ...

    @abc.abstractmethod
    def stop(self) -> None: ...

    @abc.abstractmethod
    def close(self) -> None: ...


class RealtimeProcessor:
    """A backend's per-buffer callback run through the effect chain on the GPU.

    Same surface as the reference's ``RealtimeProcessor`` (construction, ``start`` / ``stop`` / context manager,
    ``set_parameter`` staged until the next buffer boundary, ``reset_state``, ``latency_ms``).  The callback is where the
    device comes in: the host block goes through a pinned staging buffer to a persistent device buffer on the
    processor's own stream, the chain runs there -- from the second full-size block on as ONE replayed HIP graph when
    ``use_graph`` (a 512-sample block is launch-bound: tens of microseconds of launches for a few of GPU work) --
    and the result comes back through a second pinned buffer; the only host wait is the one before the block is
    handed back.  Device tensors are processed in place of the staging.  The carried IIR states / FIR histories make
    consecutive callbacks one continuous signal.
    """

    def __init__(self, effects: Sequence[FX] | nn.Sequential, backend: AudioBackend, config: StreamConfig,
                 buffer_capacity: int = 8192, device: str = "cuda", use_graph: bool = False) -> None:
        if not isinstance(config.sample_rate, int) or config.sample_rate <= 0:
            raise ValueError(f"sample_rate must be a positive integer, got {config.sample_rate!r}")
        if config.buffer_size <= 0:
            raise ValueError(f"buffer_size must be positive, got {config.buffer_size}")
        modules = list(effects)
        for e in modules:
            if not isinstance(e, FX):
                raise TypeError("All effects must inherit from FX when used in RealtimeProcessor")
            _check_streamable(e, "RealtimeProcessor")
            if any(isinstance(m, StatefulResample) for m in _members(e)):
                raise TypeError("StatefulResample cannot run in RealtimeProcessor: a sound card's output block has the input "
                                "block's length and sample rate; resample with StreamProcessor or Wave.resample instead")
            if _holds_back(e) and e.aligned:
                raise TypeError(e._aligned_refusal.format(name=type(e).__name__))
        self._runner = StreamProcessor(modules, chunk_size=config.buffer_size, overlap=0, device=device, use_graph=use_graph)
        self._backend, self._config, self._running = backend, config, False
        self._buffer_capacity = buffer_capacity
        for e in modules:                                      # same pattern as Wave.__or__
            if hasattr(e, "fs") and e.fs is None:
                e.fs = config.sample_rate
            if isinstance(e, AbstractFilter) and not e._has_computed_coeff:
                e.compute_coefficients()
        self._pending: dict[str, object] = {}
        self._param_lock = threading.Lock()
        self._primed = False
        self._stage = None           # (pinned in, device in, pinned out, stream) for the current block geometry

    # ---- life cycle ----------------------------------------------------------------------------------
    def __enter__(self) -> "RealtimeProcessor":
        self.start()
        return self

    def __exit__(self, *exc) -> None:
        if self._running:
            self.stop()

    def start(self) -> None:
        if self._running:
            raise RealtimeError("Processor is already running", suggestion="Call stop() before starting again")
        self._backend.open_stream(self._config, callback=self._audio_callback)
        self._backend.start()
        self._running = True

    def stop(self) -> None:
        if not self._running:
            raise RealtimeError("Processor is not running", suggestion="Call start() first")
        self._running = False
        self._backend.stop()
        self._backend.close()

    # ---- parameters: staged by any thread, applied at the next buffer boundary ---------------------
    def set_parameter(self, name: str, value) -> None:
        with self._param_lock:
            self._pending[name] = value

    def _apply_pending_params(self) -> None:
        if not self._pending:
            return
        with self._param_lock:
            params, self._pending = self._pending, {}
        effects = self._runner.effects
        for key, value in params.items():
            idx, _, attr = key.partition(".")
            i = int(idx)
            if not (0 <= i < len(effects)) or not attr:
                continue                                            # the reference logs a warning and goes on
            e = effects[i]
            setattr(e, attr, value)
            if isinstance(e, AbstractFilter):                       # redesign, start from silence
                e.compute_coefficients()
                if callable(getattr(e, "reset_state", None)):
                    e.reset_state()
                self._primed = False                                # the captured step holds the old tables / states
                self._runner._graph = None
            elif self._runner._graph is not None:                   # a scalar baked into captured kernels (Gain, ...)
                self._runner._graph = None

    # ---- the callback --------------------------------------------------------------------------------
    def _staging(self, rows: int, frames: int, rows_out: int, dev: torch.device):
        key = (rows, frames, rows_out, str(dev))
        if self._stage is None or self._stage[0] != key:
            self._stage = (key, torch.empty(rows, frames, dtype=torch.float32).pin_memory(),
                           torch.empty(rows, frames, dtype=torch.float32, device=dev),
                           torch.empty(rows_out, frames, dtype=torch.float32).pin_memory(), torch.cuda.Stream(dev))
        return self._stage[1:]

    def _chain(self, w: Tensor) -> Tensor:
        full = w.shape[-1] == self._config.buffer_size
        if (self._runner._use_graph and w.is_cuda and full and self._primed and not self._runner._fused(w)
                and self._runner._graphable(w)):
            return self._runner._graph_step(w)
        y = self._runner._run(w)             # the first block creates the carried states; ragged blocks run eagerly
        self._primed = self._primed or full
        return y

    @staticmethod
    def _fit_channels(y: Tensor, rows_out: int) -> Tensor:
        if y.shape[0] == rows_out:
            return y
        if y.shape[0] == 1 and rows_out > 1:                          # mono to every output channel
            return y.expand(rows_out, -1)
        return y[:rows_out]                                           # else truncate (processor.py:283-291)

    @torch.no_grad()
    def _audio_callback(self, input_data: Tensor, output_data: Tensor, frame_count: int) -> None:  # noqa: ARG002
        self._apply_pending_params()
        on_gpu = torch.device(self._runner._device).type == "cuda"
        if not on_gpu or input_data.is_cuda:                          # host-only mirror / device tensors: no staging
            y = self._chain(input_data if input_data.is_cuda or not on_gpu else input_data.to(self._runner._device))
            if output_data.numel() > 0:
                output_data.copy_(self._fit_channels(y, output_data.shape[0]))
            return
        dev = torch.device(self._runner._device)
        rows_out = output_data.shape[0] if output_data.numel() > 0 else input_data.shape[0]
        pin_in, dev_in, pin_out, stream = self._staging(input_data.shape[0], input_data.shape[-1], rows_out, dev)
        pin_in.copy_(input_data)
        with torch.cuda.stream(stream):
            dev_in.copy_(pin_in, non_blocking=True)
            y = self._fit_channels(self._chain(dev_in), rows_out)
            if output_data.numel() > 0:
                pin_out.copy_(y, non_blocking=True)
        stream.synchronize()                                          # the block is due now
        if output_data.numel() > 0:
            output_data.copy_(pin_out)

    # ---- the rest of the surface -------------------------------------------------------------------
    def reset_state(self) -> None:
        for e in self._runner.effects:
            if callable(getattr(e, "reset_state", None)):
                e.reset_state()
        self._primed = False

    latency_ms = property(lambda self: self._config.latency_ms)

    @property
    def chain_latency_samples(self) -> int:
        """The delay the effects add on top of the buffer's: the sum of their ``latency`` (``StatefulLimiter``'s and
        ``StatefulWaveshaper``'s ``D``)."""
        return sum(int(getattr(e, "latency", 0) or 0) for e in self._runner.effects)

    is_running = property(lambda self: self._running)
    effects = property(lambda self: self._runner.effects)
    config = property(lambda self: self._config)
