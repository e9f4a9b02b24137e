"""Python face of the native module: the reference's ``torchfx.torchfx_ext`` names plus our extra ops.

The three entry points of the reference's pybind module (``src/torchfx/_csrc/binding.cpp:83-96``:
``biquad_forward``, ``sos_forward``, ``delay_line_forward``) and the ops the reference implements with
torch library calls (``F.conv1d`` / ``torch.fft``) and we implement in HIP (``fir_direct_forward``,
``fft_conv_forward``, the filter-bank / sum forms, Gain / Normalize, the layout kernels).  Every tensor
call goes through the PyTorch dispatcher to the compiled extension (``torch.ops.torchfx_hip.*``,
``torchfx_amd/csrc/ext/torchfx_ext.cpp``), which calls the C ABI of ``libtorchfx_hip.so``
(``include/torchfx_hip.h``); the functions here only add keyword conveniences (``out_dtype``,
``precision``) and keep a host copy of FIR taps.  ``ctypes`` (``torchfx_amd._lib``) is used for the
host-only planning queries at the bottom, which take no tensors.

Differences a caller can observe, all deliberate:
  * tensors must be on a ROCm device -- there is no CPU path here;
  * ``x`` may be float32 *or* float64 (the reference's CUDA kernels need float64 and its Python layer
    upcasts, ``_ops.py:95,149``); by default the result has the dtype of ``x``.  The recurrences run in
    float64 unless ``precision`` says otherwise, so a float32-in/float32-out call equals "upcast,
    filter, downcast" with 8 B/sample of traffic instead of 32;
  * kernels are launched on PyTorch's *current* stream (the reference uses the default stream,
    ``parallel_scan.cu:299``).
"""
from __future__ import annotations

import ctypes
import weakref

import numpy as np
import torch
from torch import Tensor

from torchfx_amd import _lib as L
from torchfx_amd import native

__all__ = [
    "biquad_forward", "sos_forward", "sos_bank_forward", "sos_bank_sum_forward", "delay_line_forward", "delay_forward",
    "delay_amplitudes", "delay_regime", "delay_tiling_info", "delay_stream_forward", "delay_line_stream_forward", "resample_forward",
    "resample_plan_info", "resample_tiling_info", "resample_stream_forward", "resample_stream_plan_info", "sos_filtfilt", "sos_filtfilt_plan_info",
    "sos_block_energy", "sos_block_energy_plan_info", "true_peak", "true_peak_plan_info", "limiter_forward", "limiter_plan_info",
    "limiter_stream_forward", "limiter_stream_plan_info", "compressor_forward", "compressor_plan_info",
    "modulated_delay_forward", "modulated_delay_stream_forward", "modulated_delay_plan_info", "freeverb_forward", "freeverb_plan_info",
    "waveshaper_stream_forward", "waveshaper_stream_plan_info", "phaser_forward", "phaser_plan_info", "gate_forward", "gate_plan_info",
    "stft_forward", "stft_plan_info", "istft_forward", "istft_plan_info",
    "fir_direct_forward", "fft_conv_forward", "sos_fft_conv_forward", "sos_fft_conv_supported", "sos_fft_conv_warmup", "sos_fft_conv_plan_info", "workspace_bytes", "clear_caches", "env_reload", "fir_stream_forward", "chunk_forward", "chunk_supported", "normalize_apply", "Epilogue", "sum_forward", "gain_forward", "quantile_abs", "stat_forward", "normalize_forward",
    "effects_plan_info", "deinterleave_forward", "interleave_forward", "sos_plan_info", "sos_route_info", "ols_plan_info", "prewarm",
]


class Epilogue:
    """What the producing kernel does to the samples it stores (``include/torchfx_hip.h``, ``tfx_epilogue``):
    ``gain`` (linear factor) and ``clamp`` = a following ``Gain``; ``stat`` ("absmax" | "sumsq" | None, optionally
    ``per_row``) = the reduction half of a following ``Normalize``.  After the call ``stat_value`` holds the raw
    statistic on the device (float64 ``[rows]`` or ``[1]``) for :func:`normalize_apply`."""

    __slots__ = ("gain", "clamp", "stat", "per_row", "stat_value")

    def __init__(self, gain: float = 1.0, clamp: bool = False, stat: str | None = None, per_row: bool = False) -> None:
        if stat not in (None, "absmax", "sumsq"):
            raise ValueError(f"stat must be None, 'absmax' or 'sumsq', got {stat!r}")
        self.gain, self.clamp, self.stat, self.per_row = float(gain), bool(clamp), stat, bool(per_row)
        self.stat_value: Tensor | None = None

    @property
    def stat_mode(self) -> int:
        return {None: -1, "absmax": 0, "sumsq": 1}[self.stat]


def _prec(precision) -> int:
    return -1 if precision is None else L.precision_code(precision)


def _coeff(t) -> Tensor:
    """Coefficient arrays (numpy / lists / tensors) as a host float64 tensor."""
    if isinstance(t, Tensor):
        return t
    return torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))


def _dt(dtype: torch.dtype) -> int:
    """The C ABI's dtype code (``TFX_F32`` / ``TFX_F64``)."""
    return L.TFX_F64 if dtype == torch.float64 else L.TFX_F32


_OUT_KINDS = {"int64": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double, "double4": ctypes.c_double * 4}


def _query(fn, args, outs: str) -> dict:
    """One host-only planning query of the C ABI: ``fn(*args, *pointers)`` with one output pointer per word of ``outs``
    (``name``: an int64, or ``name:kind`` with a kind of ``_OUT_KINDS`` -- ``int`` for kernel codes and segment counts),
    checked with ``L.check``.  Returns ``{name: value}`` in that order."""
    names = [w.partition(":") for w in outs.split()]
    vals = [_OUT_KINDS[kind or "int64"]() for _, _, kind in names]
    L.check(fn(*args, *[v if isinstance(v, ctypes.Array) else ctypes.byref(v) for v in vals]))
    return {name: (list(v) if isinstance(v, ctypes.Array) else v.value) for (name, _, _), v in zip(names, vals)}


def sos_forward(x: Tensor, sos: Tensor | None, sos_cpu: Tensor | None, state_x: Tensor | None,
                state_y: Tensor | None, *, out_dtype: torch.dtype | None = None,
                precision=None, return_sections: bool = False, epilogue: Epilogue | None = None):
    """SOS cascade forward -- ``binding.cpp:52-66``.

    ``x [C,T]``, ``sos [K,6]`` (device copy, unused here), ``sos_cpu [K,6]`` host float64 (the reference's
    sync-avoidance argument; falls back to ``sos``), states ``[K,C,2]`` float64 or ``None`` (= zeros).
    Returns ``(y [C,T], new_state_x, new_state_y)`` (+ every section's output ``[K,C,T]`` with
    ``return_sections``); inputs are never modified."""
    ops = native.ops()
    coeff = _coeff(sos_cpu if sos_cpu is not None else sos)
    if epilogue is not None:
        if return_sections:
            raise RuntimeError("sos_forward: no epilogue together with section taps")
        y, nsx, nsy, epilogue.stat_value = ops.sos_forward_ep(
            x, coeff, state_x, state_y, epilogue.gain, epilogue.clamp, epilogue.stat_mode, epilogue.per_row,
            out_dtype=out_dtype, precision=_prec(precision))
        return y, nsx, nsy
    if return_sections:
        return ops.sos_forward_sections(x, coeff, state_x, state_y, out_dtype=out_dtype, precision=_prec(precision))
    return ops.sos_forward(x, coeff, state_x, state_y, out_dtype=out_dtype, precision=_prec(precision))


def sos_bank_forward(x: Tensor, sos_banks, state_x: Tensor | None, state_y: Tensor | None, *,
                     out_dtype: torch.dtype | None = None, precision=None):
    """Filter bank: ``sos_banks [NB,K,6]`` (host), ``x [C,T]`` -> ``y [NB,C,T]`` in one launch; states
    ``[K, NB*C, 2]`` (band-major rows) or ``None``.  Replaces the Python loop of ``LogFilterBank.forward``
    (``filterbank.py:157-185``)."""
    return native.ops().sos_bank_forward(x, _coeff(sos_banks), state_x, state_y, out_dtype=out_dtype,
                                         precision=_prec(precision))


def sos_bank_sum_forward(x: Tensor, sos_banks, state_x: Tensor | None, state_y: Tensor | None, *, precision=None):
    """``f1 + f2 + ...`` of IIR branches in one launch: ``sos_banks [NB,K,6]`` (host), ``x [C,T]`` ->
    ``y [C,T] = sum_b cascade_b(x)`` with the reference's accumulation order and rounding
    (``__base.py:1019-1026``); states ``[K, NB*C, 2]`` (band-major rows) or ``None``."""
    return native.ops().sos_bank_sum_forward(x, _coeff(sos_banks), state_x, state_y, precision=_prec(precision))


def biquad_forward(x: Tensor, b: Tensor, a1: float, a2: float, state_x: Tensor | None,
                   state_y: Tensor | None, *, out_dtype: torch.dtype | None = None, precision=None):
    """Single biquad forward -- ``binding.cpp:30-50``: ``b [3]`` tensor, ``a1``/``a2`` Python floats, states
    ``[C,2]``.  Returns ``(y, new_state_x, new_state_y)``."""
    return native.ops().biquad_forward(x, _coeff(b), float(a1), float(a2), state_x, state_y, out_dtype=out_dtype,
                                       precision=_prec(precision))


def delay_line_forward(x: Tensor, delay_samples: int, decay: float, mix: float) -> Tensor:
    """``binding.cpp:68-81`` / ``delay_cpu.cpp:43-85``.  Like the reference, returns the input tensor itself
    when the signal is not longer than the delay."""
    return native.ops().delay_line_forward(x, int(delay_samples), float(decay), float(mix))


def delay_amplitudes(taps: int, feedback: float) -> list[float]:
    """The tap gains of the reference's delay strategies (``effect.py:1118-1121``): 1.0, then ``feedback ** (i - 1)`` as
    Python computes it."""
    return [1.0 if i == 1 else float(feedback ** (i - 1)) for i in range(1, int(taps) + 1)]


def delay_forward(x: Tensor, delay_samples: int, taps: int, feedback: float, mix: float, pingpong: bool = False,
                  epilogue: Epilogue | None = None) -> Tensor:
    """The BPM-synced multi-tap ``Delay`` in one launch: ``torch.lerp(pad(x), strategy.apply_delay(x, D, taps, feedback),
    mix)`` of ``effect.py:1447-1538`` with the mono or (``pingpong`` and ``x.size(-2) == 2``) ping-pong strategy.
    ``x [..., T]`` -> ``[..., T + taps * delay_samples]``, bit-identical to that composition on the device."""
    amps = delay_amplitudes(taps, feedback)
    if epilogue is not None:
        y, epilogue.stat_value = native.ops().delay_forward_ep(x, int(delay_samples), amps, float(mix), bool(pingpong), epilogue.gain,
                                                               epilogue.clamp, epilogue.stat_mode, epilogue.per_row)
        return y
    return native.ops().delay_forward(x, int(delay_samples), amps, float(mix), bool(pingpong))


DELAY_REGIMES = ("span", "lattice", "gather")


def delay_stream_forward(x: Tensor, hist: Tensor | None, delay_samples: int, taps: int, feedback: float, mix: float,
                         pingpong: bool = False) -> tuple[Tensor, Tensor]:
    """One chunk of a streaming ``Delay`` in one launch: ``x [..., T]`` continues the last ``H = taps * delay_samples`` input
    samples of every row (``hist [rows, H]``, None = silence).  Returns ``(y [..., T], new history [rows, H])``; the chunks'
    outputs followed by those of ``H`` zero samples are bit-identical to :func:`delay_forward` on the whole signal."""
    return native.ops().delay_stream_forward(x, hist, int(delay_samples), delay_amplitudes(taps, feedback), float(mix),
                                             bool(pingpong))


def delay_line_stream_forward(x: Tensor, hist: Tensor | None, delay_samples: int, decay: float,
                              mix: float) -> tuple[Tensor, Tensor]:
    """One chunk of :func:`delay_line_forward` over a continuous stream: the ``delay_samples`` samples of every row before
    ``x [..., T]`` come from ``hist [rows, delay_samples]`` (None = silence).  Returns ``(y [..., T], new history)``."""
    return native.ops().delay_line_stream_forward(x, hist, int(delay_samples), float(decay), float(mix))


def delay_regime(delay_samples: int, taps: int, dtype: torch.dtype = torch.float32, pingpong: bool = False) -> str:
    """Which kernel :func:`delay_forward` runs (``tfx_delay_plan_info``; host-only): "span" (the taps' span staged in LDS),
    "lattice" (long delay, residue classes with the last taps in registers) or "gather"."""
    q = _query(L.load().tfx_delay_plan_info, (int(delay_samples), int(taps), _dt(dtype), int(bool(pingpong))), "regime:int")
    return DELAY_REGIMES[q["regime"]]


def delay_tiling_info(rows: int, length: int, delay_samples: int, taps: int, dtype: torch.dtype = torch.float32,
                      pingpong: bool = False) -> dict:
    """The workgroup geometry of :func:`delay_forward` on ``[rows, length]`` (``tfx_delay_tiling_info``; host-only, the launch's
    own plan): ``regime``, ``units`` (rows, or pairs / rows of a span or lattice launch), ``tiles`` (1024-sample output tiles
    per row; lattice: blocks of 256 residues), ``kc`` steps per chunk and ``nchunks`` chunks (lattice; else 0), ``groups``
    workgroups per unit, ``nwg`` in the grid and ``lds_bytes`` per workgroup."""
    q = _query(L.load().tfx_delay_tiling_info,
               (int(rows), int(length), int(delay_samples), int(taps), _dt(dtype), int(bool(pingpong))),
               "regime:int units tiles kc nchunks groups nwg lds_bytes")
    q["regime"] = DELAY_REGIMES[q["regime"]]
    return q


def resample_forward(x: Tensor, up: int, down: int, h: Tensor) -> Tensor:
    """``scipy.signal.resample_poly(x, up, down, axis=-1, padtype="constant")`` with the filter ``h`` (a 1-D host tensor in
    ``x``'s dtype, already scaled by ``up``) in one launch: ``x [..., T]`` -> ``[..., ceil(T * up / down)]``."""
    return native.ops().resample_forward(x.contiguous(), int(up), int(down), h)


RESAMPLE_KERNELS = ("resample_reg_kernel", "resample_lds_kernel", "resample_gather_kernel", "copy")


def resample_plan_info(length: int, up: int, down: int, taps: int, dtype: torch.dtype = torch.float32) -> dict:
    """What :func:`resample_forward` does for rows of ``length`` samples and a filter of ``taps`` taps (``tfx_resample_plan_info``;
    host-only): ``n_out``, ``n_pre_remove``, ``padded`` (the filter length with SciPy's zero padding), ``Lp`` (taps per
    phase), ``kernel`` and ``lds_bytes`` per workgroup."""
    q = _query(L.load().tfx_resample_plan_info, (int(length), int(up), int(down), int(taps), _dt(dtype)),
               "n_out n_pre_remove padded Lp kernel:int lds_bytes")
    q["kernel"] = RESAMPLE_KERNELS[q["kernel"]]
    return q


def resample_tiling_info(length: int, up: int, down: int, taps: int, dtype: torch.dtype = torch.float32) -> dict:
    """The workgroup geometry of that launch (``tfx_resample_tiling_info``; host-only, same checks): ``kernel``, ``G`` phase
    groups of ``up`` threads and ``G_initial`` (before the halving that makes a tile's window fit in LDS), ``E`` outputs per
    thread, ``tile_out = up * G * E`` outputs per workgroup, ``span`` (inputs in a tile's window; 0 for the gather kernel),
    ``LP`` (taps per phase a thread runs: ``Lp`` rounded up to a register bucket for the reg kernel) and ``tiles`` per row."""
    q = _query(L.load().tfx_resample_tiling_info, (int(length), int(up), int(down), int(taps), _dt(dtype)),
               "kernel:int G G_initial E tile_out span LP tiles")
    q["kernel"] = RESAMPLE_KERNELS[q["kernel"]]
    return q


def resample_stream_forward(x: Tensor, h: Tensor, hist: Tensor | None, up: int, down: int,
                            consumed: int) -> tuple[Tensor, Tensor]:
    """One chunk of a resampling stream in one launch: ``x [..., T]`` follows ``consumed`` input samples per row, whose last
    ``H`` are ``hist [rows, H]`` (None = silence).  Returns ``(y [..., M(consumed + T) - M(consumed)], new history [rows, H])``
    with ``M(N) = max(0, ceil(N * up / down) - n_pre_remove)``: the outputs of :func:`resample_forward` on the whole signal
    that these inputs complete (``tfx_resample_stream_forward``)."""
    return native.ops().resample_stream_forward(x.contiguous(), h, hist, int(up), int(down), int(consumed))


PADTYPES = {"odd": 0, "even": 1, "constant": 2, None: 3}           # enum tfx_padtype


def sos_array(sos) -> np.ndarray:
    """``sos`` (tensor / array / nested list) as a host float64 ``[K, 6]`` array."""
    a = sos.detach().cpu().numpy() if isinstance(sos, Tensor) else np.asarray(sos)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError(f"sos array must be shape (n_sections, 6), got {a.shape}")
    return a


def sos_filtfilt(x: Tensor, sos, padtype="odd", padlen: int | None = None) -> Tensor:
    """``scipy.signal.sosfiltfilt(sos, x, axis=-1, padtype=padtype, padlen=padlen)`` on a device tensor ``x [..., T]``
    (float32 / float64; the result has its dtype): two cascade launches around one float64 intermediate
    (``tfx_sos_filtfilt_forward``).  ``sos [K,6]`` on the host; ``padlen`` None = SciPy's default."""
    return native.ops().sos_filtfilt(x.contiguous(), _coeff(sos), PADTYPES[padtype], -1 if padlen is None else int(padlen))


def sos_filtfilt_plan_info(sos, rows: int, length: int, padtype="odd", padlen: int | None = None) -> dict:
    """What :func:`sos_filtfilt` does for ``rows`` rows of ``length`` samples (``tfx_sos_filtfilt_plan_info``; host-only, same
    argument checks): ``default_padlen`` (SciPy's), ``padlen`` in force, ``work_elems`` (float64 elements of the
    intermediate), ``warmup`` (halo of a time segment, -1 = one segment per row) and the segments per row of the two passes,
    ``nseg_forward`` / ``nseg_reverse``."""
    a = sos_array(sos)
    return _query(L.load().tfx_sos_filtfilt_plan_info,
                  (int(rows), int(length), a.ctypes.data, a.shape[0], PADTYPES[padtype], -1 if padlen is None else int(padlen)),
                  "default_padlen padlen work_elems warmup nseg_forward:int nseg_reverse:int")


def sos_block_energy(x: Tensor, sos, num: int, den: int = 1) -> Tensor:
    """The cascade and the energy of its output per block of samples in one launch (``tfx_sos_block_energy_forward``); the
    filtered signal is never stored.  ``x [..., T]`` on the device (float32 / float64, contiguous rows), ``sos [K,6]`` on the
    host, used from zero state in float64 -> float64 ``[..., nblk]`` with ``S[r, i] = sum(y[r, e_i : e_(i+1)] ** 2)``,
    ``e_i = (i * num) // den``, ``nblk = (T * den) // num`` (possibly 0); ``num / den >= 64``."""
    return native.ops().sos_block_energy(x.contiguous(), _coeff(sos), int(num), int(den))


def sos_block_energy_plan_info(sos, rows: int, length: int, num: int, den: int = 1) -> dict:
    """What :func:`sos_block_energy` does for ``rows`` rows of ``length`` samples (``tfx_sos_block_energy_plan_info``;
    host-only, same argument checks): ``nblk`` blocks per row, ``nseg`` time segments per row and ``warm``, the halo of a
    segment (0 with one segment).  The cut depends on ``length``, the cascade and ``num / den`` alone."""
    a = sos_array(sos)
    return _query(L.load().tfx_sos_block_energy_plan_info, (int(rows), int(length), a.ctypes.data, a.shape[0], int(num), int(den)),
                  "nblk nseg:int warm")


def true_peak(x: Tensor, taps: Tensor, up: int) -> Tensor:
    """The linear true peak per row in two launches (``tfx_true_peak_forward``): ``max |resample_forward(x, up, 1, taps)|``
    over the last axis, bit for bit on finite rows, without storing the up-sampled signal.  ``x [..., T]`` on the device
    (float32 / float64) -> ``[...]`` of its dtype; ``taps`` a 1-D host tensor in ``x``'s dtype, already scaled by ``up``
    (2, 4 or 8), at most ``64 * up`` long.  A row with a NaN sample reads NaN."""
    return native.ops().true_peak(x.contiguous(), taps, int(up))


def true_peak_plan_info(rows: int, length: int, up: int, taps: int, dtype: torch.dtype = torch.float32) -> dict:
    """What :func:`true_peak` does for ``rows`` rows of ``length`` samples and a filter of ``taps`` taps
    (``tfx_true_peak_plan_info``; host-only, same argument checks): ``Lp`` (taps per phase), ``tile_in`` (input positions per
    workgroup), ``tiles`` per row and ``work_elems`` (the per-tile maxima).  The tiling does not depend on ``rows``."""
    return _query(L.load().tfx_true_peak_plan_info, (int(rows), int(length), int(up), int(taps), _dt(dtype)),
                  "Lp tile_in tiles work_elems")


def limiter_forward(x: Tensor, c: float, A: int, H: int, window: Tensor, up: int = 1, taps: Tensor | None = None,
                    channels: int = 1, return_gain: bool = False) -> tuple[Tensor, Tensor]:
    """The look-ahead limiter in one launch (``tfx_limiter_forward``; the definition is :func:`torchfx_amd.limiter.limit`'s), in
    samples: ``x [..., T]`` on the device (float32 / float64), its rows in groups of ``channels`` consecutive rows that share
    one gain curve; ``c`` the linear ceiling already rounded to ``x``'s dtype, ``A <= 512`` look-ahead and ``H <= 4096`` hold
    samples, ``window`` the ``A`` smoothing weights and ``taps`` the interpolator (``up`` 2, 4 or 8; None for ``up == 1``) as
    1-D host tensors of ``x``'s dtype.  Returns ``(y, g)`` with ``g [groups, T]`` the gain curve, empty without ``return_gain``."""
    return native.ops().limiter_forward(x.contiguous(), float(c), int(A), int(H), window, int(up), taps, int(channels),
                                        bool(return_gain))


def limiter_plan_info(length: int, A: int, H: int, up: int = 1, taps: int = 0, dtype: torch.dtype = torch.float32,
                      groups: int = 1, channels: int = 1) -> dict:
    """What :func:`limiter_forward` does for groups of rows of ``length`` samples (``tfx_limiter_plan_info``; host-only, same
    checks on the sizes): ``tile`` (outputs per workgroup), ``tiles`` per group, ``halo_left`` / ``halo_right`` (input samples
    a tile reads behind its first and past its last output), ``Lp`` (taps per phase, 0 for ``up == 1``) and ``lds_bytes``.
    The tiling does not depend on ``groups`` or ``channels``."""
    return _query(L.load().tfx_limiter_plan_info,
                  (int(groups), int(channels), int(length), int(A), int(H), int(up), int(taps), _dt(dtype)),
                  "tile tiles halo_left halo_right Lp lds_bytes")


def limiter_stream_forward(x: Tensor, hist: Tensor | None, consumed: int, c: float, A: int, H: int, window: Tensor, up: int = 1,
                           taps: Tensor | None = None, channels: int = 1, return_gain: bool = False,
                           n_in: int | None = None) -> tuple[Tensor, Tensor | None, Tensor]:
    """One chunk of a limiter stream in one launch (``tfx_limiter_stream_forward``): ``x [..., T]`` follows ``consumed`` input
    samples per row, whose last ``Hs`` are ``hist [rows, Hs]`` (None = silence).  Returns ``(y, gain | None, new history)``:
    ``y[..., t]`` is sample ``consumed - D + t`` of :func:`limiter_forward` on the whole stream (0 where that is negative),
    ``gain [groups, T]`` the gain curve there (1 where negative) with ``return_gain``.  ``n_in`` (default: all ``T``) is the
    number of real inputs in ``x``; fewer says that the stream ends after them (the tail of a stream: ``T = D``, ``n_in = 0``).
    ``D`` and ``Hs`` are :func:`limiter_stream_plan_info`'s ``latency`` and ``history``; the other arguments are
    :func:`limiter_forward`'s."""
    y, g, h = native.ops().limiter_stream_forward(x.contiguous(), hist, int(consumed), float(c), int(A), int(H), window, int(up), taps,
                                                  int(channels), bool(return_gain), -1 if n_in is None else int(n_in))
    return y, (g if return_gain else None), h


def limiter_stream_plan_info(length: int, A: int, H: int, up: int = 1, taps: int = 0, dtype: torch.dtype = torch.float32,
                             groups: int = 1, channels: int = 1) -> dict:
    """What :func:`limiter_stream_forward` does with a chunk of ``length`` samples (``tfx_limiter_stream_plan_info``; host-only,
    same checks on the sizes): the stream's ``latency`` (D) and ``history`` (Hs) -- fixed by ``A``, ``H``, ``up`` and ``taps``
    alone --, ``tile`` (outputs per workgroup), ``tiles`` per group, ``positions`` (of the 8192 positions of the detector, the
    division and the sliding minimum, those the first workgroup sweeps) and ``lds_bytes``."""
    return _query(L.load().tfx_limiter_stream_plan_info,
                  (int(groups), int(channels), int(length), int(A), int(H), int(up), int(taps), _dt(dtype)),
                  "latency history tile tiles positions lds_bytes")


def compressor_forward(x: Tensor, th: float, s: float, w: float, alpha_a: float, alpha_r: float, makeup_db: float = 0.0,
                       channels: int = 1, state: Tensor | None = None, return_gain: bool = False,
                       segments: int = 0) -> tuple[Tensor, Tensor | None, Tensor]:
    """The feed-forward compressor (``tfx_compressor_forward``; the definition is :func:`torchfx_amd.dynamics.compress`'s) with
    its parameters already reduced: ``x [..., T]`` on the device (float32 / float64), its rows in groups of ``channels``
    consecutive rows that share one gain curve; ``th`` the threshold in dB, ``s = 1 - 1 / ratio``, ``w`` the knee width in dB,
    ``alpha_a`` / ``alpha_r`` the detector's coefficients ``exp(-1 / (time fs))`` (0 for a time of 0), ``state [groups, 2]``
    float64 ``(y1, yL)`` or None (silence).  ``segments`` cuts a group's row for the scan (0: the plan's choice; clamped to the
    tile count): one launch for one segment, three otherwise.  Returns ``(y, gain | None, new state [groups, 2] float64)``.
    The op lives in ``torch.ops.torchfx_dynamics``."""
    native.ops()                                         # loads the library: both namespaces are registered by the one module
    y, g, st = native.dynamics_ops().compressor_forward(x.contiguous(), float(th), float(s), float(w), float(alpha_a), float(alpha_r),
                                                        float(makeup_db), int(channels), state, bool(return_gain), int(segments))
    return y, (g if return_gain else None), st


def compressor_plan_info(length: int, groups: int = 1, channels: int = 1, segments: int = 0) -> dict:
    """What :func:`compressor_forward` does for ``groups`` rows of ``length`` samples (``tfx_compressor_plan_info``; host-only,
    same checks on the sizes): ``tile`` (samples per tile), ``tiles`` per group, the ``segments`` it takes for the request
    (0: chosen from ``groups`` and ``length``, 1 when the groups alone fill the chip), ``seg_tiles`` (tiles of the longest
    segment) and ``scratch_bytes`` (the summaries between the launches; 0 for one segment)."""
    return _query(L.load().tfx_compressor_plan_info, (int(groups), int(channels), int(length), int(segments)),
                  "tile tiles segments seg_tiles scratch_bytes")


LFO_SHAPES = ("sine", "triangle")                        # tfx_lfo_shape
INTERPOLATIONS = ("linear", "cubic")                     # tfx_interp


def _voice_table(voices) -> Tensor:
    """The host float64 ``[V, 5]`` table of ``(base, depth, inc, phase, gain)`` rows the modulated delay's entries take."""
    return torch.as_tensor(voices, dtype=torch.float64, device="cpu").reshape(-1, 5).contiguous()


def modulated_delay_forward(x: Tensor, voices, spread: float = 0.0, dry: float = 1.0, shape: str = "sine",
                            interpolation: str = "linear", position: int = 0) -> Tensor:
    """The modulated delay line (``tfx_modulated_delay_forward``; the definition is
    :func:`torchfx_amd.modulation.modulated_delay`'s) with its parameters already reduced: ``x [T]``, ``[C, T]`` or
    ``[B, C, T]`` on the device (float32 / float64), ``voices`` a ``[V, 5]`` table of ``(base, depth, inc, phase, gain)`` rows
    (delay and depth in samples, ``inc = rate / fs``, phase in cycles), ``position`` the absolute index of the first sample.
    One launch (``modulated_delay_kernel``).  The op lives in ``torch.ops.torchfx_modulation``."""
    native.ops()                                         # loads the library: every namespace is registered by the one module
    return native.modulation_ops().modulated_delay_forward(x.contiguous(), _voice_table(voices), float(spread), float(dry),
                                                           LFO_SHAPES.index(shape), INTERPOLATIONS.index(interpolation), int(position))


def modulated_delay_stream_forward(x: Tensor, hist: Tensor | None, pos: Tensor | None, voices, spread: float = 0.0, dry: float = 1.0,
                                   shape: str = "sine", interpolation: str = "linear") -> tuple[Tensor, Tensor, Tensor]:
    """One chunk of :func:`modulated_delay_forward` over a continuous stream, in one launch
    (``modulated_delay_stream_kernel``): the ``H`` samples of every row before ``x`` come from ``hist [rows, H]`` (None =
    silence; ``H`` is :func:`modulated_delay_plan_info`'s ``history``) and the position of the chunk's first sample from the
    device int64 ``pos [1]`` (None = 0).  Returns ``(y like x, new history, new position = pos + T)``; the chunks' outputs are
    bit-identical to the one-shot call on the whole signal."""
    native.ops()
    return native.modulation_ops().modulated_delay_stream_forward(x.contiguous(), hist, pos, _voice_table(voices), float(spread),
                                                                  float(dry), LFO_SHAPES.index(shape),
                                                                  INTERPOLATIONS.index(interpolation))


def modulated_delay_plan_info(length: int, voices, batch: int = 1, channels: int = 1, interpolation: str = "linear") -> dict:
    """What the modulated delay's launches do for ``[batch, channels, length]`` (``tfx_modulated_delay_plan_info``; host-only,
    same checks on the sizes and the voice table): ``tile`` (samples per tile), ``tiles`` per row, ``history`` (``H`` of a
    stream: ``max_v floor(base_v + depth_v) + 2``), ``batch_items`` (batch items one workgroup applies a delay ``(i, f)`` to)
    and ``batch_groups`` (the batch split of the grid; the grid is ``tiles * channels * batch_groups`` workgroups)."""
    t = _voice_table(voices)
    return _query(L.load().tfx_modulated_delay_plan_info,
                  (int(batch), int(channels), int(length), ctypes.c_void_p(t.data_ptr()), int(t.shape[0]),
                   INTERPOLATIONS.index(interpolation)), "tile tiles history batch_items batch_groups")


FREEVERB_LINES = ("lds", "global")                       # tfx_freeverb_lines


def _delay_table(delays, channels: int, what: str) -> np.ndarray:
    """A ``[channels, N]`` table of whole-sample delays as a contiguous int64 array (``N`` may be 0)."""
    a = np.asarray(delays)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"freeverb: {what} must hold integers (samples), got {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.int64).reshape(int(channels), -1)


def freeverb_forward(x: Tensor, comb_delays, allpass_delays, feedback: float, damp: float, allpass_gain: float = 0.5,
                     input_gain: float = 0.015, dry_gain: float = 1.0, wet1: float = 1.0, wet2: float = 0.0, tail: int = 0,
                     state: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """Freeverb (``tfx_freeverb_forward``; the definition is :func:`torchfx_amd.reverb.freeverb_bank`'s): ``x [T]``, ``[C, T]`` or
    ``[B, C, T]`` on the device (float32 / float64) with ``C`` 1 or 2, ``comb_delays [C, NC]`` and ``allpass_delays [C, NA]`` in
    samples, ``state [B * C, state_len]`` float64 or None (silence).  One workgroup per bank (``freeverb_kernel``), one launch
    for ``C = 1`` or ``wet2 = 0``, else a second one mixes (:func:`freeverb_plan_info`).  Returns ``(y [..., T + tail], new
    state)``.  The op lives in ``torch.ops.torchfx_reverb``."""
    native.ops()                                         # loads the library: every namespace is registered by the one module
    C = int(x.shape[-2]) if x.dim() >= 2 else 1
    return native.reverb_ops().freeverb_forward(x.contiguous(), _delay_table(comb_delays, C, "comb_delays").ravel().tolist(),
                                                _delay_table(allpass_delays, C, "allpass_delays").ravel().tolist(), float(feedback),
                                                float(damp), float(allpass_gain), float(input_gain), float(dry_gain), float(wet1),
                                                float(wet2), int(tail), state)


def freeverb_plan_info(length: int, comb_delays, allpass_delays, batch: int = 1, channels: int = 1, wet2: float = 0.0,
                       tail: int = 0) -> dict:
    """What :func:`freeverb_forward` does for ``[batch, channels, length]`` (``tfx_freeverb_plan_info``; host-only, same checks
    on the sizes and the delays): ``block`` (samples per block: the shortest comb delay, at most 1024), ``placement`` (``"lds"``
    or ``"global"``: where the delay lines live), ``state_len`` (float64 words per bank of the state), ``launches`` (2 when the
    channels cross-feed: ``channels = 2`` and ``wet2 != 0``) and ``workspace_bytes``."""
    cd, ad = _delay_table(comb_delays, channels, "comb_delays"), _delay_table(allpass_delays, channels, "allpass_delays")
    info = _query(L.load().tfx_freeverb_plan_info,
                  (int(batch), int(channels), int(length), int(tail), ctypes.c_void_p(cd.ctypes.data), int(cd.shape[1]),
                   ctypes.c_void_p(ad.ctypes.data) if ad.size else None, int(ad.shape[1]), float(wet2)),
                  "block placement:int state_len launches workspace_bytes")
    info["placement"] = FREEVERB_LINES[info["placement"]]
    return info


WAVESHAPES = ("hard", "cubic", "tanh", "curve")           # tfx_shape


def waveshaper_forward(x: Tensor, oversample: int, shape: str, curve: Tensor | None, drive: float, bias: float, dry: float, wet: float,
                       taps_up: Tensor | None = None, taps_dn: Tensor | None = None) -> Tensor:
    """The oversampled waveshaper in one launch (``tfx_waveshaper_forward``; the definition is
    :func:`torchfx_amd.waveshaper.waveshape`'s) with its parameters already reduced: ``x [..., T]`` on the device (float32 /
    float64), ``oversample`` 1, 2, 4 or 8, ``shape`` one of ``WAVESHAPES`` (``"curve"`` with ``curve``, a 1-D host tensor of 2
    to 4096 points in ``x``'s dtype), the linear ``drive``, ``bias``, ``dry`` and ``wet``, and for ``oversample > 1`` the taps of
    ``resample_poly(x, L, 1)`` and ``(x, 1, L)`` as 1-D host tensors of ``x``'s dtype, at most ``64 * oversample`` each
    (``waveshaper_kernel``; ``oversample = 1``: ``waveshaper_plain_kernel``).  The op lives in ``torch.ops.torchfx_shaper``."""
    native.ops()                                         # loads the library: every namespace is registered by the one module
    return native.shaper_ops().waveshaper_forward(x.contiguous(), int(oversample), WAVESHAPES.index(shape), curve, float(drive),
                                                  float(bias), float(dry), float(wet), taps_up, taps_dn)


def waveshaper_plan_info(length: int, oversample: int, taps_up: int = 0, taps_dn: int = 0, curve: int = 0,
                         dtype: torch.dtype = torch.float32, rows: int = 1) -> dict:
    """What :func:`waveshaper_forward` does for rows of ``length`` samples (``tfx_waveshaper_plan_info``; host-only, same checks
    on the sizes): ``tile`` (outputs per workgroup), ``tiles`` per row, ``reach_before`` / ``reach_after`` (the future / past
    input samples an output depends on), ``lds_bytes`` per workgroup, and ``taps_up`` / ``taps_dn`` (taps per phase of the
    up-sampler, taps of the zero-padded decimator).  The tiling does not depend on ``rows``."""
    return _query(L.load().tfx_waveshaper_plan_info,
                  (int(rows), int(length), int(oversample), int(taps_up), int(taps_dn), int(curve), _dt(dtype)),
                  "tile tiles reach_before reach_after lds_bytes taps_up taps_dn")


def waveshaper_stream_forward(x: Tensor, hist: Tensor | None, consumed: int, oversample: int, shape: str, curve: Tensor | None,
                              drive: float, bias: float, dry: float, wet: float, taps_up: Tensor | None = None,
                              taps_dn: Tensor | None = None, n_in: int | None = None) -> tuple[Tensor, Tensor]:
    """One chunk of a waveshaper stream in one launch (``tfx_waveshaper_stream_forward``): ``x [..., T]`` follows ``consumed``
    input samples per row, whose last ``Hs`` are ``hist [rows, Hs]`` (None = silence).  Returns ``(y, new history)``:
    ``y[..., t]`` is sample ``consumed - D + t`` of :func:`waveshaper_forward` on the whole stream (0 where that is negative),
    bit for bit.  ``n_in`` (default: all ``T``) is the number of real inputs in ``x``; fewer says that the stream ends after them
    (the tail of a stream: ``T = D``, ``n_in = 0``).  ``D`` and ``Hs`` are :func:`waveshaper_stream_plan_info`'s ``latency`` and
    ``history`` (both 0 for ``oversample = 1``); the other arguments are :func:`waveshaper_forward`'s
    (``waveshaper_stream_kernel``).  The op lives in ``torch.ops.torchfx_shaper_stream``."""
    native.ops()
    return native.shaper_stream_ops().waveshaper_stream_forward(x.contiguous(), hist, int(consumed), int(oversample),
                                                                WAVESHAPES.index(shape), curve, float(drive), float(bias), float(dry),
                                                                float(wet), taps_up, taps_dn, -1 if n_in is None else int(n_in))


def waveshaper_stream_plan_info(length: int, oversample: int, taps_up: int = 0, taps_dn: int = 0, curve: int = 0,
                                dtype: torch.dtype = torch.float32, rows: int = 1) -> dict:
    """What :func:`waveshaper_stream_forward` does with a chunk of ``length`` samples (``tfx_waveshaper_stream_plan_info``;
    host-only, same checks on the sizes): the stream's ``latency`` (D = ``reach_before``) and ``history`` (Hs = ``reach_before +
    reach_after``) -- fixed by ``oversample`` and the tap counts alone --, ``tile`` (outputs per workgroup), ``tiles`` per row,
    ``positions`` (of a workgroup's 2048 / 1024 positions, those whose up-sampled samples the first workgroup computes: whole
    waves) and ``lds_bytes``."""
    return _query(L.load().tfx_waveshaper_stream_plan_info,
                  (int(rows), int(length), int(oversample), int(taps_up), int(taps_dn), int(curve), _dt(dtype)),
                  "latency history tile tiles positions lds_bytes")


def phaser_forward(x: Tensor, stages: int, fs: float, rate: float, min_freq: float, max_freq: float, phase: float = 0.0,
                   spread: float = 0.0, dry: float = 0.5, wet: float = 0.5, shape: str = "sine", position: int = 0,
                   pos: Tensor | None = None, state: Tensor | None = None, return_coef: bool = False,
                   segments: int = 0) -> tuple[Tensor, Tensor | None, Tensor, Tensor | None]:
    """The phaser (``tfx_phaser_forward``; the definition is :func:`torchfx_amd.phaser.phase_shift`'s): ``x [T]``, ``[C, T]`` or
    ``[B, C, T]`` on the device (float32 / float64), ``stages`` all-pass sections swept between ``min_freq`` and ``max_freq`` Hz
    at ``rate`` Hz.  The position of the first sample is the host scalar ``position``, or the device int64 ``pos [1]`` of a
    stream; ``state [rows, stages + 1]`` float64 ``(x_0[-1], .., x_N[-1])`` or None (silence).  ``segments`` cuts a row for the
    scan (0: the plan's choice; clamped to the tile count): one launch for one segment, two otherwise.  Returns ``(y, coef |
    None, new state, pos + T | None)``: ``coef`` is ``a[n]`` as the kernel computed it, float64 ``[C, T]`` (``[1, T]`` when
    ``spread == 0`` or ``C == 1``); the new position is a fresh device tensor when ``pos`` was given.  The op lives in
    ``torch.ops.torchfx_phaser``."""
    native.ops()                                         # loads the library: every namespace is registered by the one module
    y, coef, st, pout = native.phaser_ops().phaser_forward(x.contiguous(), int(stages), float(fs), float(rate), float(min_freq),
                                                           float(max_freq), float(phase), float(spread), float(dry), float(wet),
                                                           LFO_SHAPES.index(shape), int(position), pos, state, bool(return_coef),
                                                           int(segments))
    return y, (coef if return_coef else None), st, (pout if pos is not None else None)


def phaser_plan_info(length: int, rows: int = 1, channels: int = 1, stages: int = 4, segments: int = 0) -> dict:
    """What :func:`phaser_forward` does for ``rows`` rows of ``length`` samples (``tfx_phaser_plan_info``; host-only, same checks
    on the sizes): ``tile`` (samples per tile), ``tiles`` per row, the ``segments`` it takes for the request (0: chosen from
    ``rows`` and ``length``, 1 when the rows alone fill the chip), ``seg_tiles`` (tiles of the longest segment) and
    ``scratch_bytes`` (the summaries between the launches; 0 for one segment)."""
    return _query(L.load().tfx_phaser_plan_info, (int(rows), int(channels), int(length), int(stages), int(segments)),
                  "tile tiles segments seg_tiles scratch_bytes")


def gate_forward(x: Tensor, p_open: float, p_close: float, r: float, hold: int, alpha_a: float, alpha_r: float, channels: int = 1,
                 state: Tensor | None = None, return_gain: bool = False, return_open: bool = False,
                 segments: int = 0) -> tuple[Tensor, Tensor | None, Tensor | None, Tensor]:
    """The noise gate (``tfx_gate_forward``; the definition is :func:`torchfx_amd.gate.gate`'s) with its parameters already
    reduced: ``x [..., T]`` on the device (float32 / float64), its rows in groups of ``channels`` consecutive rows that share one
    gain curve; ``p_open`` / ``p_close`` the linear opening and closing levels, ``r`` the linear gain of the closed gate,
    ``hold`` in samples, ``alpha_a`` / ``alpha_r`` the smoother's coefficients ``exp(-1 / (time fs))`` (0 for a time of 0),
    ``state [groups, 3]`` float64 ``(g, open, c)`` or None (closed, ``g = r``).  ``segments`` cuts a group's row for the scans
    (0: the plan's choice; clamped to the tile count): one launch for one segment, three otherwise.  Returns ``(y, gain | None,
    open | None, new state [groups, 3] float64)``.  The op lives in ``torch.ops.torchfx_gate``."""
    native.ops()                                         # loads the library: every namespace is registered by the one module
    y, g, o, st = native.gate_ops().gate_forward(x.contiguous(), float(p_open), float(p_close), float(r), int(hold), float(alpha_a),
                                                 float(alpha_r), int(channels), state, bool(return_gain), bool(return_open),
                                                 int(segments))
    return y, (g if return_gain else None), (o if return_open else None), st


def gate_plan_info(length: int, groups: int = 1, channels: int = 1, segments: int = 0) -> dict:
    """What :func:`gate_forward` does for ``groups`` rows of ``length`` samples (``tfx_gate_plan_info``; host-only, same checks
    on the sizes): ``tile`` (samples per tile), ``tiles`` per group, the ``segments`` it takes for the request (0: chosen from
    ``groups`` and ``length``, 1 when the groups alone fill the chip), ``seg_tiles`` (tiles of the longest segment) and
    ``scratch_bytes`` (the summaries between the launches; 0 for one segment)."""
    return _query(L.load().tfx_gate_plan_info, (int(groups), int(channels), int(length), int(segments)),
                  "tile tiles segments seg_tiles scratch_bytes")


STFT_PAD_MODES = {"constant": 0, "reflect": 1, "replicate": 2, "circular": 3}      # enum tfx_stft_pad
STFT_POWERS = {None: 0, 1.0: 1, 2.0: 2}                                            # complex, |X|, |X|^2


def stft_forward(x: Tensor, window: Tensor | None, n_fft: int, hop: int, pad: int, pad_mode: str = "reflect",
                 power: float | None = None, normalized: bool = False) -> Tensor:
    """The short-time Fourier transform of the LDS route (``tfx_stft_forward``; the definition is
    :func:`torchfx_amd.spectral.stft`'s): ``x [..., T]`` on the device (float32 / float64), ``window`` a 1-D device tensor of
    ``x``'s dtype with 1 to ``n_fft`` values (centred in zeros) or None (ones), ``pad`` samples added at each end
    (``n_fft // 2`` for ``center=True``, 0 without) by ``pad_mode`` ("reflect" / "constant"), ``power`` None (complex), 1.0 or 2.0.
    Returns ``[..., n_fft // 2 + 1, frames]``, a transposed view of a contiguous ``[..., frames, bins]`` buffer.  A geometry
    off the route (:func:`stft_plan_info`) is an error here, not a fall-back.  The op lives in ``torch.ops.torchfx_spectral``."""
    native.ops()                                         # loads the library: every namespace is registered by the one module
    if pad_mode not in STFT_PAD_MODES:
        raise ValueError(f"stft_forward: pad_mode must be one of {sorted(STFT_PAD_MODES)}, got {pad_mode!r}")
    if power not in STFT_POWERS:
        raise ValueError(f"stft_forward: power must be None, 1.0 or 2.0, got {power!r}")
    return native.spectral_ops().stft_forward(x, window, int(n_fft), int(hop), int(pad), STFT_PAD_MODES[pad_mode], STFT_POWERS[power],
                                              bool(normalized))


def stft_plan_info(n_fft: int, hop: int, win_length: int, length: int, rows: int = 1, dtype: torch.dtype = torch.float32,
                   center: bool = True, pad_mode: str = "reflect", onesided: bool = True) -> dict:
    """What an STFT of this geometry does (``tfx_stft_plan_info``; host-only, same checks on the sizes): ``route`` ("lds": the
    one-launch kernel, "torch": ``torch.stft`` on the tensor's device), ``frames`` per row and, for the LDS route,
    ``frames_per_workgroup``, ``threads_per_frame``, ``lds_bytes`` and ``workgroups`` (``rows * ceil(frames /
    frames_per_workgroup)``; zeros on the torch route)."""
    if pad_mode not in STFT_PAD_MODES:
        raise ValueError(f"stft_plan_info: pad_mode must be one of {sorted(STFT_PAD_MODES)}, got {pad_mode!r}")
    info = _query(L.load().tfx_stft_plan_info, (int(n_fft), int(hop), int(win_length), int(length), int(rows), _dt(dtype), int(bool(center)),
                                                STFT_PAD_MODES[pad_mode], int(bool(onesided))),
                  "route:int frames frames_per_workgroup threads_per_frame lds_bytes workgroups")
    info["route"] = "lds" if info["route"] == 1 else "torch"
    return info


def istft_forward(spec: Tensor, window: Tensor | None, n_fft: int, hop: int, pad: int, length: int | None = None,
                  normalized: bool = False) -> tuple[Tensor, Tensor]:
    """The inverse short-time Fourier transform of the LDS route (``tfx_istft_forward``; the definition is
    :func:`torchfx_amd.spectral.istft`'s): ``spec [bins, frames]``, ``[C, bins, frames]`` or ``[B, C, bins, frames]`` on the device
    (complex64 / complex128, ``bins = n_fft // 2 + 1``), ``window`` a 1-D device tensor of the matching real dtype with ``hop`` to
    ``n_fft`` values (centred in zeros) or None (ones), ``pad`` samples cut from each end (``n_fft // 2`` for ``center=True``),
    ``length`` None for the natural length.  Returns ``(y [..., T], flag)``: ``flag`` is a one-element int32 device tensor, 1
    when the window's overlap-add envelope vanishes somewhere in the returned range (torch's "window overlap add min" error).
    It is not read here, so the call does not synchronise.  The kernel reads the layout :func:`stft_forward` returns (the
    transpose of a contiguous ``[..., frames, bins]`` buffer) in place; any other layout costs one copy into it first.  A
    geometry off the route (:func:`istft_plan_info`) is an error here, not a fall-back.  The op lives in
    ``torch.ops.torchfx_spectral_inverse``."""
    native.ops()                                         # loads the library: every namespace is registered by the one module
    return native.spectral_inverse_ops().istft_forward(spec, window, int(n_fft), int(hop), int(pad), -1 if length is None else int(length),
                                                       bool(normalized))


def istft_plan_info(n_fft: int, hop: int, win_length: int, frames: int, rows: int = 1, dtype: torch.dtype = torch.float32,
                    center: bool = True, length: int | None = None, onesided: bool = True) -> dict:
    """What an ISTFT of this geometry does (``tfx_istft_plan_info``; host-only, same checks on the sizes): ``route`` ("lds": the
    one-launch kernel, "torch": ``torch.istft`` on the tensor's device), the output ``length`` and, for the LDS route, ``tile``
    (output samples a workgroup owns), ``frames_per_batch``, ``threads_per_frame``, ``lds_bytes``, ``workgroups`` (``rows *
    ceil(length / tile)``) and ``redundant_share``: ``e / (tile / hop + e)`` with ``e = ceil(n_fft / hop) - 1``, the share of a
    tile's transforms that its neighbour runs too (zeros on the torch route).  ``dtype`` is the real or the complex one."""
    dtype = {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(dtype, dtype)
    info = _query(L.load().tfx_istft_plan_info, (int(n_fft), int(hop), int(win_length), int(frames), int(rows), _dt(dtype), int(bool(center)),
                                                 -1 if length is None else int(length), int(bool(onesided))),
                  "route:int length tile frames_per_batch threads_per_frame lds_bytes workgroups redundant_share:double")
    info["route"] = "lds" if info["route"] == 1 else "torch"
    return info


RESAMPLE_STREAM_KERNELS = ("resample_stream_reg_kernel", "resample_stream_lds_kernel", "resample_stream_gather_kernel", "copy")


def resample_stream_plan_info(consumed: int, length: int, up: int, down: int, taps: int,
                              dtype: torch.dtype = torch.float32) -> dict:
    """What :func:`resample_stream_forward` does with a chunk of ``length`` samples after ``consumed`` (host-only):
    the outputs ``[out_begin, out_end)`` it emits, ``hist_len`` (H), ``n_pre_remove`` (outputs held back), ``Lp`` (taps per
    phase), ``kernel`` and ``lds_bytes`` per workgroup."""
    q = _query(L.load().tfx_resample_stream_plan_info, (int(consumed), int(length), int(up), int(down), int(taps), _dt(dtype)),
               "out_begin out_end hist_len n_pre_remove Lp kernel:int lds_bytes")
    q["kernel"] = RESAMPLE_STREAM_KERNELS[q["kernel"]]
    return q


_TAPS_HOST: dict = {}        # (id(base tensor), offset, numel, dtype wanted) -> (weakref to base, version, host tensor)


def _kernel_host(kernel, dtype: torch.dtype) -> Tensor:
    """Flat host copy of the taps in the signal's dtype.  The C ABI takes the taps as a host array (they
    key its device-side caches), so a filter whose taps live on the GPU, or in another dtype (the planner's merged
    kernels are float64), would otherwise pay a copy on every forward -- a blocking device-to-host copy in the first
    case, a fresh quarter-megabyte host allocation in the second (and a process that keeps mapping and unmapping
    host memory while kernels are in flight gets its GPU queues stalled by the driver for tens of milliseconds:
    measured, `profiles/r02_experiments.txt`).  The copy is cached per BASE tensor object -- modules hand in
    `self.kernel.reshape(-1)`, a new view object per call -- and invalidated by the version counter (in-place
    edits) or the tensor's death."""
    if not isinstance(kernel, Tensor):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(kernel).reshape(-1))).to(dtype)
    base = kernel._base if kernel._base is not None else kernel
    key = (id(base), kernel.storage_offset(), kernel.numel(), tuple(kernel.stride()), dtype)
    ent = _TAPS_HOST.get(key)
    if ent is not None and ent[0]() is base and ent[1] == kernel._version:
        return ent[2]
    k = kernel.detach().to(device="cpu").reshape(-1).to(dtype).contiguous()
    if k.data_ptr() == kernel.data_ptr():          # nothing was copied: nothing to cache (and nothing allocated per call)
        return k
    if len(_TAPS_HOST) > 64:
        for dead in [kk for kk, e in _TAPS_HOST.items() if e[0]() is None] or list(_TAPS_HOST)[:32]:
            _TAPS_HOST.pop(dead, None)
    _TAPS_HOST[key] = (weakref.ref(base), kernel._version, k)
    return k


def fir_direct_forward(x: Tensor, kernel) -> Tensor:
    """Causal depthwise FIR, direct form: the ``conv_mode="direct"`` branch of ``FIR.forward``
    (``fir.py:556-568``).  ``x [C,T]``; ``kernel`` = the FLIPPED taps (the module's ``[1,1,K]`` buffer, any
    shape with K elements)."""
    return native.ops().fir_direct_forward(x, _kernel_host(kernel, x.dtype))


def fft_conv_forward(x: Tensor, kernel, padding: tuple[int, int] = (0, 0), epilogue: Epilogue | None = None) -> Tensor:
    """Overlap-save FFT convolution with ``fft_conv1d`` semantics (``_fftconv.py:70-141``) on ``x [C,T]``:
    returns ``[C, T + l + r - K + 1]``."""
    if epilogue is not None:
        y, epilogue.stat_value = native.ops().fft_conv_forward_ep(
            x, _kernel_host(kernel, x.dtype), int(padding[0]), int(padding[1]), epilogue.gain, epilogue.clamp,
            epilogue.stat_mode, epilogue.per_row)
        return y
    return native.ops().fft_conv_forward(x, _kernel_host(kernel, x.dtype), int(padding[0]), int(padding[1]))


def sos_fft_conv_supported(T: int, sos, taps: int, padding: tuple[int, int] = (0, 0), force_block: bool = False) -> bool:
    """Whether :func:`sos_fft_conv_forward` serves float32 rows of ``T`` samples with this cascade and tap count
    (``tfx_sos_fft_conv_supported``; host-only, no device needed)."""
    s = sos_array(sos)
    return bool(L.load().tfx_sos_fft_conv_supported(
        ctypes.c_int64(int(T)), s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int64(s.shape[0]),
        ctypes.c_int64(int(taps)), ctypes.c_int64(int(padding[0])), ctypes.c_int64(int(padding[1])), ctypes.c_int(int(force_block))))


def sos_fft_conv_plan_info(T: int, sos, taps: int, padding: tuple[int, int] = (0, 0), force_block: int = 0) -> dict | None:
    """Block length ``N``, hop ``S``, frames per row ``F`` and warm-up samples of :func:`sos_fft_conv_forward` for rows of
    ``T`` samples, or None where it does not serve the geometry (``tfx_sos_fft_conv_plan_info2``; host-only).  ``tail_N`` /
    ``tail_S``: block and hop of the row's last frame where it runs at a smaller block than the ``F - 1`` before it, else 0."""
    s = sos_array(sos)
    n, h, f, w, tn, ts = (ctypes.c_int64(0) for _ in range(6))
    ok = L.load().tfx_sos_fft_conv_plan_info2(ctypes.c_int64(int(T)), s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                             ctypes.c_int64(s.shape[0]), ctypes.c_int64(int(taps)), ctypes.c_int64(int(padding[0])),
                                             ctypes.c_int64(int(padding[1])), ctypes.c_int(int(force_block)), ctypes.byref(n),
                                             ctypes.byref(h), ctypes.byref(f), ctypes.byref(w), ctypes.byref(tn), ctypes.byref(ts))
    return {"N": n.value, "S": h.value, "F": f.value, "warmup": w.value, "tail_N": tn.value, "tail_S": ts.value,
            "workspace_bytes_held": workspace_bytes()} if ok else None


def clear_caches() -> None:
    """Drop every cached plan and hand all device workspaces back to their allocator (``tfx_clear_caches``): PyTorch's caching
    allocator under this module, so ``torch.cuda.empty_cache()`` afterwards returns them to the driver."""
    L.check(L.load().tfx_clear_caches())


def workspace_bytes() -> int:
    """Bytes of device workspace the library holds right now (overlap-save slabs, statistic partials ...; all streams and
    devices).  Under the torch module they come from PyTorch's caching allocator (``tfx_set_workspace_allocator``): they are
    part of ``torch.cuda.memory_allocated()`` and :func:`clear_caches` hands them back to it."""
    return int(L.load().tfx_workspace_bytes())


def sos_fft_conv_warmup(sos) -> int:
    """Samples a row's recursion starts early (from zero state) inside the column pass of :func:`sos_fft_conv_forward`."""
    s = sos_array(sos)
    return int(L.load().tfx_sos_fft_conv_warmup(s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int64(s.shape[0])))


def sos_fft_conv_forward(x: Tensor, sos, kernel, padding: tuple[int, int] = (0, 0), *, return_sections: bool = False,
                         force_block: int = 0, epilogue: Epilogue | None = None):
    """A zero-state SOS cascade followed by ``fft_conv1d`` as ONE overlap-save pipeline in the reference's arithmetic:
    float64 DF1 recursion (``_ops.py:119-176`` with ``state=None`` -> ``iir_cpu.cpp:64-159``), the downcast to float32
    (``iir.py:84-184``), float32 overlap-save (``_fftconv.py:70-141``).  The recursion runs inside the forward column
    pass of the transform.  ``x [C,T]`` float32; returns ``y [C, T+l+r-K+1]`` (+ the float64 output of every section
    ``[K,C,T]`` with ``return_sections``).  ``force_block``: 1 / 2 = take the 2^20 / 2^21-point block whatever the row length
    (tests at fixture size).  Raises when :func:`sos_fft_conv_supported` says no."""
    ep = epilogue if epilogue is not None else Epilogue()
    y, stat, sec = native.ops().sos_fft_conv_forward(
        x, _coeff(sos), _kernel_host(kernel, x.dtype), int(padding[0]), int(padding[1]), bool(return_sections),
        int(force_block), ep.gain, ep.clamp, ep.stat_mode, ep.per_row)
    if epilogue is not None:
        epilogue.stat_value = stat
    return (y, sec) if return_sections else y


def normalize_apply(x: Tensor, stat: Tensor, peak: float, mode: int = 0, per_row: bool = False) -> Tensor:
    """The apply half of ``Normalize`` on a raw statistic an epilogue left on the device (``stat``: float64
    ``[rows]`` or ``[1]``, max|x| for ``STAT_ABSMAX``, sum of squares for ``STAT_RMS``): one streaming pass."""
    return native.ops().normalize_apply(x, stat, float(peak), int(mode), bool(per_row))


def fir_stream_forward(x: Tensor, kernel, hist: Tensor | None, direct: bool = False) -> tuple[Tensor, Tensor]:
    """One chunk of a stateful FIR: ``x [C,T]`` continues the signal whose last ``K-1`` samples are ``hist
    [C,K-1]`` (``None`` = silence).  Returns ``(y [C,T], new_hist [C,K-1])``.  The kernels read history and
    chunk from their two buffers -- no concatenated copy of the chunk."""
    return native.ops().fir_stream_forward(x, _kernel_host(kernel, x.dtype), hist, bool(direct))


def chunk_supported(C: int, T: int, K: int, taps: int) -> bool:
    """Whether :func:`chunk_forward` takes a ``[C, T]`` chunk with ``K`` sections and ``taps`` FIR taps (host-only query)."""
    return bool(L.load().tfx_chunk_supported(int(C), int(T), int(K), int(taps)))


def chunk_forward(x: Tensor, sos, state_x: Tensor | None, state_y: Tensor | None, kernel, hist: Tensor | None,
                  gain: float | None = None, clamp: bool = False, *, precision=None):
    """ONE launch for one small streaming chunk ``x [C, T]`` (float32): SOS cascade with carried state -> stateful
    direct FIR (``kernel`` = flipped taps, ``hist [C, K-1]`` or None) -> ``* gain`` (None = no gain stage) and clip.
    Returns ``(y, new_state_x, new_state_y, new_hist)``; same arithmetic as ``sos_forward`` -> ``fir_stream_forward(direct)`` ->
    ``gain_forward`` (equal to float64 round-off of the recursion).  ``sos [K, 6]`` host float64 (``K`` may be 0), limits: :func:`chunk_supported`."""
    return native.ops().chunk_forward(x, _coeff(sos), state_x, state_y, _kernel_host(kernel, torch.float32), hist,
                                      1.0 if gain is None else float(gain), gain is not None, bool(clamp), _prec(precision))


def sum_forward(tensors: list[Tensor]) -> Tensor:
    """Sum of equally-shaped tensors in list order (``__base.py:1022-1026``)."""
    if not tensors:
        raise RuntimeError("sum_forward: need at least one tensor")
    return native.ops().sum_forward(list(tensors))


STAT_ABSMAX, STAT_RMS = 0, 1


def gain_forward(x: Tensor, gain: float, clamp: bool = False) -> Tensor:
    """``y = x * gain`` (+ clip to [-1, 1]) -- ``Gain.forward``, ``effect.py:361-383``; ``gain`` is the linear
    factor."""
    return native.ops().gain_forward(x, float(gain), bool(clamp))


def quantile_abs(x: Tensor, q: float) -> Tensor:
    """``torch.quantile(torch.abs(x), q, interpolation="linear")`` over all elements of a float32 signal as a three-pass radix
    select on the device (no sort, no 16 M element limit, no host sync): float64 ``[1]`` on the device, the same value
    torch.quantile returns wherever it runs; NaN anywhere in ``x`` -> NaN.  Feed it to :func:`normalize_apply`."""
    return native.ops().quantile_abs(x, float(q))


def stat_forward(x: Tensor, mode: int = STAT_ABSMAX, per_row: bool = False) -> Tensor:
    """``max|x|`` (``STAT_ABSMAX``) or ``sqrt(mean(x^2))`` (``STAT_RMS``) over everything, or per row of the
    ``[rows, T]`` view -- float64 on the device, no host sync."""
    return native.ops().stat_forward(x, int(mode), bool(per_row))


def normalize_forward(x: Tensor, peak: float, mode: int = STAT_ABSMAX, per_row: bool = False) -> Tensor:
    """``s > 0 ? x / s * peak : x`` with ``s`` = abs-max or RMS, global or per row of the ``[rows, T]`` view
    (``effect.py:696-698,719-721,775-786``); two streaming passes, statistic stays on device."""
    return native.ops().normalize_forward(x, float(peak), int(mode), bool(per_row))


def effects_plan_info(length: int, dtype: torch.dtype = torch.float32) -> dict:
    """The geometry of :func:`gain_forward`, :func:`stat_forward`, :func:`normalize_forward`, :func:`sum_forward` and the two
    delay-line ops for rows of ``length`` samples (``tfx_effects_plan_info``; host-only, the launches' own constants): ``vec``
    (samples per 16-byte vector), ``tile`` (samples per workgroup of an elementwise pass), ``group`` (samples one first-stage
    reduce workgroup turns into one partial), ``groups`` (partials per row), ``finish_threads`` (threads of the second stage's
    workgroup; more partials than that take strided trips) and ``stream_tile`` (samples per workgroup of
    :func:`delay_line_stream_forward`)."""
    return _query(L.load().tfx_effects_plan_info, (int(length), _dt(dtype)), "vec tile group groups finish_threads stream_tile")


def deinterleave_forward(frames: Tensor, out: Tensor | None = None, frame_base: int = 0,
                         scale: float = 1.0 / 32768.0) -> Tensor:
    """Interleaved ``[F, C]`` (float32, or int16 PCM scaled by ``scale``) -> planar float32 ``[C, F]`` (the
    device-side ``data_np.T.copy()`` of ``wave.py:448-452``).  With ``out`` ``[C, F_total]`` the chunk lands
    at frames ``[frame_base, frame_base + F)`` of every row."""
    if out is None:
        return native.ops().deinterleave_forward(frames, float(scale))
    native.ops().deinterleave_into(frames, out, int(frame_base), float(scale))
    return out


def interleave_forward(x: Tensor, frame_base: int = 0, frames: int | None = None) -> Tensor:
    """Planar float32 ``[C, F_total]`` -> interleaved ``[F, C]`` of frames ``[frame_base, frame_base+F)`` (the
    device-side ``.numpy().T`` of ``wave.py:566-573``)."""
    return native.ops().interleave_forward(x, int(frame_base), -1 if frames is None else int(frames))


# ---- host-only planning queries (no tensors, no GPU needed): ctypes over the C ABI --------------------
def sos_plan_info(sos, refine: bool = True) -> dict:
    """Host-side plan facts for an SOS matrix: warm-up halo length, the float32 error estimate and what
    ``precision='auto'`` would choose; ``unit_form`` (float32 signals on aligned rows run the unit-b0 form) and the
    refinement rule of the float64 arithmetic (``tfx_sos_refine_info``): ``refine_f32`` / ``refine_f64`` = launches with a
    float32 / float64 result take the kernels with refined start states, decided on ``blocked_error`` against
    ``sequential_error`` (each at 64 and at 16 samples per lane).  ``refine=False`` leaves those five out and with them the
    host replay they rest on (about 10 ms for four sections, once per plan and tile size)."""
    lib = L.load()
    s = np.ascontiguousarray(sos.detach().cpu().numpy() if isinstance(sos, Tensor) else sos, dtype=np.float64)
    if s.ndim != 2 or s.shape[-1] != 6:
        raise RuntimeError(f"expected [K, 6], got shape {tuple(s.shape)}")
    coeffs = (s.ctypes.data_as(ctypes.c_void_p), s.shape[0])
    q = _query(lib.tfx_sos_plan_info, coeffs, "auto_precision:int warmup f32_error_bound:double")
    q["auto_precision"] = "f32" if q["auto_precision"] == L.PREC_F32 else "f64"
    if not refine:          # the warm-up and the float32 estimate alone: no replay of the float64 kernel (about 10 ms per plan)
        return q
    r = _query(lib.tfx_sos_refine_info, coeffs, "unit_form:int refine_f32:int refine_f64:int errs:double4")
    errs = r.pop("errs")
    q.update({k: bool(v) for k, v in r.items()})
    q.update(blocked_error=(errs[0], errs[2]), sequential_error=(errs[1], errs[3]))
    return q


SOS_ROUTES = ("sequential", "halo", "handoff")          # enum tfx_sos_route


def sos_route_info(sos, rows: int, length: int, dtype: torch.dtype = torch.float32, out_dtype: torch.dtype | None = None,
                   precision=None, sections: bool = False, wave_slots: int = 0) -> dict:
    """How :func:`sos_forward` cuts ``rows`` rows of ``length`` samples into time segments (``tfx_sos_route_info``; the call's own
    decision, host-only when ``wave_slots`` is given): ``route`` ("sequential", "halo" or "handoff" -- exact segment starts for
    cascades whose memory is too long for a halo), ``nseg`` segments per row, ``seg_len`` samples between segment starts,
    ``warmup`` (the halo in force; 0 unless "halo"), ``passes`` (reads of the signal) and ``bytes_per_sample``.
    ``wave_slots``: the wavefronts the device is taken to hold (2048 on MI355X for the float64 kernels); 0 asks the current
    device.  ``TFX_SOS_NSEG`` / ``TFX_SOS_HANDOFF`` act on the query as on the call."""
    a = sos_array(sos)
    q = _query(L.load().tfx_sos_route_info,
               (int(rows), int(length), a.ctypes.data, a.shape[0], _dt(dtype), _dt(dtype if out_dtype is None else out_dtype),
                L.precision_code(precision), int(bool(sections)), int(wave_slots)),
               "route:int nseg seg_len warmup passes:int bytes_per_sample:double")
    q["route"] = SOS_ROUTES[q["route"]]
    return q


def env_reload() -> None:
    """The library reads every ``TFX_*`` knob ONCE per process; after changing one in ``os.environ`` call this (``tfx_env_reload``)
    -- or start the process with ``TFX_ENV_DYNAMIC=1`` to make every lookup a fresh ``getenv``."""
    L.check(L.load().tfx_env_reload())


def prewarm(device=None) -> None:
    """Start the one-time per-device set-up of the overlap-save path on a helper thread (``tfx_prewarm``); returns at once."""
    lib = L.load()
    if device is not None and torch.device(device).type == "cuda":
        with torch.cuda.device(device):
            L.check(lib.tfx_prewarm())
    else:
        L.check(lib.tfx_prewarm())


def ols_plan_info(K: int, T: int, padding: tuple[int, int] = (0, 0), dtype: torch.dtype = torch.float32) -> dict:
    """Block geometry of the overlap-save op for a signal of `dtype` (FFT length N, hop S, blocks per row F) and the
    path that runs: "lds" (one launch, 4096-point transform in LDS), "passes" (three-pass four-step pipeline) or
    "rocfft"; `native` = a hand-written path; `bytes_per_sample` = modelled HBM traffic per output sample."""
    q = _query(L.load().tfx_ols_plan_info2, (int(K), int(T), int(padding[0]), int(padding[1]), _dt(dtype)), "N S F path:int")
    path, esz = q["path"], 8 if dtype == torch.float64 else 4
    bps = {2: esz * q["N"] / q["S"] + esz, 1: (20.0 * q["N"] / q["S"] + 4.0) * esz / 4, 0: 95.0 * esz / 4}[path]
    return {"N": q["N"], "S": q["S"], "F": q["F"], "native": path != 0, "path": ("rocfft", "passes", "lds")[path],
            "bytes_per_sample": bps}
