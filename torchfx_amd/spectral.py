"""Looking at a signal in frequency, and coming back: the short-time Fourier transform, the spectrogram and the inverse.

:func:`stft` is ``torch.stft(..., return_complex=True)`` along the last axis -- same defaults, errors, result shape and result
strides -- and :func:`spectrogram` its magnitude or power with a named window.  :func:`istft` is ``torch.istft`` over the last two
axes, so that ``istft(stft(x) * mask)`` is a round trip through the library.  These are analyses and a synthesis: they return
tensors, there is no ``FX`` class, nothing in the planner and nothing in the stream processors.

On a ROCm device the transform is one launch of ``torchfx_amd/csrc/stft.hip`` (``torchfx_ext.stft_forward``) that reads the signal
once and writes only the result: the centre padding is part of the kernel's addressing, the frames are formed in LDS and each is
transformed on its own, so a frame's bits depend on its ``n_fft`` samples and the window alone.  That route serves ``n_fft`` in
256 ... 4096 (powers of two), ``onesided=True`` and ``pad_mode`` "reflect" / "constant" (any with ``center=False``); every other
geometry, and every CPU tensor, takes ``torch.stft`` on the tensor's own device, so the functions are total.
``torchfx_ext.stft_plan_info`` says which route a geometry takes.

The inverse is one launch of ``torchfx_amd/csrc/istft.hip`` (``torchfx_ext.istft_forward``) that reads the spectrum once, in the
layout :func:`stft` returns, and writes only the signal: a workgroup owns a tile of output samples, transforms the frames that
cover it with the forward kernel's stages and tables, and adds them in ascending frame order in registers -- no frame matrix, no
envelope array, no atomics -- so a sample's bits depend on the frames that cover it and the window alone.  That route serves the
same ``n_fft``, one-sided spectra and ``return_complex=False``; everything else takes ``torch.istft`` on the tensor's own device
(``torchfx_ext.istft_plan_info``).

The mel spectrogram (:func:`mel_spectrogram`, :class:`MelSpectrogram`, :func:`mel_filterbank`) is one launch of
``torchfx_amd/csrc/mel.hip`` (``torchfx_ext.mel_forward``): the STFT kernel's front, then the filterbank -- as a table of bands --
and the logarithm applied to the power spectrum while it lies in the workgroup's LDS, so that only ``[..., frames, n_mels]`` is
written.  It serves what the STFT's route serves with up to 256 filters whose bands fit LDS; everything else (CPU tensors, other
``n_fft``, dense banks) is the composition spectrogram, ``matmul``, logarithm on the tensor's own device
(``torchfx_ext.mel_plan_info``).

Not here: ``onesided=False`` and ``return_complex=True`` on the device route, MFCC / DCT, the inverse mel transform, streaming
forms, autograd, axes other than the last.

Between the two transforms stands the phase vocoder (:func:`phase_vocoder`, ``torchaudio.functional.phase_vocoder``'s meaning):
one or two launches of ``torchfx_amd/csrc/phasevocoder.hip`` (``torchfx_ext.phase_vocoder_forward``) that read the spectrum once,
in the layout :func:`stft` returns, and write the stretched one once, in the layout :func:`istft` reads, with the running phase
kept exactly as a 64-bit integer.  On it rest :func:`time_stretch` / :class:`TimeStretch` (tempo without pitch) and
:func:`pitch_shift` / :class:`PitchShift` (pitch without tempo; the last step is :func:`torchfx_amd.resample_poly`).
``phase_lock="identity"`` on any of them locks every bin's phase to its nearest spectral peak (Laroche & Dolson 1999): a kernel
of its own in the same file, one workgroup per (row, time segment) with the frame's moduli, phases and peak mask in LDS.  Not
provided: scaled phase locking, transient preservation, formant correction, a streaming vocoder, autograd, axes
other than the last two, a time-varying ``rate``.
"""
from __future__ import annotations

import fractions
import math
import re
import warnings

import numpy as np
import torch
from torch import Tensor

from torchfx_amd import torchfx_ext as E
from torchfx_amd.effect import FX

__all__ = ["stft", "spectrogram", "istft", "named_window", "mel_filterbank", "mel_spectrogram", "MelSpectrogram", "phase_vocoder",
           "time_stretch", "pitch_shift", "TimeStretch", "PitchShift"]

_NAMED = {"hann": torch.hann_window, "hamming": torch.hamming_window, "rect": torch.ones}


def named_window(name: str, win_length: int, dtype: torch.dtype = torch.float32, device=None) -> Tensor:
    """torch's periodic ``"hann"`` / ``"hamming"`` window or ``"rect"`` (ones) of ``win_length`` values, built in float64 and
    rounded once to ``dtype``."""
    if name not in _NAMED:
        raise ValueError(f"window must be a tensor or one of {sorted(_NAMED)}, got {name!r}")
    if name == "rect":
        return torch.ones(int(win_length), dtype=dtype, device=device)
    return _NAMED[name](int(win_length), periodic=True, dtype=torch.float64).to(dtype=dtype, device=device)


def _torch_stft(x: Tensor, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided) -> Tensor:
    """``torch.stft`` itself; the one thing added is a ``[B, C, T]`` input, whose leading axes it takes as rows."""
    lead = None
    if x.dim() == 3:
        lead, x = x.shape[:2], x.reshape(-1, x.shape[-1])
    y = torch.stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, return_complex=True)
    return y if lead is None else y.unflatten(0, tuple(lead))


def _check_as_torch(x: Tensor, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided) -> None:
    """Raise what ``torch.stft`` raises for these arguments, in its wording: it is asked itself, on tensors without storage
    (whose type names in the message are put back to the real tensors': ``MetaFloatType`` -> ``torch.cuda.FloatTensor``)."""
    xm = torch.empty(x.shape, dtype=x.dtype, device="meta")
    wm = None if window is None else torch.empty(window.shape, dtype=window.dtype, device="meta")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _torch_stft(xm, n_fft, hop_length, win_length, wm, center, pad_mode, normalized, onesided)
    except RuntimeError as e:
        prefix = "torch.cuda." if x.is_cuda else "torch."
        msg = re.sub(r"Meta(\w+?)Type", lambda m: f"{prefix}{m.group(1)}Tensor", str(e))
        raise type(e)(re.sub(r"torch\.Size\((\[[^\]]*\])\)", r"\1", msg)) from None      # the padding check prints sizes bare


def _on_lds_route(x: Tensor, n_fft: int, hop: int, win_length: int, window: Tensor | None, center: bool, pad_mode: str,
                  onesided: bool | None) -> bool:
    if not x.is_cuda or x.dtype not in (torch.float32, torch.float64) or x.dim() not in (1, 2, 3) or pad_mode not in E.STFT_PAD_MODES:
        return False
    if window is not None and (window.dtype != x.dtype or window.device != x.device):
        return False
    rows = x.numel() // max(1, x.shape[-1])
    info = E.stft_plan_info(n_fft, hop, win_length, x.shape[-1], rows, x.dtype, center, pad_mode, onesided is None or bool(onesided))
    return info["route"] == "lds"


def _to_power(y: Tensor, power: float | None) -> Tensor:
    if power is None:
        return y
    return y.abs() if power == 1.0 else y.real.square() + y.imag.square()


def _stft(x: Tensor, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, power) -> Tensor:
    if not isinstance(x, Tensor):
        raise TypeError(f"stft: expected a tensor, got {type(x).__name__}")
    if not x.is_cuda:
        return _to_power(_torch_stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided), power)
    _check_as_torch(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided)
    hop = int(hop_length) if hop_length is not None else int(n_fft) // 4
    wl = int(win_length) if win_length is not None else int(n_fft)
    if _on_lds_route(x, int(n_fft), hop, wl, window, bool(center), pad_mode, onesided):
        w = window
        if w is None and wl < n_fft:
            w = torch.ones(wl, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            return E.stft_forward(x, w, int(n_fft), hop, int(n_fft) // 2 if center else 0, pad_mode, power, bool(normalized))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = _torch_stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided)
    return _to_power(y, power)


def stft(x: Tensor, n_fft: int, hop_length: int | None = None, win_length: int | None = None, window: Tensor | None = None,
         center: bool = True, pad_mode: str = "reflect", normalized: bool = False, onesided: bool = True) -> Tensor:
    """``torch.stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, return_complex=True)`` for
    ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 -> complex64, float64 -> complex128): ``[..., n_fft // 2 + 1, frames]`` with
    ``frames = 1 + (T + 2 pad - n_fft) // hop``, a transposed view of a contiguous ``[..., frames, bins]`` buffer.
    ``window=None`` is rectangular, a window shorter than ``n_fft`` is centred in zeros, and the window is applied in the signal's
    dtype: one rounded product per sample, then the transform.  On the device route a non-finite sample makes exactly the frames
    that hold it non-finite in every bin (an Inf turns into NaN on the way) and leaves every other frame's bits alone."""
    return _stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided, None)


def spectrogram(x: Tensor, n_fft: int = 1024, hop_length: int | None = None, win_length: int | None = None,
                window: Tensor | str = "hann", power: float | None = 2.0, center: bool = True, pad_mode: str = "reflect",
                normalized: bool = False) -> Tensor:
    """``|stft(x)| ** power`` for ``power`` 1.0 or 2.0 (real, the signal's dtype), the complex STFT itself for ``power=None``.
    ``window`` is a tensor or "hann" / "hamming" / "rect" (:func:`named_window` over ``win_length``).  On the device route the
    magnitude or power is formed in registers from the complex value -- ``re * re + im * im`` and its square root -- and the
    complex spectrum is never stored."""
    if power is not None:
        if isinstance(power, bool) or not isinstance(power, (int, float)) or float(power) not in (1.0, 2.0):
            raise ValueError(f"spectrogram: power must be None, 1.0 or 2.0, got {power!r}")
        power = float(power)
    if isinstance(window, str):
        wl = int(win_length) if win_length is not None else int(n_fft)
        if not isinstance(x, Tensor):
            raise TypeError(f"spectrogram: expected a tensor, got {type(x).__name__}")
        window = named_window(window, wl, x.dtype if x.dtype.is_floating_point else torch.float32, x.device)
    return _stft(x, n_fft, hop_length, win_length, window, center, pad_mode, normalized, True, power)


def _torch_istft(X: Tensor, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex) -> Tensor:
    """``torch.istft`` itself; the one thing added is a ``[B, C, bins, frames]`` input, whose leading axes it takes as rows."""
    lead = None
    if isinstance(X, Tensor) and X.dim() == 4:
        lead, X = X.shape[:2], X.reshape((-1,) + tuple(X.shape[-2:]))
    y = torch.istft(X, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex)
    return y if lead is None else y.unflatten(0, tuple(lead))


def _check_istft(X: Tensor, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex):
    """The argument checks of ``torch.istft``, in its order, with its exception types and the telling part of its messages.
    ``torch.istft`` cannot be asked on tensors without storage (its envelope check reads a value), so the device route checks
    for itself.  Returns ``(hop, win_length, onesided, output length)`` as torch resolves the defaults."""
    if not X.is_complex():
        raise RuntimeError("istft requires a complex-valued input tensor matching the output from stft with return_complex=True.")
    if window is not None and window.is_complex() and not return_complex:
        raise RuntimeError("Complex windows are incompatible with return_complex=False")
    n_fft = int(n_fft)
    hop = int(hop_length) if hop_length is not None else n_fft >> 2
    wl = int(win_length) if win_length is not None else n_fft
    if X.dim() < 2:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-(X.dim() + 1)}, {X.dim()}], but got -3)")
    one = bool(onesided) if onesided is not None else X.shape[-2] != n_fft
    if return_complex and one:
        raise RuntimeError("Cannot have onesided output if window or input is complex")
    what = (f"istft({tuple(X.shape)}, n_fft={n_fft}, hop_length={hop}, win_length={wl}, window={None if window is None else tuple(window.shape)}, "
            f"center={int(bool(center))}, normalized={int(bool(normalized))}, onesided={onesided}, length={length}, "
            f"return_complex={int(bool(return_complex))})")
    if X.numel() == 0:
        raise RuntimeError(f"{what} : input tensor cannot be empty.")
    if X.dim() > 4:
        raise RuntimeError(f"{what} : expected a tensor with 3 or 4 dimensions, but got {X.dim() + 1}")
    if X.shape[-2] != (n_fft // 2 + 1 if one else n_fft):
        raise RuntimeError(f"{what} : expected the frequency dimension (3rd to the last) of the input tensor to match "
                           f"{'n_fft / 2 + 1 when onesided=True' if one else 'n_fft when onesided=False'}, but got {X.shape[-2]}")
    if not 0 < hop <= wl:
        raise RuntimeError(f"{what} : expected 0 < hop_length <= win_length")
    if not 0 < wl <= n_fft:
        raise RuntimeError(f"{what} : expected 0 < win_length <= n_fft")
    if window is not None and (window.dim() != 1 or window.shape[0] != wl):
        raise RuntimeError(f"{what} : Invalid window shape. window has to be 1D and length of `win_length`")
    T = int(length) if length is not None else (X.shape[-1] - 1) * hop + n_fft - (2 * (n_fft // 2) if center else 0)
    if T <= 0:      # torch fails here too, inside its envelope check
        raise RuntimeError(f"{what} : no output sample is left (min(): Expected reduction dim to be specified for input.numel() == 0)")
    return hop, wl, one, T


def _on_istft_route(X: Tensor, n_fft: int, hop: int, wl: int, window: Tensor | None, center: bool, onesided: bool, length,
                    return_complex: bool) -> bool:
    if not X.is_cuda or X.dtype not in (torch.complex64, torch.complex128) or return_complex or not onesided:
        return False
    real = torch.float32 if X.dtype == torch.complex64 else torch.float64
    if window is not None and (window.dtype != real or window.device != X.device):
        return False
    rows = X.numel() // (X.shape[-1] * X.shape[-2])
    return E.istft_plan_info(n_fft, hop, wl, X.shape[-1], rows, real, center, length, True)["route"] == "lds"


def istft(X: Tensor, n_fft: int, hop_length: int | None = None, win_length: int | None = None, window: Tensor | None = None,
          center: bool = True, normalized: bool = False, onesided: bool | None = None, length: int | None = None,
          return_complex: bool = False) -> Tensor:
    """``torch.istft(X, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex)`` over the
    last two axes of ``X [bins, frames]``, ``[C, bins, frames]`` or ``[B, C, bins, frames]`` (complex64 -> float32, complex128 ->
    float64): ``[..., T]`` with ``T = length`` or ``(frames - 1) hop + n_fft - 2 pad`` (``pad = n_fft // 2`` when centred).

    Frame ``f`` is ``s_f = irfft(X[..., :, f], n_fft)`` (scaled by ``1 / n_fft``, ``n_fft ** -0.5`` when ``normalized``; the
    imaginary parts of bins 0 and ``n_fft / 2`` are not read), ``w`` the window centred in ``n_fft`` zeros (None: ones), and
    ``y[t - pad] = sum_f fl(w s_f)[t - f hop] / sum_f fl(w w)[t - f hop]``, both sums over the frames that cover ``t`` in ascending
    frame order, in the signal's dtype.  Positions past the last frame read 0.  Where the envelope does not exceed ``1e-11`` in
    the returned range the call raises ``RuntimeError`` ("window overlap add min"), as torch does; like torch it synchronises
    once to know (``torchfx_ext.istft_forward`` returns the flag unread).

    On the device route the kernel reads the layout :func:`stft` returns (which ``X * mask`` keeps) in place; any other layout
    costs one copy into it first.  A non-finite bin makes exactly the samples its frame covers non-finite -- also under a zero of
    the window -- and leaves every other sample's bits alone.  ``onesided=False``, ``return_complex=True``, other ``n_fft`` and
    CPU tensors take ``torch.istft`` on the tensor's own device."""
    if not isinstance(X, Tensor):
        raise TypeError(f"istft: expected a tensor, got {type(X).__name__}")
    if not X.is_cuda:
        return _torch_istft(X, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex)
    hop, wl, one, _ = _check_istft(X, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex)
    if _on_istft_route(X, int(n_fft), hop, wl, window, bool(center), one, length, bool(return_complex)):
        w = window
        if w is None and wl < n_fft:
            w = torch.ones(wl, dtype=torch.float32 if X.dtype == torch.complex64 else torch.float64, device=X.device)
        with torch.cuda.device(X.device):
            y, flag = E.istft_forward(X, w, int(n_fft), hop, int(n_fft) // 2 if center else 0, length, bool(normalized))
            if int(flag.item()):
                raise RuntimeError(f"istft({tuple(X.shape)}, n_fft={int(n_fft)}, hop_length={hop}, win_length={wl}, center={int(bool(center))}, "
                                   f"length={length}) window overlap add min: 1")
        return y
    return _torch_istft(X, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex)


def _hz_to_mel(f, mel_scale: str):
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1000.0) / 1000.0) / math.log(6.4))


def _mel_to_hz(m, mel_scale: str):
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp(math.log(6.4) * (np.maximum(m, 15.0) - 15.0) / 27.0))


def _mel_design(n_freqs, sample_rate, n_mels, f_min, f_max, norm, mel_scale) -> np.ndarray:
    """The mel filterbank ``[n_freqs, n_mels]`` in float64, after the argument checks."""
    if int(n_mels) < 1:
        raise ValueError(f"n_mels must be at least 1, got {n_mels!r}")
    nyquist = float(sample_rate) / 2.0
    f_max = nyquist if f_max is None else float(f_max)
    if not 0.0 <= float(f_min) < f_max:
        raise ValueError(f"f_min must satisfy 0 <= f_min < f_max, got f_min {f_min!r} and f_max {f_max!r}")
    if f_max > nyquist:
        raise ValueError(f"f_max must not exceed sample_rate / 2 = {nyquist}, got {f_max!r}")
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be None or 'slaney', got {norm!r}")
    if mel_scale not in ("htk", "slaney"):
        raise ValueError(f"mel_scale must be 'htk' or 'slaney', got {mel_scale!r}")
    all_freqs = np.linspace(0.0, nyquist, int(n_freqs))
    f_pts = _mel_to_hz(np.linspace(_hz_to_mel(float(f_min), mel_scale), _hz_to_mel(f_max, mel_scale), int(n_mels) + 2), mel_scale)
    down = (all_freqs[:, None] - f_pts[None, :-2]) / (f_pts[1:-1] - f_pts[:-2])
    up = (f_pts[None, 2:] - all_freqs[:, None]) / (f_pts[2:] - f_pts[1:-1])
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:] - f_pts[:-2]))
    return fb


def mel_filterbank(n_freqs: int, sample_rate: float, n_mels: int = 128, f_min: float = 0.0, f_max: float | None = None,
                   norm: str | None = None, mel_scale: str = "htk", dtype: torch.dtype = torch.float32, device=None) -> Tensor:
    """The triangular mel filterbank ``[n_freqs, n_mels]`` (``torchaudio.functional.melscale_fbanks`` for even integer rates),
    built in float64 on the host and rounded once to ``dtype``.  With ``all_freqs = linspace(0, sample_rate / 2, n_freqs)`` and
    ``f_pts = mel_to_hz(linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2))`` (``f_max=None``: ``sample_rate / 2``) column
    ``m`` is ``max(0, min((f - f_pts[m]) / (f_pts[m+1] - f_pts[m]), (f_pts[m+2] - f) / (f_pts[m+2] - f_pts[m+1])))``, times
    ``2 / (f_pts[m+2] - f_pts[m])`` for ``norm="slaney"``.  ``mel_scale`` "htk": ``mel = 2595 log10(1 + f / 700)``; "slaney":
    ``3 f / 200`` below 1000 Hz and ``15 + 27 ln(f / 1000) / ln 6.4`` from there.  A filter narrower than the bin spacing can be
    an all-zero column."""
    return torch.from_numpy(_mel_design(n_freqs, sample_rate, n_mels, f_min, f_max, norm, mel_scale)).to(dtype=dtype, device=device)


class _Bank:
    """A filterbank prepared for both routes: the float64 design (or the caller's tensor), its dense form per dtype and device
    and its host band table per dtype, each built on first use."""

    def __init__(self, design: np.ndarray | None = None, tensor: Tensor | None = None) -> None:
        self.design, self.tensor = design, tensor
        self.n_filters = int(design.shape[1] if design is not None else tensor.shape[1])
        self._dense: dict = {}
        self._tables: dict = {}

    def dense(self, dtype: torch.dtype, device) -> Tensor:
        key = (dtype, torch.device(device))
        if key not in self._dense:
            src = torch.from_numpy(self.design) if self.design is not None else self.tensor
            self._dense[key] = src.to(dtype=dtype, device=device)
        return self._dense[key]

    def fits(self, x: Tensor) -> bool:
        """The route's condition on a caller's tensor: the signal's dtype and device (the design is rounded to any dtype)."""
        return self.design is not None or (self.tensor.dtype == x.dtype and self.tensor.device == x.device)

    def table(self, dtype: torch.dtype) -> tuple[Tensor, int]:
        """``torchfx_ext.mel_band_table`` of the bank rounded to ``dtype``; a caller's device tensor costs one device-to-host copy."""
        if dtype not in self._tables:
            host = self.design if self.design is not None else self.tensor.detach().cpu().numpy()
            self._tables[dtype] = E.mel_band_table(host.astype(np.float32 if dtype == torch.float32 else np.float64))
        return self._tables[dtype]


def _mel_log(v: Tensor, log: str, power: float, amin: float) -> Tensor:
    v = torch.where(v < amin, torch.full_like(v, amin), v)              # not clamp: a NaN stays
    if log == "ln":
        return v.log()
    return v.log10() * (10.0 if power == 2.0 else 20.0) if log == "db" else v.log10()


class MelSpectrogram:
    """:func:`mel_spectrogram` with everything but the signal fixed: the filterbank and its band table are built once, with the
    object (a ``filterbank=`` tensor on the device costs one device-to-host copy, at the first call on the device route), and
    ``MelSpectrogram(sample_rate, ...)(x)`` has the function's bits.  Not an ``FX``: it returns a tensor."""

    def __init__(self, sample_rate: float, n_fft: int = 1024, hop_length: int | None = None, win_length: int | None = None,
                 window: Tensor | str = "hann", n_mels: int = 128, f_min: float = 0.0, f_max: float | None = None,
                 norm: str | None = None, mel_scale: str = "htk", power: float = 2.0, center: bool = True, pad_mode: str = "reflect",
                 normalized: bool = False, log: str | None = None, amin: float = 1e-10, top_db: float | None = None,
                 filterbank: Tensor | None = None) -> None:
        n_freqs = int(n_fft) // 2 + 1
        design = (n_freqs, float(sample_rate), int(n_mels), float(f_min), None if f_max is None else float(f_max), norm, mel_scale)
        if filterbank is None and design not in E._MEL_BANKS:
            fb = _mel_design(*design)
        if isinstance(power, bool) or not isinstance(power, (int, float)) or float(power) not in (1.0, 2.0):
            raise ValueError(f"power must be 1.0 or 2.0, got {power!r}")
        if log not in E.MEL_LOGS:
            raise ValueError(f"log must be None, 'db', 'log10' or 'ln', got {log!r}")
        if not float(amin) > 0.0:
            raise ValueError(f"amin must be positive, got {amin!r}")
        if top_db is not None and not float(top_db) >= 0.0:
            raise ValueError(f"top_db must not be negative, got {top_db!r}")
        if filterbank is not None:
            if not isinstance(filterbank, Tensor) or filterbank.dim() != 2 or filterbank.shape[0] != n_freqs or filterbank.shape[1] < 1 \
                    or not filterbank.dtype.is_floating_point:
                raise ValueError(f"filterbank must be a real [n_fft / 2 + 1 = {n_freqs}, n_filters] tensor, got "
                                 f"{tuple(filterbank.shape) if isinstance(filterbank, Tensor) else type(filterbank).__name__}")
            self.bank = _Bank(tensor=filterbank)
        else:
            if design not in E._MEL_BANKS:
                if len(E._MEL_BANKS) >= 64:
                    E._MEL_BANKS.clear()
                E._MEL_BANKS[design] = _Bank(design=fb)
            self.bank = E._MEL_BANKS[design]
        self.n_fft, self.hop_length, self.win_length, self.window = int(n_fft), hop_length, win_length, window
        self.power, self.center, self.pad_mode, self.normalized = float(power), bool(center), pad_mode, bool(normalized)
        self.log, self.amin, self.top_db = log, float(amin), None if top_db is None else float(top_db)

    def __call__(self, x: Tensor) -> Tensor:
        if not isinstance(x, Tensor):
            raise TypeError(f"mel_spectrogram: expected a tensor, got {type(x).__name__}")
        n_fft, bank = self.n_fft, self.bank
        hop = int(self.hop_length) if self.hop_length is not None else n_fft // 4
        wl = int(self.win_length) if self.win_length is not None else n_fft
        window = self.window
        if isinstance(window, str):
            window = named_window(window, wl, x.dtype if x.dtype.is_floating_point else torch.float32, x.device)
        y = None
        if x.is_cuda and bank.fits(x):
            _check_as_torch(x, n_fft, hop, wl, window, self.center, self.pad_mode, self.normalized, True)
            if _on_lds_route(x, n_fft, hop, wl, window, self.center, self.pad_mode, True):
                table, total = bank.table(x.dtype)
                rows = x.numel() // x.shape[-1]
                info = E.mel_plan_info(n_fft, hop, wl, x.shape[-1], rows, x.dtype, self.center, self.pad_mode, bank.n_filters, total)
                if info["route"] == "lds":
                    w = window
                    if w is None and wl < n_fft:
                        w = torch.ones(wl, dtype=x.dtype, device=x.device)
                    with torch.cuda.device(x.device):
                        y = E.mel_forward(x, w, table, bank.n_filters, n_fft, hop, n_fft // 2 if self.center else 0, self.pad_mode,
                                          self.power, self.normalized, self.log, self.amin)
        if y is None:
            P = spectrogram(x, n_fft, self.hop_length, self.win_length, window, self.power, self.center, self.pad_mode, self.normalized)
            y = torch.matmul(P.transpose(-1, -2), bank.dense(P.dtype, P.device)).transpose(-1, -2)
            if self.log is not None:
                y = _mel_log(y, self.log, self.power, self.amin)
        if self.log == "db" and self.top_db is not None:
            item = y if y.dim() <= 3 else y.flatten(1)
            peak = item.amax() if y.dim() <= 3 else item.amax(dim=1).view(-1, 1, 1, 1)
            y = torch.maximum(y, peak - self.top_db)
        return y


def mel_spectrogram(x: Tensor, sample_rate: float, n_fft: int = 1024, hop_length: int | None = None, win_length: int | None = None,
                    window: Tensor | str = "hann", n_mels: int = 128, f_min: float = 0.0, f_max: float | None = None,
                    norm: str | None = None, mel_scale: str = "htk", power: float = 2.0, center: bool = True, pad_mode: str = "reflect",
                    normalized: bool = False, log: str | None = None, amin: float = 1e-10, top_db: float | None = None,
                    filterbank: Tensor | None = None) -> Tensor:
    """The mel spectrogram ``[..., n_mels, frames]`` of ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64, the result's
    dtype), the transposed view of a contiguous ``[..., frames, n_mels]`` buffer.  With ``P = spectrogram(x, n_fft, hop_length,
    win_length, window, power, center, pad_mode, normalized)`` (``power`` 1.0 or 2.0) and ``fb = mel_filterbank(n_fft // 2 + 1,
    sample_rate, n_mels, f_min, f_max, norm, mel_scale, x.dtype)``: ``mel[f, m] = sum_k fb[k, m] P[f, k]`` over the filter's band,
    in the signal's dtype.  ``log`` "db" gives ``c log10(v')`` with ``c`` 10 (``power=2``) or 20 (``power=1``), "log10"
    ``log10(v')`` and "ln" ``ln(v')``, where ``v' = v < amin ? amin : v`` (a NaN passes the floor).  ``top_db`` with ``log="db"``
    raises everything to ``y.amax() - top_db``, the maximum taken over each ``[C, T]`` signal or batch item (two torch ops on
    the small result, no host synchronisation).  ``filterbank=`` takes any real ``[n_fft // 2 + 1, n_filters]`` tensor in place
    of the mel design (negative weights allowed); ``ValueError`` names a bad argument.

    On a ROCm device one launch reads the signal once and writes only the result; the power spectrum has :func:`spectrogram`'s
    bits and never reaches global memory.  The mel design's band table is cached by its parameters
    (``torchfx_ext.clear_caches`` drops it); a ``filterbank=`` tensor builds its table per call, which on the device costs one
    device-to-host copy -- :class:`MelSpectrogram` pays it once.  A frame's bits depend on its ``n_fft`` samples, the window and
    the filterbank alone (the same with and without ``log``); a non-finite sample makes exactly the frames that hold it non-finite
    in every filter with a non-empty band; an all-zero filter reads exactly 0, the ``amin`` floor with ``log``.  Served:
    :func:`stft`'s device geometries with at most 256 filters whose bands fit LDS and a ``filterbank`` of the signal's dtype and
    device; everything else (CPU tensors, ``n_fft=400``, dense banks) is ``spectrogram``, ``matmul(P.transpose(-1, -2),
    fb).transpose(-1, -2)`` and the logarithm in torch ops on the tensor's own device."""
    return MelSpectrogram(sample_rate, n_fft, hop_length, win_length, window, n_mels, f_min, f_max, norm, mel_scale, power, center,
                          pad_mode, normalized, log, amin, top_db, filterbank)(x)


def _vocoder_rate(rate, what: str = "phase_vocoder") -> float:
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not math.isfinite(rate) or not rate > 0:
        raise ValueError(f"{what}: rate must be a finite number > 0, got {rate!r}")
    return float(rate)


def _lock_served(what: str, bins: int, dtype: torch.dtype) -> None:
    """``ValueError`` where the device's locked route does not serve ``bins``: the plan's own answer, asked before any launch."""
    try:
        E.phase_vocoder_plan_info(1, bins, 1.0, 1, dtype, 0, 1)
    except RuntimeError as e:
        raise ValueError(f"{what}: {e}") from None


def _vocoder_lock(phase_lock, what: str = "phase_vocoder") -> int:
    """``phase_lock`` as the native ``lock`` code: ``None`` 0, ``"identity"`` 1."""
    if phase_lock is None:
        return 0
    if phase_lock != "identity":
        raise ValueError(f'{what}: phase_lock must be None or "identity", got {phase_lock!r}')
    return 1


def _locked_phase(A: np.ndarray, mag: np.ndarray, i: np.ndarray) -> np.ndarray:
    """Identity phase locking, frame by frame: ``A [..., bins, F + 2]`` (uint64 turns), ``mag [..., bins, Fo]`` in the real dtype
    -> ``phi [..., bins, Fo]`` (uint64)."""
    bins = A.shape[-2]
    k = np.arange(bins)
    phi = np.empty(mag.shape, np.uint64)
    U = A[..., 0].copy()                                                 # the plain update of the frame to come
    for t in range(len(i)):
        m = mag[..., t]
        peak = np.ones(m.shape, bool)
        for s in (1, 2):                                                 # strictly above every in-range neighbour; a NaN compares false
            peak[..., s:] &= m[..., s:] > m[..., :-s]
            peak[..., :-s] &= m[..., :-s] > m[..., s:]
        lo = np.maximum.accumulate(np.where(peak, k, -1), axis=-1)       # the nearest peak at or below, -1: none
        hi = np.minimum.accumulate(np.where(peak, k, bins)[..., ::-1], axis=-1)[..., ::-1]      # at or above, bins: none
        near = np.where(lo < 0, np.where(hi == bins, k, hi), np.where((hi == bins) | (k - lo <= hi - k), lo, hi))
        A0 = A[..., i[t]]
        phi[..., t] = np.take_along_axis(U - A0, near, axis=-1) + A0     # U[P] + (A[i, k] - A[i, P]); no peak: U[k]
        U = phi[..., t] + (A[..., i[t] + 1] - A0)
    return phi


def _vocoder_host(X: np.ndarray, rate: float, lock: int = 0) -> np.ndarray:
    """The definition of :func:`phase_vocoder` on a host array ``[..., bins, F]``, with the device's fixed-point phase."""
    real = np.float32 if X.dtype == np.complex64 else np.float64
    F = X.shape[-1]
    Fo = int(math.ceil(F / rate))
    pos = np.arange(Fo, dtype=np.float64) * rate
    i = np.floor(pos).astype(np.int64)
    alpha = (pos - i).astype(real)
    Xp = np.concatenate([X, np.zeros(X.shape[:-1] + (2,), dtype=X.dtype)], axis=-1)          # frames F and F + 1 are zeros
    re, im = Xp.real.astype(np.float64), Xp.imag.astype(np.float64)
    finite = np.isfinite(re) & np.isfinite(im)
    with np.errstate(invalid="ignore", over="ignore"):
        turns = np.where(finite & ((re != 0) | (im != 0)), np.arctan2(im, re) * 0.15915494309189535, 0.0)
        w = np.rint(turns * 2.0 ** 64)
        A = np.where(w >= 2.0 ** 63, w - 2.0 ** 64, w).astype(np.int64).view(np.uint64)      # 2^64 = one turn
        inc = A[..., i + 1] - A[..., i]                                                      # wraps, as the sum does
        M = np.abs(Xp).astype(real)
        mag = alpha * M[..., i + 1] + (real(1) - alpha) * M[..., i]
        if lock:
            P = _locked_phase(A, mag, i)
        else:
            P = A[..., :1] + np.concatenate([np.zeros_like(inc[..., :1]), np.cumsum(inc, axis=-1, dtype=np.uint64)[..., :-1]], axis=-1)
        ang = P.view(np.int64).astype(np.float64) * (math.pi * 2.0 ** -63)                   # [-pi, pi]
        mag = mag.astype(np.float64)
        Y = (mag * np.cos(ang) + 1j * (mag * np.sin(ang))).astype(X.dtype)
    bad = np.logical_or.accumulate(~(finite[..., i] & finite[..., i + 1]), axis=-1)
    if lock:                                                             # the paths couple the bins: the poison is the row's
        bad = np.broadcast_to(bad.any(axis=-2, keepdims=True), bad.shape)
    Y[bad] = complex(np.nan, np.nan)
    return Y


@torch.no_grad()
def phase_vocoder(X: Tensor, rate: float, phase_advance: Tensor | None = None, phase_lock: str | None = None) -> Tensor:
    """``torchaudio.functional.phase_vocoder(X, rate, phase_advance)``: the spectrum ``X [bins, F]``, ``[C, bins, F]`` or
    ``[B, C, bins, F]`` (complex64 / complex128) sped up by ``rate > 0`` (a Python float) without a change of pitch:
    ``[..., bins, Fo]`` with ``Fo = ceil(F / rate)``, computed in double as ``torch.arange(0, F, rate)`` sizes itself.

    Output frame ``t`` stands at ``p = t rate`` (double), ``i = floor(p)``, ``alpha = p - i`` rounded once to the real dtype;
    input frames ``F`` and ``F + 1`` are zeros (torchaudio's padding).  ``mag[t] = alpha |X[i+1]| + (1 - alpha) |X[i]|`` in the
    real dtype, ``phase[t] = angle(X[0]) + sum_{s<t} (angle(X[i_s + 1]) - angle(X[i_s]))`` and ``Y[t] = polar(mag[t], phase[t])``,
    formed in double and rounded once.  torchaudio adds ``wrap(d - pa) + pa`` per step, with ``pa`` the expected advance
    ``phase_advance``: that differs from ``d`` by whole turns and only ``phase mod 2 pi`` reaches ``Y``, so **``phase_advance``
    drops out of the result**.  It is accepted for compatibility (torchaudio's default is ``linspace(0, pi hop, bins)[..., None]``),
    checked to be a real ``[bins, 1]`` tensor when given, and changes nothing.

    The phase is kept in turns as 64-bit fixed point: each bin's angle once, ``A = rint(atan2(im, re) / 2 pi * 2^64)`` in
    float64 (0 for the zero bin), and the sum in wrapping integers -- exact however long the signal, equal to ``A[t]`` at
    ``rate=1``, and the same bits whatever the segment count, the other rows or the batch.  From the first output frame that
    reads a bin with a NaN or Inf component every later frame of that (row, bin) is NaN in both parts; earlier frames, other
    bins and other rows keep their bits.

    ``phase_lock="identity"`` locks the phases around each spectral peak (Laroche & Dolson 1999, identity phase locking), which
    takes the plain vocoder's smeared, reverberant colour away.  With ``U[t,k] = phase[t-1,k] + (A[i_{t-1}+1,k] - A[i_{t-1},k])``
    the plain update (``U[0] = A[0]``), bin ``k`` is a peak of frame ``t`` iff ``mag[t,k] > mag[t,j]``, strictly, for every
    in-range ``j`` in ``{k-2, k-1, k+1, k+2}`` (a comparison with a NaN is false; a single bin is a peak), ``P(k)`` is the peak
    nearest to ``k`` (the lower one at equal distance), and ``phase[t,k] = U[t,P(k)] + (A[i_t,k] - A[i_t,P(k)])``: a peak keeps its
    own update, every other bin the analysis frame's phase relation to its peak.  A frame without a peak (silence, a flat frame)
    keeps ``U``.  The same integer phase: at ``rate=1`` the result is bit-identical to the plain one, and so is a spectrum without
    peaks at any rate; the bits do not depend on the segment count, the other rows or the batch.  The paths couple a row's bins,
    so from the first output frame that reads a NaN or Inf bin **every bin** of every later frame of that row is NaN, that frame
    included.  The device serves up to 4097 bins (``n_fft=8192``) this way; more raise ``ValueError``.  Any other value of
    ``phase_lock`` raises ``ValueError``; scaled locking is not provided.

    Device tensors take ``torchfx_amd/csrc/phasevocoder.hip`` (``torchfx_ext.phase_vocoder_forward``), which reads the layout
    :func:`stft` returns in place and writes the one :func:`istft` reads; CPU tensors run the same definition in NumPy with the
    same integer phase.  There is no other route.  ``ValueError`` names a bad argument."""
    if not isinstance(X, Tensor) or X.dtype not in (torch.complex64, torch.complex128) or X.dim() not in (2, 3, 4):
        got = f"{X.dtype} {tuple(X.shape)}" if isinstance(X, Tensor) else type(X).__name__
        raise ValueError(f"phase_vocoder: X must be a complex64 / complex128 tensor [bins, F], [C, bins, F] or [B, C, bins, F], got {got}")
    rate = _vocoder_rate(rate)
    lock = _vocoder_lock(phase_lock)
    if phase_advance is not None:
        if not isinstance(phase_advance, Tensor) or phase_advance.is_complex() or not phase_advance.dtype.is_floating_point \
                or tuple(phase_advance.shape) != (X.shape[-2], 1):
            got = tuple(phase_advance.shape) if isinstance(phase_advance, Tensor) else type(phase_advance).__name__
            raise ValueError(f"phase_vocoder: phase_advance must be a real [bins, 1] = [{X.shape[-2]}, 1] tensor, got {got}")
    if X.is_cuda:
        if lock:
            _lock_served("phase_vocoder", X.shape[-2], X.dtype)
        with torch.cuda.device(X.device):
            return E.phase_vocoder_forward(X, rate, 0, lock)
    return torch.from_numpy(_vocoder_host(X.detach().numpy(), rate, lock))


def _stretch_geometry(what: str, x: Tensor, n_fft, hop_length, win_length, window, length: int | None = None):
    """The checks of a stretch of ``x`` (rows of ``length`` samples, default x's) and its resolved ``(n_fft, hop, win_length,
    window)``."""
    if not isinstance(x, Tensor) or x.dtype not in (torch.float32, torch.float64) or x.dim() not in (1, 2, 3) or x.shape[-1] < 1:
        got = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, Tensor) else type(x).__name__
        raise ValueError(f"{what}: x must be a float32 / float64 tensor [T], [C, T] or [B, C, T] with T >= 1, got {got}")
    n_fft = int(n_fft)
    hop = int(hop_length) if hop_length is not None else n_fft // 4
    wl = int(win_length) if win_length is not None else n_fft
    if n_fft < 2 or not 0 < wl <= n_fft or not 0 < hop <= wl:
        raise ValueError(f"{what}: need n_fft >= 2 and 0 < hop_length <= win_length <= n_fft, got n_fft {n_fft}, hop_length {hop}, "
                         f"win_length {wl}")
    T = int(x.shape[-1]) if length is None else int(length)
    if T <= n_fft // 2:
        raise ValueError(f"{what}: x must be longer than n_fft / 2 = {n_fft // 2} samples (the reflected edge), got {T}")
    if isinstance(window, str):
        window = named_window(window, wl, x.dtype, x.device)
    elif not isinstance(window, Tensor) or tuple(window.shape) != (wl,) or window.dtype != x.dtype or window.device != x.device:
        got = f"{window.dtype} {tuple(window.shape)} on {window.device}" if isinstance(window, Tensor) else type(window).__name__
        raise ValueError(f"{what}: window must be a name or a [win_length = {wl}] tensor of x's dtype and device ({x.dtype} on "
                         f"{x.device}), got {got}")
    return n_fft, hop, wl, window


@torch.no_grad()
def time_stretch(x: Tensor, rate: float, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None,
                 window: Tensor | str = "hann", phase_lock: str | None = None) -> Tensor:
    """Change the tempo of ``x [T]``, ``[C, T]`` or ``[B, C, T]`` by ``rate`` and keep its pitch: ``istft(phase_vocoder(stft(x),
    rate), length=round(T / rate))`` with a centred, reflected :func:`stft` (``hop_length`` defaults to ``n_fft // 4``,
    ``window`` is a tensor or a name of :func:`named_window`).  ``rate > 1`` is faster and shorter.  On a ROCm device with
    ``n_fft`` in 256 ... 4096 that is three kernels and no copy between them: the vocoder reads the buffer the transform wrote
    and the inverse reads the buffer the vocoder wrote.  ``phase_lock="identity"`` is :func:`phase_vocoder`'s: phases locked to the
    spectral peaks, the same three kernels with the locked vocoder in the middle."""
    rate = _vocoder_rate(rate, "time_stretch")
    lock = _vocoder_lock(phase_lock, "time_stretch")
    n_fft, hop, wl, window = _stretch_geometry("time_stretch", x, n_fft, hop_length, win_length, window)
    if lock and x.is_cuda:
        _lock_served("time_stretch", n_fft // 2 + 1, x.dtype)             # before the transform runs
    Y = phase_vocoder(stft(x, n_fft, hop, wl, window), rate, phase_lock=phase_lock)
    return istft(Y, n_fft, hop, wl, window, length=int(round(x.shape[-1] / rate)))


def _pitch_ratio(n_steps, bins_per_octave) -> tuple[float, int, int]:
    """``(r, up, down)``: the stretch rate ``r = 2 ** (-n_steps / bins_per_octave)`` and, with ``down / up`` the rational
    approximation of ``1 / r`` (``Fraction(1 / r).limit_denominator(1000)``), the ``resample_poly(up, down)`` that brings the
    stretched ``T / r`` samples back to ``T``."""
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, float)) or not math.isfinite(n_steps):
        raise ValueError(f"pitch_shift: n_steps must be a finite number, got {n_steps!r}")
    if isinstance(bins_per_octave, bool) or not isinstance(bins_per_octave, int) or bins_per_octave < 1:
        raise ValueError(f"pitch_shift: bins_per_octave must be an integer >= 1, got {bins_per_octave!r}")
    r = 2.0 ** (-float(n_steps) / bins_per_octave)
    q = fractions.Fraction(1.0 / r).limit_denominator(1000)
    if q <= 0:
        raise ValueError(f"pitch_shift: n_steps {n_steps!r} is out of range")
    return r, q.denominator, q.numerator


@torch.no_grad()
def pitch_shift(x: Tensor, n_steps: float, bins_per_octave: int = 12, n_fft: int = 2048, hop_length: int | None = None,
                win_length: int | None = None, window: Tensor | str = "hann", phase_lock: str | None = None) -> Tensor:
    """Shift the pitch of ``x [T]``, ``[C, T]`` or ``[B, C, T]`` by ``n_steps`` steps of ``bins_per_octave`` to the octave
    (12: semitones) and keep length and rate: with ``r = 2 ** (-n_steps / bins_per_octave)``, :func:`time_stretch` by ``r``,
    then ``resample_poly(up, down)`` with ``down / up`` the rational approximation of ``1 / r``
    (``fractions.Fraction(1 / r).limit_denominator(1000)``: that many input samples per output sample, so ``T / r`` samples
    come back to ``T``), then the result is trimmed or zero-padded to ``T``.  ``phase_lock`` is :func:`time_stretch`'s."""
    r, up, down = _pitch_ratio(n_steps, bins_per_octave)
    _vocoder_lock(phase_lock, "pitch_shift")
    from torchfx_amd.resample import resample_poly

    T = x.shape[-1] if isinstance(x, Tensor) and x.dim() else 0
    y = resample_poly(time_stretch(x, r, n_fft, hop_length, win_length, window, phase_lock), up, down)
    if y.shape[-1] >= T:
        return y[..., :T].contiguous()
    return torch.nn.functional.pad(y, (0, T - y.shape[-1]))


class TimeStretch(FX):
    """:func:`time_stretch` as an effect: ``wave | TimeStretch(0.8)`` is a ``Wave`` of ``round(T / rate)`` samples at the same
    ``fs``.  A whole-signal effect that changes the length: the planner keeps it as a step of its own, and
    ``StreamProcessor`` and ``RealtimeProcessor`` refuse it.  ``phase_lock="identity"`` locks the phases to the spectral peaks
    (:func:`phase_vocoder`)."""

    def __init__(self, rate: float, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None,
                 window: Tensor | str = "hann", phase_lock: str | None = None) -> None:
        super().__init__()
        self.rate = _vocoder_rate(rate, type(self).__name__)
        _vocoder_lock(phase_lock, type(self).__name__)
        self.phase_lock = phase_lock
        self.n_fft, self.hop_length, self.win_length = int(n_fft), hop_length, win_length
        if isinstance(window, Tensor):
            self.register_buffer("window", window, persistent=False)    # moves with the effect (.to)
        else:
            self.window = window

    def _stretch(self) -> float:
        return self.rate

    def output_length(self, length: int) -> int:
        return int(round(int(length) / self.rate))

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (<kernels>, <the vocoder's plan>)`` or ``numpy on host -- <reason>`` for ``x`` (rows of ``length`` samples,
        default x's)."""
        n = int(x.shape[-1]) if length is None else int(length)
        try:
            n_fft, hop, wl, _ = _stretch_geometry(type(self).__name__, x, self.n_fft, self.hop_length, self.win_length, self.window, n)
        except ValueError as e:
            return f"refused -- {e}"
        if not x.is_cuda:
            return f"torch.stft, phase vocoder in numpy, torch.istft on host -- {x.device.type} tensor"
        rows, rate = max(1, x.numel() // max(1, int(x.shape[-1]))), self._stretch()
        fwd = E.stft_plan_info(n_fft, hop, wl, n, rows, x.dtype)
        lock = _vocoder_lock(self.phase_lock)
        try:
            pv = E.phase_vocoder_plan_info(fwd["frames"], n_fft // 2 + 1, rate, rows, x.dtype, 0, lock)
        except RuntimeError as e:                                        # more bins than the locked route serves
            return f"refused -- {e}"
        inv = E.istft_plan_info(n_fft, hop, wl, pv["out_frames"], rows, x.dtype, True, int(round(n / rate)))
        cut = "one launch" if pv["launches"] == 1 else f"summary pass + final pass over {pv['segments']} segments of {pv['seg_frames']} frames"
        if lock:
            vocoder = (f"phase_lock_kernel (identity phase locking, {fwd['frames']} -> {pv['out_frames']} frames, {cut}, {pv['threads']} lanes x "
                       f"{pv['bins_per_thread']} bins, {pv['lds_bytes']} B LDS)")
        else:
            vocoder = f"phase_vocoder_kernel ({fwd['frames']} -> {pv['out_frames']} frames, {cut}, bin tile {pv['bin_tile']})"
        steps = ["stft_kernel" if fwd["route"] == "lds" else "torch.stft", vocoder,
                 "istft_kernel" if inv["route"] == "lds" else "torch.istft"]
        copies = "no layout copy between them" if fwd["route"] == inv["route"] == "lds" else "torch's transforms own their layouts"
        return f"native ({' + '.join(steps + self._last_step(x, int(round(n / rate))))}; {copies})"

    def _last_step(self, x: Tensor, length: int) -> list[str]:
        return []

    def forward(self, x: Tensor) -> Tensor:
        return time_stretch(x, self.rate, self.n_fft, self.hop_length, self.win_length, self.window, self.phase_lock)

    def extra_repr(self) -> str:
        lock = f", phase_lock={self.phase_lock!r}" if self.phase_lock is not None else ""
        return f"rate={self.rate}, n_fft={self.n_fft}, hop_length={self.hop_length}, win_length={self.win_length}{lock}"


class PitchShift(TimeStretch):
    """:func:`pitch_shift` as an effect: ``wave | PitchShift(3)`` is the signal three semitones up, at the same length and
    ``fs``.  A whole-signal effect: the planner keeps it as a step of its own, and ``StreamProcessor`` and
    ``RealtimeProcessor`` refuse it."""

    def __init__(self, n_steps: float, bins_per_octave: int = 12, n_fft: int = 2048, hop_length: int | None = None,
                 win_length: int | None = None, window: Tensor | str = "hann", phase_lock: str | None = None) -> None:
        r, self.up, self.down = _pitch_ratio(n_steps, bins_per_octave)
        super().__init__(r, n_fft, hop_length, win_length, window, phase_lock)
        self.n_steps, self.bins_per_octave = n_steps, bins_per_octave

    def output_length(self, length: int) -> int:
        return int(length)

    def _last_step(self, x: Tensor, length: int) -> list[str]:
        from torchfx_amd.resample import design_taps

        if self.up == self.down:
            return []
        taps = int(design_taps(self.up, self.down, ("kaiser", 5.0), x.dtype).numel())
        return [f"{E.resample_plan_info(length, self.up, self.down, taps, x.dtype)['kernel']} ({self.up} / {self.down})"]

    def forward(self, x: Tensor) -> Tensor:
        return pitch_shift(x, self.n_steps, self.bins_per_octave, self.n_fft, self.hop_length, self.win_length, self.window, self.phase_lock)

    def extra_repr(self) -> str:
        lock = f", phase_lock={self.phase_lock!r}" if self.phase_lock is not None else ""
        return f"n_steps={self.n_steps}, bins_per_octave={self.bins_per_octave}, n_fft={self.n_fft}, hop_length={self.hop_length}{lock}"
