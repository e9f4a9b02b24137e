"""Looking at a signal in frequency: the short-time Fourier transform and the spectrogram.

:func:`stft` is ``torch.stft(..., return_complex=True)`` along the last axis -- same defaults, errors, result shape and result
strides -- and :func:`spectrogram` its magnitude or power with a named window.  These are analyses: they return tensors, there is
no ``FX`` class, nothing in the planner and nothing in the stream processors.

On a ROCm device the transform is one launch of ``torchfx_amd/csrc/stft.hip`` (``torchfx_ext.stft_forward``) that reads the signal
once and writes only the result: the centre padding is part of the kernel's addressing, the frames are formed in LDS and each is
transformed on its own, so a frame's bits depend on its ``n_fft`` samples and the window alone.  That route serves ``n_fft`` in
256 ... 4096 (powers of two), ``onesided=True`` and ``pad_mode`` "reflect" / "constant" (any with ``center=False``); every other
geometry, and every CPU tensor, takes ``torch.stft`` on the tensor's own device, so the functions are total.
``torchfx_ext.stft_plan_info`` says which route a geometry takes.

Not here: the inverse (ISTFT), mel / log scaling, a streaming form, autograd, axes other than the last.
"""
from __future__ import annotations

import re
import warnings

import torch
from torch import Tensor

from torchfx_amd import torchfx_ext as E

__all__ = ["stft", "spectrogram", "named_window"]

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
