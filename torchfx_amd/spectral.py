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

Not here: ``onesided=False`` and ``return_complex=True`` on the device route, mel / log scaling, streaming forms, autograd, axes
other than the last, round-trip effect classes.
"""
from __future__ import annotations

import re
import warnings

import torch
from torch import Tensor

from torchfx_amd import torchfx_ext as E

__all__ = ["stft", "spectrogram", "istft", "named_window"]

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
