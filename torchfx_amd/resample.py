"""Polyphase rational resampling: :func:`resample_poly` and the :class:`Resample` effect.

The semantics are ``scipy.signal.resample_poly`` (SciPy 1.15) along the last axis, which the reference's guide names as the
way to reconcile two sample rates.  On ROCm device float32 / float64 tensors one HIP launch computes it
(``csrc/resample.hip``, :func:`torchfx_ext.resample_forward`); CPU tensors call SciPy on the host.  The output has the
input's dtype (SciPy returns float64 for a float32 signal with a float64 window array).
"""
from __future__ import annotations

import math
import numbers
import threading
from collections import OrderedDict

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.effect import FX

_TAPS: "OrderedDict[tuple, Tensor]" = OrderedDict()          # (up, down, window key, dtype) -> host taps, scaled by up
_TAPS_LOCK = threading.Lock()
_TAPS_CAP = 64


def _is_window_array(window) -> bool:
    return isinstance(window, (list, np.ndarray, Tensor))


def window_key(window) -> tuple:
    """A hashable key for a window spec (str / tuple) or a 1-D window array (by its bytes)."""
    if _is_window_array(window):
        a = window.detach().cpu().numpy() if isinstance(window, Tensor) else np.asarray(window)
        return ("array", a.dtype.str, a.shape, a.tobytes())
    return ("spec", window)


def _rate(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    if v < 1:
        raise ValueError(f"{name} must be >= 1, got {v}")
    return int(v)


def _reduce(up, down) -> tuple[int, int]:
    up, down = _rate(up, "up"), _rate(down, "down")
    g = math.gcd(up, down)
    return up // g, down // g


def design_taps(up: int, down: int, window=("kaiser", 5.0), dtype: torch.dtype = torch.float32) -> Tensor:
    """The filter ``resample_poly`` runs for reduced ``up / down``, as SciPy builds it: ``firwin(2 * half_len + 1,
    1 / max(up, down), window=window)`` with ``half_len = 10 * max(up, down)`` cast to the signal dtype, or a 1-D window
    array as given; then ``h *= up``.  A host tensor of ``dtype``, cached per ``(up, down, window, dtype)``."""
    key = (up, down, window_key(window), dtype)
    with _TAPS_LOCK:
        h = _TAPS.get(key)
        if h is not None:
            _TAPS.move_to_end(key)
            return h
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    if _is_window_array(window):
        w = window.detach().cpu().numpy() if isinstance(window, Tensor) else window
        h = np.array(w)                                  # a copy, as SciPy makes
        if h.ndim != 1:
            raise ValueError("window must be 1-D")
        if h.size == 0:
            raise ValueError("window must not be empty")
        h *= up
        h = h.astype(np_dtype)
    else:
        from scipy.signal import firwin

        max_rate = max(up, down)
        h = firwin(2 * 10 * max_rate + 1, 1.0 / max_rate, window=window).astype(np_dtype)
        h *= up
    t = torch.from_numpy(np.ascontiguousarray(h))
    with _TAPS_LOCK:
        _TAPS[key] = t
        while len(_TAPS) > _TAPS_CAP:
            _TAPS.popitem(last=False)
    return t


def _check_args(x: Tensor, padtype: str, cval) -> None:
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"resample_poly: float32 or float64 signals only, got {x.dtype}")
    if padtype != "constant":
        raise ValueError(f"resample_poly: padtype {padtype!r} is not supported; only 'constant' (zeros) is")
    if cval is not None and cval != 0:
        raise ValueError(f"resample_poly: cval {cval!r} is not supported; only padding with zeros (cval None or 0) is")
    if x.dim() == 0:
        raise ValueError("resample_poly: x must have a time dimension")


@torch.no_grad()
def resample_poly(x: Tensor, up, down, window=("kaiser", 5.0), padtype: str = "constant", cval=None) -> Tensor:
    """``scipy.signal.resample_poly(x, up, down, axis=-1, window=window, padtype="constant")``.

    ``x [..., T]`` float32 / float64 -> ``[..., ceil(T * up / down)]`` of the same dtype; rows are independent.
    ``up`` and ``down`` are reduced by their gcd, and ``up == down`` returns a copy.  ``window`` is a window spec for
    ``scipy.signal.firwin`` or a 1-D array of filter taps.  Device tensors run the HIP kernel; CPU tensors run SciPy.
    Other dtypes raise ``TypeError``; another ``padtype`` or a nonzero ``cval`` raises ``ValueError``."""
    if not isinstance(x, Tensor):
        raise TypeError(f"resample_poly: x must be a torch.Tensor, got {type(x).__name__}")
    up, down = _reduce(up, down)
    _check_args(x, padtype, cval)
    if up == down == 1:
        return x.clone()
    if not x.is_cuda:
        from scipy.signal import resample_poly as _scipy_resample_poly

        w = window.detach().cpu().numpy() if isinstance(window, Tensor) else window
        y = _scipy_resample_poly(x.detach().numpy(), up, down, axis=-1, window=w, padtype="constant")
        return torch.from_numpy(np.ascontiguousarray(y.astype(x.detach().numpy().dtype, copy=False)))
    from torchfx_amd import torchfx_ext

    h = design_taps(up, down, window, x.dtype)
    with torch.cuda.device(x.device):
        return torchfx_ext.resample_forward(x, up, down, h)


class Resample(FX):
    """Change the sample rate to ``new_fs``: :func:`resample_poly` with ``up / down = new_fs / fs``.

    ``fs`` is the input rate; with ``fs=None`` it comes from the ``Wave`` the effect is piped into.  ``wave | Resample(r)``
    is a ``Wave`` at rate ``r``, and the effects piped after it design their coefficients at ``r``."""

    def __init__(self, new_fs: int, fs: int | None = None, window=("kaiser", 5.0)) -> None:
        super().__init__()
        self.new_fs = _rate(new_fs, "new_fs")
        self.fs = None if fs is None else _rate(fs, "fs")
        self.window = window

    def _ratio(self) -> tuple[int, int]:
        assert self.fs is not None, ("Sample rate (fs) is required for Resample. "
                                     "Either provide fs parameter or use with Wave pipeline (wave | resample).")
        return _reduce(self.new_fs, self.fs)

    @property
    def up(self) -> int:
        return self._ratio()[0]

    @property
    def down(self) -> int:
        return self._ratio()[1]

    def output_length(self, length: int) -> int:
        up, down = self._ratio()
        return -(-int(length) * up // down)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (<kernel>)`` or ``scipy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"scipy on host -- {x.device.type} tensor"
        if x.dtype not in (torch.float32, torch.float64):
            return f"refused -- {x.dtype} signal (float32 / float64 only)"
        from torchfx_amd import torchfx_ext

        up, down = self._ratio()
        if up == down:
            return "native (copy)"
        n = int(x.shape[-1]) if length is None else int(length)
        taps = int(design_taps(up, down, self.window, x.dtype).numel())
        return f"native ({torchfx_ext.resample_plan_info(n, up, down, taps, x.dtype)['kernel']})"

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        up, down = self._ratio()
        return resample_poly(x, up, down, window=self.window)

    def extra_repr(self) -> str:
        return f"new_fs={self.new_fs}, fs={self.fs}"
