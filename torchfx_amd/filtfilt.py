"""Zero-phase IIR filtering: :func:`sosfiltfilt`.

The semantics are ``scipy.signal.sosfiltfilt`` (SciPy 1.15) along the last axis: the cascade runs forward over the signal
extended at both ends, then backward over its own output, each pass started from the cascade's steady state for the first
sample it sees, and the extension is dropped -- the result has the squared magnitude response and no phase shift.  On ROCm
device float32 / float64 tensors two launches of the HIP cascade kernel compute it around one float64 intermediate
(``csrc/sos.hip``, :func:`torchfx_ext.sos_filtfilt`): the edge extension and the time reversal are index arithmetic, so no
padded, flipped or widened copy of the signal exists.  CPU tensors call SciPy on the host.  The output has the input's dtype.
"""
from __future__ import annotations

import numbers
from collections import OrderedDict

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.torchfx_ext import PADTYPES, sos_array

_CHECKED: "OrderedDict[bytes, None]" = OrderedDict()         # cascades SciPy's sosfilt_zi has accepted, by content
_CHECKED_CAP = 64


def _check_steady_state(a: np.ndarray) -> None:
    """SciPy's own checks of the cascade (a0 = 1, a steady state exists), once per cascade: its errors propagate."""
    key = a.tobytes()
    if key in _CHECKED:
        return
    from scipy.signal import sosfilt_zi

    sosfilt_zi(a)
    _CHECKED[key] = None
    while len(_CHECKED) > _CHECKED_CAP:
        _CHECKED.popitem(last=False)


def default_padlen(sos: np.ndarray) -> int:
    """SciPy's default: ``3 * (2 K + 1 - min(#(b2 == 0), #(a2 == 0)))``."""
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


def check_pad(padtype, padlen) -> None:
    if padtype not in PADTYPES:
        raise ValueError(f"Unknown value '{padtype}' given to padtype.  padtype must be 'even', 'odd', 'constant', or None.")
    if padlen is not None:
        if isinstance(padlen, bool) or not isinstance(padlen, numbers.Integral):
            raise ValueError(f"padlen must be an integer or None, got {padlen!r}")
        if padlen < 0:
            raise ValueError(f"padlen must be >= 0, got {padlen}")


def padlen_in_force(sos: np.ndarray, padtype, padlen) -> int:
    if padtype is None:
        return 0
    return default_padlen(sos) if padlen is None else int(padlen)


def steady_state_gains(sos) -> np.ndarray:
    """``G[s] = prod_{j < s} sum(b_j) / sum(a_j)`` for ``s = 0 ... K``: the DC gain of the sections in front of section ``s``.
    A DF1 cascade that has seen the constant ``v`` for ever holds ``v * G[s]`` as section ``s``'s two past inputs and
    ``v * G[s + 1]`` as its two past outputs -- ``scipy.signal.sosfilt_zi(sos) * v`` in direct form 1.  The device kernel
    starts each pass of :func:`sosfiltfilt` from this state (the library computes the same products in ``long double``)."""
    a = sos_array(sos)
    g = np.ones(a.shape[0] + 1)
    for s in range(a.shape[0]):
        g[s + 1] = g[s] * (a[s, :3].sum() / a[s, 3:].sum())
    return g


@torch.no_grad()
def sosfiltfilt(x: Tensor, sos, padtype="odd", padlen: int | None = None) -> Tensor:
    """``scipy.signal.sosfiltfilt(sos, x, axis=-1, padtype=padtype, padlen=padlen)``.

    ``x`` is ``[T]``, ``[C, T]`` or ``[B, C, T]``; the result has its shape, dtype and device, rows are independent.
    ``sos [K, 6]`` (tensor or array) is used in float64.  ``padtype`` is "odd", "even", "constant" or None; ``padlen`` None
    is SciPy's default ``3 * (2 K + 1 - min(#(b2 == 0), #(a2 == 0)))``.  ``T <= padlen``, a bad ``padtype`` and a negative
    ``padlen`` raise ``ValueError``; a cascade with a pole at z = 1 has no steady state and SciPy's error from
    ``sosfilt_zi`` propagates.  Device float32 / float64 tensors run the HIP kernels (other device dtypes: ``TypeError``);
    CPU tensors run SciPy in float64."""
    import scipy.signal as sg

    if not isinstance(x, Tensor):
        raise TypeError(f"sosfiltfilt: x must be a torch.Tensor, got {type(x).__name__}")
    if x.dim() not in (1, 2, 3):
        raise ValueError("Input must be of shape [T], [C, T], or [B, C, T]")
    a = sos_array(sos)
    check_pad(padtype, padlen)
    edge = padlen_in_force(a, padtype, padlen)
    if x.shape[-1] <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if not x.is_cuda:
        y = sg.sosfiltfilt(a, x.detach().to(torch.float64).numpy(), axis=-1, padtype=padtype, padlen=padlen)
        return torch.from_numpy(np.ascontiguousarray(y)).to(x.dtype if x.is_floating_point() else torch.float64)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"sosfiltfilt: float32 or float64 device signals only, got {x.dtype}")
    _check_steady_state(a)
    from torchfx_amd import torchfx_ext

    with torch.cuda.device(x.device):
        return torchfx_ext.sos_filtfilt(x, a, padtype, edge)
