"""``ZeroPhase``: SOS filters run forward and backward -- :func:`torchfx_amd.sosfiltfilt` as an effect."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from torchfx_amd.effect import FX
from torchfx_amd.filter._sos import CascadeTable


class ZeroPhase(FX):
    """Zero-phase (forward-backward) filtering with one or more SOS filters: ``scipy.signal.sosfiltfilt`` semantics.

    ``filters`` are ``IIR`` / ``Biquad`` modules or ``FusedSOSCascade``; several mean their sections concatenated in order
    and run as ONE ``sosfiltfilt`` (not one forward-backward pair per filter).  They are submodules, so a ``Wave`` the effect
    is piped into gives them its rate and designs them: ``wave | ZeroPhase(LoButterworth(1000))`` works with ``fs=None``.
    The effect is stateless: it neither reads nor writes the filters' carried ``_state_x`` / ``_state_y``.  The magnitude
    response is the cascade's squared -- a Linkwitz-Riley crossover is ``ZeroPhase`` of a Butterworth.  Non-causal:
    ``StreamProcessor`` and ``RealtimeProcessor`` refuse it."""

    def __init__(self, *filters: nn.Module, padtype="odd", padlen: int | None = None) -> None:
        super().__init__()
        from torchfx_amd.filter.biquad import Biquad
        from torchfx_amd.filter.fused import FusedSOSCascade
        from torchfx_amd.filter.iir import IIR
        from torchfx_amd.filtfilt import check_pad

        if not filters:
            raise ValueError("ZeroPhase needs at least one SOS filter")
        for f in filters:
            if not isinstance(f, (IIR, Biquad, FusedSOSCascade)):
                raise TypeError(f"ZeroPhase wraps IIR / Biquad filters or a FusedSOSCascade, got {type(f).__name__}")
        check_pad(padtype, padlen)
        self.filters = nn.ModuleList(filters)
        self.padtype, self.padlen = padtype, padlen
        self._sos_key, self._sos_cache, self._sos_held = None, None, []

    @property
    def fs(self) -> int | None:
        return next((f.fs for f in self.filters if getattr(f, "fs", None) is not None), None)

    @fs.setter
    def fs(self, value: int | None) -> None:
        if value is None:
            return
        for f in self.filters:
            if isinstance(f, FX) and getattr(f, "fs", 0) is None:
                f.fs = value

    def sos(self) -> Tensor:
        """The members' sections in order, host float64 ``[sum K, 6]`` (designing a member whose design is pending)."""
        key = tuple((id(t), t._version) if isinstance(t, Tensor) else None for t in (getattr(f, "_sos", None) for f in self.filters))
        if None in key or key != self._sos_key:             # a member was (re)designed or edited: gather again
            self._sos_cache = CascadeTable.gather(list(self.filters)).sos
            self._sos_key = tuple((id(f._sos), f._sos._version) for f in self.filters)
            self._sos_held = [f._sos for f in self.filters]      # keeps the ids from being recycled
        return self._sos_cache

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``scipy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"scipy on host -- {x.device.type} tensor"
        if x.dtype not in (torch.float32, torch.float64):
            return f"refused -- {x.dtype} signal (float32 / float64 only)"
        from torchfx_amd import torchfx_ext

        n = int(x.shape[-1]) if length is None else int(length)
        rows = max(1, x.numel() // max(1, int(x.shape[-1]))) if x.dim() else 1
        try:
            info = torchfx_ext.sos_filtfilt_plan_info(self.sos(), rows, n, self.padtype, self.padlen)
        except RuntimeError as e:
            return f"refused -- {e}"
        return (f"native (sos_filtfilt_forward_kernel + sos_filtfilt_reverse_kernel, padlen {info['padlen']}, "
                f"{info['nseg_forward']} + {info['nseg_reverse']} segments per row, float64 intermediate of {8 * info['work_elems']} B)")

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        from torchfx_amd.filtfilt import sosfiltfilt

        return sosfiltfilt(x, self.sos(), padtype=self.padtype, padlen=self.padlen)

    def extra_repr(self) -> str:
        return f"padtype={self.padtype!r}, padlen={self.padlen}"
