"""Oversampled waveshaping: :func:`waveshape` and the parameters behind :class:`torchfx_amd.effect.Waveshaper` and
:class:`~torchfx_amd.effect.Distortion`.

A memoryless nonlinearity (a clipper, a saturator, a transfer curve as in WebAudio's ``WaveShaperNode``) makes harmonics above
Nyquist that fold back as aliases, so the signal is up-sampled by ``oversample``, shaped and decimated.  On ROCm device float32 /
float64 tensors that is one launch of ``csrc/waveshaper.hip`` (:func:`torchfx_ext.waveshaper_forward`): the oversampled signal
lives in LDS only.  CPU tensors run the same definition over SciPy's ``resample_poly`` and NumPy, in the signal's dtype.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.loudness import _check_signal

SHAPES = ("hard", "cubic", "tanh")
OVERSAMPLE = (1, 2, 4, 8)
MAX_CURVE = 4096
MAX_TAPS_PER_RATE = 64          # a stage takes at most 64 * oversample taps


def _real(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"waveshape: {name} must be a finite number, got {v!r}")
    return float(v)


def shape_f64(v: np.ndarray, shape: str, curve: np.ndarray | None = None) -> np.ndarray:
    """The transfer function in the precision of ``v`` (float64 or wider), as the definition states it."""
    if shape == "hard":
        return np.minimum(np.maximum(v, -1.0), 1.0)
    if shape == "cubic":
        c = np.minimum(np.maximum(v, -1.0), 1.0)
        return 1.5 * c - 0.5 * c * c * c
    if shape == "tanh":
        return np.tanh(v)
    n = len(curve)
    pos = np.minimum(np.maximum((v + 1.0) * ((n - 1) / 2.0), 0.0), n - 1.0)
    i = np.minimum(np.floor(pos), n - 2.0).astype(np.int64)
    c = np.asarray(curve, dtype=v.dtype)
    return c[i] + (pos - i) * (c[i + 1] - c[i])


class ShaperParams:
    """What a waveshaper call works with, checked: ``shape`` ("hard", "cubic", "tanh" or "curve"), ``curve`` (float64 1-D array
    or None), ``drive`` (linear), ``bias``, ``oversample``, ``dry = 1 - mix``, ``wet = mix 10^(output_db / 20)`` and ``window``."""

    __slots__ = ("shape", "curve", "drive", "bias", "oversample", "dry", "wet", "window")

    def __init__(self, shape=None, drive_db=0.0, bias=0.0, oversample=4, mix=1.0, output_db=0.0, curve=None,
                 window=("kaiser", 5.0)) -> None:
        if isinstance(oversample, bool) or not isinstance(oversample, numbers.Integral) or int(oversample) not in OVERSAMPLE:
            raise ValueError(f"waveshape: oversample must be one of {OVERSAMPLE}, got {oversample!r}")
        if curve is not None:
            if shape is not None:
                raise ValueError(f"waveshape: give a shape or a curve, not both (shape={shape!r})")
            c = curve.detach().cpu().numpy() if isinstance(curve, Tensor) else np.asarray(curve)
            if c.ndim != 1 or c.dtype.kind not in "fiu":
                raise TypeError("waveshape: curve must be a 1-D array of real numbers")
            if not 2 <= c.size <= MAX_CURVE:
                raise ValueError(f"waveshape: a curve must have 2 to {MAX_CURVE} points, got {c.size}")
            c = c.astype(np.float64)
            if not np.isfinite(c).all():
                raise ValueError("waveshape: curve must be finite")
            self.shape, self.curve = "curve", c
        else:
            shape = "tanh" if shape is None else shape
            if shape not in SHAPES:
                raise ValueError(f"waveshape: shape must be one of {SHAPES}, got {shape!r}")
            self.shape, self.curve = shape, None
        self.bias, mix = _real("bias", bias), _real("mix", mix)
        try:
            self.drive = 10.0 ** (_real("drive_db", drive_db) / 20.0)
            self.dry, self.wet = 1.0 - mix, mix * 10.0 ** (_real("output_db", output_db) / 20.0)
        except OverflowError:
            self.drive = self.wet = math.inf
        if not (math.isfinite(self.drive) and math.isfinite(self.wet)):
            raise ValueError("waveshape: drive_db and output_db must give finite gains")
        self.oversample, self.window = int(oversample), window

    def taps(self, dtype: torch.dtype) -> tuple[Tensor | None, Tensor | None]:
        """The host taps of the two stages in ``dtype`` (None, None for ``oversample = 1``); a tap array longer than
        ``64 * oversample`` is refused."""
        from torchfx_amd.resample import design_taps

        L = self.oversample
        if L == 1:
            return None, None
        up, dn = design_taps(L, 1, self.window, dtype), design_taps(1, L, self.window, dtype)
        if up.numel() > MAX_TAPS_PER_RATE * L:
            raise ValueError(f"waveshape: {up.numel()} taps, a stage takes at most 64 * oversample = {MAX_TAPS_PER_RATE * L}")
        return up, dn

    def c0(self, np_dtype) -> np.generic:
        """``f(bias)`` in float64 from the bias and the curve as ``np_dtype`` holds them, rounded to ``np_dtype``."""
        b = np.array([np_dtype(self.bias)], np.float64)
        c = None if self.curve is None else self.curve.astype(np_dtype).astype(np.float64)
        return np_dtype(shape_f64(b, self.shape, c)[0])


def _shape_host(v: np.ndarray, P: ShaperParams) -> np.ndarray:
    """The transfer function in ``v``'s dtype."""
    dt = v.dtype.type
    if P.shape == "hard":
        return np.clip(v, dt(-1), dt(1))
    if P.shape == "cubic":
        c = np.clip(v, dt(-1), dt(1))
        return c * (dt(1.5) - dt(0.5) * (c * c))
    if P.shape == "tanh":
        return np.tanh(v)
    n = P.curve.size
    c = P.curve.astype(v.dtype)
    pos = np.clip((v + dt(1)) * dt((n - 1) / 2.0), dt(0), dt(n - 1))
    pos = np.where(np.isnan(pos), dt(0), pos)
    i = np.minimum(np.floor(pos), dt(n - 2)).astype(np.int64)
    return c[i] + (pos - i.astype(v.dtype)) * (c[i + 1] - c[i])


def _waveshape_host(x: Tensor, P: ShaperParams) -> Tensor:
    from torchfx_amd.resample import resample_poly

    L = P.oversample
    a = x.detach().contiguous()
    dt = a.numpy().dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        u = (resample_poly(a, L, 1, window=P.window) if L > 1 else a).numpy()
        v = u * dt(P.drive) + dt(P.bias)
        w = _shape_host(v, P) - P.c0(dt)
        w = np.where(np.isfinite(u), w, dt(np.nan)).astype(u.dtype)
        z = resample_poly(torch.from_numpy(w), 1, L, window=P.window).numpy() if L > 1 else w
        y = dt(P.dry) * a.numpy() + dt(P.wet) * z
    return torch.from_numpy(np.ascontiguousarray(y.astype(u.dtype, copy=False)))


def check_gains(P: ShaperParams, dtype: torch.dtype) -> None:
    """Refuse gains that are finite as Python floats but not in the signal's dtype, which is how both paths hold them: a float32
    drive of 10^40 is Inf, and silence would shape to ``0 * Inf = NaN``."""
    if dtype != torch.float32:
        return
    with np.errstate(over="ignore"):
        bad = [n for n in ("drive", "bias", "dry", "wet") if not np.isfinite(np.float32(getattr(P, n)))]
    if bad:
        raise ValueError(f"waveshape: {', '.join(bad)} must be finite in the signal's dtype {dtype}")


@torch.no_grad()
def shape_signal(x: Tensor, P: ShaperParams) -> Tensor:
    """:func:`waveshape` with the parameters already checked and reduced (the effects' entry)."""
    _check_signal(x, "waveshape")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"waveshape: float32 or float64 signals only, got {x.dtype}")
    check_gains(P, x.dtype)
    up, dn = P.taps(x.dtype)
    if x.shape[-1] == 0 or x.numel() == 0:
        return torch.empty_like(x)
    if not x.is_cuda:
        return _waveshape_host(x, P)
    from torchfx_amd import torchfx_ext

    curve = None if P.curve is None else torch.from_numpy(P.curve).to(x.dtype)
    with torch.cuda.device(x.device):
        return torchfx_ext.waveshaper_forward(x, P.oversample, P.shape, curve, P.drive, P.bias, P.dry, P.wet, up, dn)


@torch.no_grad()
def waveshape(x: Tensor, shape: str | None = None, drive_db: float = 0.0, bias: float = 0.0, oversample: int = 4, mix: float = 1.0,
              output_db: float = 0.0, curve=None, window=("kaiser", 5.0)) -> Tensor:
    """Oversampled waveshaping: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 / float64) -> the same shape, dtype and device.
    The effect is rate-independent (no ``fs``).  With ``L = oversample`` in ``{1, 2, 4, 8}`` and the library's own resampling
    filters for ``window`` (a ``firwin`` window spec or a 1-D tap array of at most ``64 L`` taps, as in
    :func:`~torchfx_amd.resample.resample_poly`), all in the signal's dtype:

    1. ``u = resample_poly(x, L, 1)``: length ``T L``, zeros outside ``[0, T)``
    2. ``v = drive u + bias`` with ``drive = 10^(drive_db / 20)``: a multiplication, then an addition
    3. ``w = f(v) - c0``, ``c0 = f(bias)`` evaluated in float64 and rounded once: silence stays silence under a bias
    4. ``z = resample_poly(w, 1, L)``: length ``T`` again; ``w`` counts as zero outside ``[0, T L)``
    5. ``y = dry x + wet z`` with ``dry = 1 - mix`` and ``wet = mix 10^(output_db / 20)``

    ``L = 1`` has no filters (``z = w``).  Both resamplers compensate their delay, so there is no latency and ``x`` mixes in
    without a delay line.  ``shape`` (default ``"tanh"``): ``"hard"`` ``min(max(v, -1), 1)``; ``"cubic"`` ``1.5 v - 0.5 v^3``
    inside ``[-1, 1]``, ``sign(v)`` outside; ``"tanh"``.  Or ``curve``, a table ``c`` of ``N`` in ``[2, 4096]`` points over
    ``[-1, 1]`` read by WebAudio's rule: ``pos = (v + 1)(N - 1)/2`` clamped to ``[0, N - 1]``, ``i = min(floor(pos), N - 2)``,
    ``f = c[i] + (pos - i)(c[i+1] - c[i])``.  Give a shape or a curve, not both.

    What follows from it (device tensors):

    * **Bits of the composition.**  A finite signal with ``shape="hard"``, ``mix=1``, ``output_db=0`` is ``torch.equal`` to
      ``resample_poly(torch.clamp(resample_poly(x, L, 1) * drive, -1, 1), 1, L)``.
    * **Transparency.**  ``mix=0`` returns a finite input bit for bit.
    * **Independence.**  A row's bits depend on its own samples alone, not on the other rows or on where tiles fall.
    * **Non-finite input.**  ``y[m]`` is NaN exactly when ``x[m - reach_after .. m + reach_before]`` holds a NaN or an Inf
      (:func:`torchfx_ext.waveshaper_plan_info`; 20 and 21 samples for the default window at every ``L > 1``): every tap of both
      zero-padded filters counts.  An up-sampled value that is not finite shapes to NaN -- the composition's ``tanh`` of an Inf
      would come back finite.  Every other output has the bits it has with a zero in that sample's place.

    Argument errors are ``ValueError`` / ``TypeError`` before any launch; that includes gains that are finite numbers but not in
    the signal's dtype (``drive_db=800`` on a float32 signal: the drive would be Inf and silence would shape to NaN).  For chunked streams use
    :class:`torchfx_amd.realtime.StatefulWaveshaper` / ``StatefulDistortion``, whose chunks plus ``flush()`` are ``torch.equal`` to
    this call on the whole signal.  Shapes with memory, autograd and axes other than the last are not provided."""
    _check_signal(x, "waveshape")
    return shape_signal(x, ShaperParams(shape, drive_db, bias, oversample, mix, output_db, curve, window))
