"""Programme loudness after ITU-R BS.1770-4 / EBU R128: :func:`integrated_loudness` (LUFS, two-stage gating),
:func:`momentary_loudness`, :func:`short_term_loudness`, :func:`loudness_range` (LU, EBU Tech 3342) and the measurement under
them, :func:`block_energy`; and the true peak of BS.1770-4 Annex 2, :func:`true_peak` (dBTP) / :func:`true_peak_linear`.

Everything is built on ONE array per signal: the energy of the K-weighted signal in consecutive 100 ms sub-blocks,
``S[.., c, i] = sum(y[c, e_i : e_(i+1)] ** 2)`` with ``e_i = (i * fs) // 10`` and ``y`` the float64 K-weighting cascade of
channel ``c`` from zero state.  A 400 ms gating block with 75 % overlap is four consecutive sub-blocks, a 3 s short-term
window thirty.  On ROCm device float32 / float64 tensors one HIP launch computes ``S`` (``csrc/sos.hip``,
:func:`torchfx_ext.sos_block_energy`): it reads the signal once and never stores the filtered one.  CPU tensors run SciPy's
``sosfilt`` and NumPy in float64.  The gating is a few torch ops on the ``[.., nblk]`` array, on the signal's device, with
no host synchronisation.

The true peak is the largest magnitude of the signal oversampled to at least 192 kHz with the library's own interpolator
(:func:`torchfx_amd.resample.resample_poly`).  On device tensors two HIP launches compute it per row (``csrc/resample.hip``,
:func:`torchfx_ext.true_peak`): they read the signal once and never store the oversampled one.  CPU tensors run SciPy's
``resample_poly``.  A streaming meter is not provided.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

ABSOLUTE_GATE = -70.0          # LUFS
RELATIVE_GATE = -10.0          # LU under the mean of the absolutely gated blocks
LRA_RELATIVE_GATE = -20.0      # Tech 3342: LU under the mean of the absolutely gated short-term windows
LRA_LOW, LRA_HIGH = 10, 95     # Tech 3342: the percentiles whose spread is the loudness range
OVERSAMPLE_FACTORS = (1, 2, 4, 8)
MAX_TAPS_PER_PHASE = 64        # the native kernel holds a phase's taps in registers
OFFSET = -0.691                # BS.1770: L = -0.691 + 10 log10(sum_c w_c z_c)


def _check_fs(fs) -> int:
    if isinstance(fs, bool) or not isinstance(fs, numbers.Integral) or fs < 8000:
        raise ValueError(f"fs must be an integer >= 8000, got {fs!r}")
    return int(fs)


def _biquad(f0: float, q: float, fs: int, vh: float = 1.0, vb: float = 0.0, high_pass: bool = False) -> list[float]:
    k = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + k / q + k * k
    b = [1.0, -2.0, 1.0] if high_pass else [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0]
    return b + [1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]


def kweighting_sos(fs: int) -> np.ndarray:
    """The K-weighting filter of BS.1770 at ``fs`` as a float64 ``[2, 6]`` SOS array: the high shelf (+4 dB above 1.68 kHz,
    the head's acoustic effect) and the RLB high-pass (38 Hz), from the analogue prototypes the standard's 48 kHz table was
    derived from.  At 48 kHz the coefficients are the table's to all 14 printed digits."""
    fs = _check_fs(fs)
    vh = 10.0 ** (3.999843853973347 / 20.0)
    shelf = _biquad(1681.974450955533, 0.7071752369554196, fs, vh, vh ** 0.4996667741545416)
    high = _biquad(38.13547087602444, 0.5003270373238773, fs, high_pass=True)
    return np.array([shelf, high], dtype=np.float64)


def block_edges(nblk: int, fs: int) -> np.ndarray:
    """``e_i = (i * fs) // 10`` for ``i = 0 ... nblk`` (int64)."""
    return (np.arange(nblk + 1, dtype=np.int64) * int(fs)) // 10


def _check_signal(x, what: str) -> None:
    if not isinstance(x, Tensor):
        raise TypeError(f"{what}: x must be a torch.Tensor, got {type(x).__name__}")
    if x.dim() not in (1, 2, 3):
        raise ValueError("Input must be of shape [T], [C, T], or [B, C, T]")


@torch.no_grad()
def block_energy(x: Tensor, fs: int) -> Tensor:
    """Energy of the K-weighted signal per 100 ms sub-block: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` -> float64
    ``[.., nblk]`` on ``x``'s device, ``nblk = (T * 10) // fs`` (samples after the last whole sub-block belong to none).
    A NaN / Inf sample makes its sub-block and every later one of its row non-finite."""
    _check_signal(x, "block_energy")
    fs = _check_fs(fs)
    sos = kweighting_sos(fs)
    if x.is_cuda:
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"block_energy: float32 or float64 device signals only, got {x.dtype}")
        from torchfx_amd import torchfx_ext

        with torch.cuda.device(x.device):
            return torchfx_ext.sos_block_energy(x, sos, fs, 10)
    import scipy.signal as sg

    a = x.detach().to(torch.float64).numpy()
    nblk = (a.shape[-1] * 10) // fs
    e = block_edges(nblk, fs)
    if nblk == 0:
        return torch.zeros(a.shape[:-1] + (0,), dtype=torch.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = sg.sosfilt(sos, a, axis=-1)[..., :e[-1]]
        s = np.add.reduceat(y * y, e[:-1], axis=-1)
    return torch.from_numpy(np.ascontiguousarray(s))


def _weights(channel_weights, channels: int, like: Tensor) -> Tensor:
    if channel_weights is None:
        return torch.ones(channels, dtype=torch.float64, device=like.device)
    w = [float(v) for v in (channel_weights.tolist() if isinstance(channel_weights, (Tensor, np.ndarray)) else channel_weights)]
    if len(w) != channels:
        raise ValueError(f"channel_weights has {len(w)} entries, the signal has {channels} channel(s)")
    return torch.tensor(w, dtype=torch.float64).to(like.device)


def _window_power(x: Tensor, fs: int, channel_weights, width: int) -> tuple[Tensor, int]:
    """``P[.., j] = sum_c w_c * (S[c, j] + ... + S[c, j + width - 1]) / (e_(j + width) - e_j)`` -- the weighted mean square
    of the windows of ``width`` sub-blocks at a 100 ms hop, ``[J]`` for ``[T]`` / ``[C, T]`` and ``[B, J]`` for ``[B, C, T]``,
    with ``J = max(0, nblk - width + 1)``."""
    _check_signal(x, "loudness")
    fs = _check_fs(fs)
    channels = 1 if x.dim() == 1 else int(x.shape[-2])
    w = _weights(channel_weights, channels, x)
    s = block_energy(x, fs)
    if x.dim() == 1:
        s = s.unsqueeze(0)
    nblk = int(s.shape[-1])
    count = max(0, nblk - width + 1)
    if count == 0:
        return torch.zeros(s.shape[:-2] + (0,), dtype=torch.float64, device=s.device), 0
    e = block_edges(nblk, fs)
    n = torch.from_numpy((e[width:] - e[:-width]).astype(np.float64)).to(s.device)
    z = s.unfold(-1, width, 1).sum(-1) / n                       # [.., C, J]
    return (z * w.unsqueeze(-1)).sum(-2), count


def _lufs(p: Tensor) -> Tensor:
    return OFFSET + 10.0 * torch.log10(p)


@torch.no_grad()
def momentary_loudness(x: Tensor, fs: int, channel_weights=None) -> Tensor:
    """Momentary loudness (400 ms windows, 100 ms hop) in LUFS: float64 ``[.., nblk - 3]``, empty when the signal is
    shorter than 400 ms."""
    return _lufs(_window_power(x, fs, channel_weights, 4)[0])


@torch.no_grad()
def short_term_loudness(x: Tensor, fs: int, channel_weights=None) -> Tensor:
    """Short-term loudness (3 s windows, 100 ms hop) in LUFS: float64 ``[.., nblk - 29]``, empty when the signal is
    shorter than 3 s."""
    return _lufs(_window_power(x, fs, channel_weights, 30)[0])


@torch.no_grad()
def integrated_loudness(x: Tensor, fs: int, channel_weights=None) -> Tensor:
    """Integrated (programme) loudness in LUFS after BS.1770-4: float64 on ``x``'s device, 0-d for ``[T]`` and ``[C, T]``,
    ``[B]`` for ``[B, C, T]``.

    Gating blocks are 400 ms with 75 % overlap; ``P_j`` is their weighted mean square (``channel_weights`` default 1.0 per
    channel; 1.41 for the surround channels of a 5.1 layout) and ``l_j = -0.691 + 10 log10 P_j``.  Blocks with ``l_j > -70``
    pass the absolute gate; the relative gate lies 10 LU under the loudness of their mean; the result is the loudness of the
    mean of the blocks that pass both.  A signal shorter than 400 ms, or with no block above -70 LUFS, measures ``-inf``;
    any NaN block makes the result NaN.  No host synchronisation: the gating is masks and sums on the device."""
    p, count = _window_power(x, fs, channel_weights, 4)
    if count == 0:
        return torch.full(p.shape[:-1], -math.inf, dtype=torch.float64, device=p.device)
    lj = _lufs(p)
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    above = lj > ABSOLUTE_GATE
    n_abs = above.sum(-1)
    gate = _lufs(torch.where(above, p, zero).sum(-1) / n_abs) + RELATIVE_GATE
    both = above & (lj > gate.unsqueeze(-1))
    out = _lufs(torch.where(both, p, zero).sum(-1) / both.sum(-1))
    out = torch.where(n_abs > 0, out, torch.full_like(out, -math.inf))
    return torch.where(torch.isnan(p).any(-1), torch.full_like(out, math.nan), out)


@torch.no_grad()
def loudness_range(x: Tensor, fs: int, channel_weights=None) -> Tensor:
    """Loudness range (LRA) in LU after EBU Tech 3342: float64 on ``x``'s device, 0-d for ``[T]`` and ``[C, T]``, ``[B]`` for
    ``[B, C, T]``.

    The short-term values ``l_j`` (3 s windows, 100 ms hop) with ``l_j > -70`` pass the absolute gate; the relative gate
    lies 20 LU under the loudness of their mean power; of the ``n`` values that pass both, sorted, the range is
    ``v[(95 (n - 1) + 50) // 100] - v[(10 (n - 1) + 50) // 100]`` -- Tech 3342's nearest-rank percentiles, halves rounded up.
    ``0.0`` when no window passes or the signal is shorter than 3 s; NaN when any window is NaN.  No host synchronisation:
    the values that fail are masked to ``+inf`` before the sort and the two ranks are gathered on the device."""
    p, count = _window_power(x, fs, channel_weights, 30)
    if count == 0:
        return torch.zeros(p.shape[:-1], dtype=torch.float64, device=p.device)
    lj = _lufs(p)
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    above = lj > ABSOLUTE_GATE
    gate = _lufs(torch.where(above, p, zero).sum(-1) / above.sum(-1)) + LRA_RELATIVE_GATE
    both = above & (lj > gate.unsqueeze(-1))
    n = both.sum(-1, keepdim=True)
    v = torch.sort(torch.where(both, lj, torch.full_like(lj, math.inf)), dim=-1).values
    last = (n - 1).clamp(min=0)
    low = torch.div(LRA_LOW * last + 50, 100, rounding_mode="floor")
    high = torch.div(LRA_HIGH * last + 50, 100, rounding_mode="floor")
    out = (v.gather(-1, high) - v.gather(-1, low)).squeeze(-1)
    out = torch.where(n.squeeze(-1) > 0, out, torch.zeros_like(out))
    return torch.where(torch.isnan(p).any(-1), torch.full_like(out, math.nan), out)


def default_oversample(fs: int) -> int:
    """BS.1770-4 Annex 2 oversamples to at least 192 kHz: 4 below 96 kHz, 2 below 192 kHz, 1 (the sample peak) from there."""
    return 4 if fs < 96000 else 2 if fs < 192000 else 1


def _interpolator(taps, oversample: int, dtype: torch.dtype):
    """The caller's interpolation filter (already scaled by ``oversample``) as a 1-D host tensor of ``dtype``; None = the
    library's own design."""
    if taps is None:
        return None
    a = taps.detach().cpu().numpy() if isinstance(taps, Tensor) else np.asarray(taps)
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"true_peak: taps must be a non-empty 1-D array, got shape {a.shape}")
    if a.size > MAX_TAPS_PER_PHASE * oversample:
        raise ValueError(f"true_peak: {a.size} taps, at most {MAX_TAPS_PER_PHASE} * oversample = "
                         f"{MAX_TAPS_PER_PHASE * oversample} are supported")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if dtype == torch.float64 else np.float32))


@torch.no_grad()
def true_peak_linear(x: Tensor, fs: int, oversample: int | None = None, taps=None) -> Tensor:
    """:func:`true_peak` as a linear magnitude in the signal's dtype (same shapes): ``max |resample_poly(row, L, 1)|`` over
    that function's ``T * L`` outputs, ``0`` for a row of no samples."""
    _check_signal(x, "true_peak")
    fs = _check_fs(fs)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"true_peak: float32 or float64 signals only, got {x.dtype}")
    if oversample is None:
        oversample = default_oversample(fs)
    if isinstance(oversample, bool) or oversample not in OVERSAMPLE_FACTORS:
        raise ValueError(f"true_peak: oversample must be one of {OVERSAMPLE_FACTORS}, got {oversample!r}")
    up = int(oversample)
    h = _interpolator(taps, up, x.dtype)
    if x.shape[-1] == 0:
        return torch.zeros(x.shape[:-1], dtype=x.dtype, device=x.device)
    if not x.is_cuda:
        if up == 1:
            return x.abs().amax(-1)
        from torchfx_amd.resample import resample_poly

        # resample_poly takes the filter before its `h *= up`; up is a power of two, so the division is exact
        window = ("kaiser", 5.0) if h is None else (h / up).numpy()
        return resample_poly(x, up, 1, window=window).abs().amax(-1)
    from torchfx_amd import torchfx_ext

    with torch.cuda.device(x.device):
        if up == 1:
            return torchfx_ext.stat_forward(x, torchfx_ext.STAT_ABSMAX, per_row=True).reshape(x.shape[:-1]).to(x.dtype)
        if h is None:
            from torchfx_amd.resample import design_taps

            h = design_taps(up, 1, ("kaiser", 5.0), x.dtype)
        return torchfx_ext.true_peak(x, h, up)


@torch.no_grad()
def true_peak(x: Tensor, fs: int, oversample: int | None = None, taps=None) -> Tensor:
    """True peak in dBTP per channel after ITU-R BS.1770-4 Annex 2: ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (float32 /
    float64) -> float64 on ``x``'s device, 0-d for ``[T]``, ``[C]`` for ``[C, T]``, ``[B, C]`` for ``[B, C, T]``.  The
    programme figure is the largest channel's, ``true_peak(x, fs).amax(-1)``.

    The reading of a row is ``20 log10 max |resample_poly(row, L, 1, window=("kaiser", 5.0))|`` over exactly that function's
    ``T * L`` outputs.  ``oversample`` = ``L`` is 1, 2, 4 or 8; None picks 4 below 96 kHz, 2 below 192 kHz and 1 from there
    (Annex 2: oversample to at least 192 kHz); ``L = 1`` is the sample peak.  The interpolator is
    :func:`torchfx_amd.resample.design_taps` ``(L, 1)`` (``firwin``, ``20 L + 1`` taps, scaled by ``L``); ``taps`` replaces
    it with the caller's own 1-D filter, already scaled by ``L`` and at most ``64 L`` long (the table in Annex 2 is one such
    filter).  Silence reads ``-inf``; a row with a NaN sample reads NaN, a row with an Inf sample NaN or ``+inf``; other rows
    are unaffected.  Device tensors run the HIP kernel, CPU tensors SciPy's ``resample_poly`` in the signal's dtype; no
    host synchronisation."""
    return 20.0 * torch.log10(true_peak_linear(x, fs, oversample, taps).to(torch.float64))
