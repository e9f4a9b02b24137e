"""Freeverb room reverb: :func:`freeverb_bank`, :func:`freeverb` and the parameters behind :class:`torchfx_amd.effect.Freeverb`.

Freeverb (Jezar at Dreampoint, public domain) is the Schroeder-Moorer network: per channel eight parallel feedback combs, each
with a one-pole low-pass (the *damping*) in its loop, summed and sent through four all-passes in series.  A comb with a delay
of ``D`` samples reads only samples at least ``D`` old, so a block of up to ``D`` samples has all its inputs at hand and only
the damping filter -- a first-order linear scan -- is sequential inside it: on ROCm device float32 / float64 tensors one
workgroup per *bank* (one channel of one batch item) runs ``csrc/reverb.hip`` (:func:`torchfx_ext.freeverb_forward`), on CPU
tensors the same blocks run over NumPy arrays with ``scipy.signal.lfilter`` for the scan.  Everything is float64 for both
signal dtypes.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch
from torch import Tensor

from torchfx_amd.loudness import _check_fs, _check_signal

MAX_COMBS = 8
MAX_ALLPASS = 4
MAX_DELAY = 65536
# Freeverb's tunings in samples at 44.1 kHz (the second channel's are STEREO_SPREAD samples longer) and its fixed constants
COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_TUNING = (556, 441, 341, 225)
STEREO_SPREAD = 23
TUNING_FS = 44100
FIXED_GAIN = 0.015
ALLPASS_GAIN = 0.5
SCALE_ROOM, OFFSET_ROOM, SCALE_DAMP, SCALE_WET, SCALE_DRY = 0.28, 0.7, 0.4, 3.0, 2.0


def _real(name: str, v, what: str = "a finite number") -> float:
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"freeverb: {name} must be {what}, got {v!r}")
    return float(v)


def _unit(name: str, v) -> float:
    v = _real(name, v, "a number in [0, 1]")
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"freeverb: {name} must be in [0, 1], got {v!r}")
    return v


def _samples(name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
        raise ValueError(f"freeverb: {name} must be an integer number of samples >= 0, got {v!r}")
    return int(v)


def _delays(name: str, delays, channels: int, lo: int, hi: int) -> np.ndarray:
    """``delays`` as an int64 ``[channels, N]`` table with ``lo <= N <= hi`` and every delay in ``[1, MAX_DELAY]``."""
    if isinstance(delays, Tensor):
        delays = delays.detach().cpu().numpy()
    try:
        a = np.asarray(delays)
    except ValueError:
        raise ValueError(f"freeverb: {name} must be a [C, N] table of delays in samples, got {delays!r}") from None
    if a.size == 0:
        a = np.zeros((channels, 0), np.int64)
    if a.dtype == object or not (np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_):
        raise TypeError(f"freeverb: {name} must hold integers (samples), got {a.dtype}")
    if a.ndim == 1 and channels == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[0] != channels:
        raise ValueError(f"freeverb: {name} must have shape [C, N] = [{channels}, N], got {list(a.shape)}")
    if not lo <= a.shape[1] <= hi:
        raise ValueError(f"freeverb: {name} must hold {lo} to {hi} delays per channel, got {a.shape[1]}")
    if a.size and (a.min() < 1 or a.max() > MAX_DELAY):
        raise ValueError(f"freeverb: {name} must be in [1, {MAX_DELAY}] samples, got {int(a.min())} to {int(a.max())}")
    return np.ascontiguousarray(a, dtype=np.int64)


class BankParams:
    """What a :func:`freeverb_bank` call works with: ``comb`` / ``allpass`` (int64 ``[C, NC]`` / ``[C, NA]`` delays in samples),
    ``fb``, ``d1`` (the damping), ``g`` (the all-pass gain), ``input_gain``, ``dry``, ``wet1``, ``wet2`` and ``state_len`` (the
    float64 words per bank of the state: the longest bank's ``sum_k (D_k + 1) + sum_j D_j``)."""

    __slots__ = ("comb", "allpass", "fb", "d1", "g", "input_gain", "dry", "wet1", "wet2", "state_len")

    def __init__(self, channels: int, comb_delays, allpass_delays, feedback, damp, allpass_gain=ALLPASS_GAIN, input_gain=FIXED_GAIN,
                 dry_gain=1.0, wet1=1.0, wet2=0.0) -> None:
        if channels not in (1, 2):
            raise ValueError(f"freeverb: the signal must have 1 or 2 channels, got {channels}")
        self.comb = _delays("comb_delays", comb_delays, channels, 1, MAX_COMBS)
        self.allpass = _delays("allpass_delays", allpass_delays, channels, 0, MAX_ALLPASS)
        self.fb = _real("feedback", feedback)
        if not abs(self.fb) < 1.0:
            raise ValueError(f"freeverb: |feedback| must be < 1 (the combs decay), got {feedback!r}")
        self.d1 = _real("damp", damp)
        if not 0.0 <= self.d1 < 1.0:
            raise ValueError(f"freeverb: damp must be in [0, 1), got {damp!r}")
        self.g = _real("allpass_gain", allpass_gain)
        if not abs(self.g) < 1.0:
            raise ValueError(f"freeverb: |allpass_gain| must be < 1, got {allpass_gain!r}")
        self.input_gain = _real("input_gain", input_gain, "a finite gain")
        self.dry = _real("dry_gain", dry_gain, "a finite gain")
        self.wet1 = _real("wet1", wet1, "a finite gain")
        self.wet2 = _real("wet2", wet2, "a finite gain")
        self.state_len = int((self.comb.sum(1) + self.comb.shape[1] + self.allpass.sum(1)).max())


def tunings(fs, channels: int = 2) -> tuple[np.ndarray, np.ndarray]:
    """Freeverb's comb and all-pass delays at ``fs`` as int64 ``[channels, 8]`` and ``[channels, 4]``: the 44.1 kHz tunings
    ``t`` (the second channel's 23 samples longer) scaled to ``max(1, floor(t fs / 44100 + 0.5))``."""
    fs = _check_fs(fs)

    def at(t: int) -> int:
        return max(1, (2 * t * fs + TUNING_FS) // (2 * TUNING_FS))

    comb = [[at(t + c * STEREO_SPREAD) for t in COMB_TUNING] for c in range(channels)]
    allpass = [[at(t + c * STEREO_SPREAD) for t in ALLPASS_TUNING] for c in range(channels)]
    return np.array(comb, np.int64), np.array(allpass, np.int64)


class FreeverbParams:
    """Freeverb's user parameters reduced to a bank's: ``fb = 0.7 + 0.28 room_size``, ``d1 = 0.4 damping``,
    ``dry_gain = 2 dry``, ``wet1 = 3 wet (width / 2 + 0.5)``, ``wet2 = 3 wet (1 - width) / 2`` and ``tail_samples =
    floor(tail fs + 0.5)``; :meth:`bank` adds the tunings at ``fs`` for a channel count."""

    __slots__ = ("fs", "fb", "d1", "dry", "wet1", "wet2", "tail_samples")

    def __init__(self, fs, room_size=0.5, damping=0.5, wet=1.0 / 3.0, dry=0.5, width=1.0, tail=0.0) -> None:
        self.fs = _check_fs(fs)
        room_size, damping, wet = _unit("room_size", room_size), _unit("damping", damping), _unit("wet", wet)
        dry, width = _unit("dry", dry), _unit("width", width)
        tail = _real("tail", tail, "a finite time >= 0 in seconds")
        if tail < 0:
            raise ValueError(f"freeverb: tail must be a finite time >= 0 in seconds, got {tail!r}")
        self.fb = OFFSET_ROOM + SCALE_ROOM * room_size
        self.d1 = SCALE_DAMP * damping
        self.dry = SCALE_DRY * dry
        self.wet1 = SCALE_WET * wet * (width / 2.0 + 0.5)
        self.wet2 = SCALE_WET * wet * ((1.0 - width) / 2.0)
        self.tail_samples = int(math.floor(tail * self.fs + 0.5))

    def bank(self, channels: int) -> BankParams:
        if channels not in (1, 2):
            raise ValueError(f"freeverb: the signal must have 1 or 2 channels, got {channels}")
        comb, allpass = tunings(self.fs, channels)
        return BankParams(channels, comb, allpass, self.fb, self.d1, ALLPASS_GAIN, FIXED_GAIN, self.dry, self.wet1, self.wet2)


def _shape(x: Tensor) -> tuple[int, int, int]:
    """``(batch, channels, T)`` of a ``[T]``, ``[C, T]`` or ``[B, C, T]`` signal."""
    return (int(x.shape[0]) if x.dim() == 3 else 1), (int(x.shape[-2]) if x.dim() >= 2 else 1), int(x.shape[-1])


def _freeverb_host(xb: np.ndarray, P: BankParams, Tn: int, state: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """``xb [batch, C, T]`` -> ``(y [batch, C, Tn] in xb's dtype, new state [batch, C, state_len])``; ``state`` likewise.  Block
    by block as the device kernel: a comb's block is as long as the shortest comb delay, an all-pass's as long as its own."""
    from scipy.signal import lfilter

    Bt, C, T = xb.shape
    x64 = np.zeros((Bt, C, Tn), np.float64)
    x64[..., :T] = xb
    u = (P.input_gain * (2.0 / C)) * (x64[:, 0] if C == 1 else x64[:, 0] + x64[:, 1])
    d1, d2 = P.d1, 1.0 - P.d1
    r = np.empty((Bt, C, Tn), np.float64)
    new = np.zeros_like(state)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for c in range(C):
            comb, allpass = P.comb[c], P.allpass[c]
            # w of every comb with its D words of history in front: index n holds w[n - D]
            W, fl, off = [], [], 0
            for D in comb:
                D = int(D)
                w = np.empty((Bt, D + Tn), np.float64)
                w[:, :D] = state[:, c, off:off + D]
                W.append(w)
                fl.append(state[:, c, off + D])
                off += D + 1
            B = int(comb.min())
            for n0 in range(0, Tn, B):
                n1 = min(Tn, n0 + B)
                for k, D in enumerate(comb):
                    f, _ = lfilter([d2], [1.0, -d1], W[k][:, n0:n1], axis=-1, zi=d1 * fl[k][:, None])
                    fl[k] = f[:, -1]
                    W[k][:, int(D) + n0:int(D) + n1] = u[:, n0:n1] + P.fb * f
            s = W[0][:, :Tn].copy()
            for w in W[1:]:
                s += w[:, :Tn]
            soff = 0
            for k, D in enumerate(comb):
                D = int(D)
                new[:, c, soff:soff + D] = W[k][:, Tn:]
                new[:, c, soff + D] = fl[k]
                soff += D + 1
            del W
            for D in allpass:
                D = int(D)
                v = np.empty((Bt, D + Tn), np.float64)
                v[:, :D] = state[:, c, off:off + D]
                for n0 in range(0, Tn, D):
                    n1 = min(Tn, n0 + D)
                    b, sj = v[:, n0:n1], s[:, n0:n1].copy()
                    v[:, D + n0:D + n1] = sj + P.g * b
                    s[:, n0:n1] = b - sj
                new[:, c, soff:soff + D] = v[:, Tn:]
                off += D
                soff += D
            r[:, c] = s
        if C == 1:
            y = P.dry * x64 + (P.wet1 + P.wet2) * r
        else:
            y = P.dry * x64 + P.wet1 * r + P.wet2 * r[:, ::-1]
    return y.astype(xb.dtype), new


def _check_state(state, banks: int, state_len: int, device) -> Tensor | None:
    if state is None:
        return None
    if not isinstance(state, Tensor):
        raise TypeError(f"freeverb: state must be a torch.Tensor, got {type(state).__name__}")
    if tuple(state.shape) != (banks, state_len):
        raise ValueError(f"freeverb: state must have shape [banks, state_len] = [{banks}, {state_len}], got {list(state.shape)}")
    return state.detach().to(device=device, dtype=torch.float64)


@torch.no_grad()
def freeverb_bank(x: Tensor, comb_delays, allpass_delays, feedback: float, damp: float, allpass_gain: float = ALLPASS_GAIN,
                  input_gain: float = FIXED_GAIN, dry_gain: float = 1.0, wet1: float = 1.0, wet2: float = 0.0, tail_samples: int = 0,
                  state: Tensor | None = None, return_state: bool = False):
    """The comb / all-pass network behind :func:`freeverb` with every delay and gain given: ``x [T]``, ``[C, T]`` or
    ``[B, C, T]`` (float32 / float64, ``C`` 1 or 2) -> ``[..., T + tail_samples]`` in the same dtype and on the same device; with
    ``return_state`` also the end state ``[banks, state_len]`` float64.

    A *bank* is one channel of one batch item; batch items are independent.  ``comb_delays`` is ``[C, NC]`` (``1 <= NC <= 8``),
    ``allpass_delays`` ``[C, NA]`` (``0 <= NA <= 4``, ``()`` for none), whole samples in ``[1, 65536]`` (a flat sequence serves a
    single channel).  ``|feedback| < 1``, ``0 <= damp < 1``, ``|allpass_gain| < 1``, the gains finite.  With ``d1 = damp``,
    ``d2 = 1 - d1``, ``fb = feedback``, ``g = allpass_gain``, everything in float64 for both signal dtypes and ``w``, ``f``,
    ``v`` zero before sample 0 (or taken from ``state``):

    * feed ``u[n] = input_gain (2 / C) sum_c x_c[n]`` -- Freeverb's ``(L + R) gain`` for stereo, ``L = R`` for mono;
    * comb ``k`` of bank ``c`` (delay ``D``): ``o_k[n] = w_k[n - D]``, ``f_k[n] = d2 o_k[n] + d1 f_k[n-1]``,
      ``w_k[n] = u[n] + fb f_k[n]``;
    * the comb sum ``s_0[n] = ((o_0[n] + o_1[n]) + o_2[n]) + ...`` in this order;
    * all-pass ``j`` (delay ``D``): ``b[n] = v_j[n - D]``, ``s_{j+1}[n] = b[n] - s_j[n]``, ``v_j[n] = s_j[n] + g b[n]``;
    * the mix, with ``r_c = s_NA`` of bank ``c``: ``y_c[n] = dry_gain x_c[n] + wet1 r_c[n] + wet2 r_{1-c}[n]`` (one channel:
      ``dry_gain x[n] + (wet1 + wet2) r_0[n]``), summed left to right and rounded once to the signal's dtype.

    The input counts as zero from ``T`` on.  The state is one float64 row per bank: for each comb the last ``D`` values of
    ``w``, oldest first, then ``f``; then for each all-pass the last ``D`` values of ``v``, oldest first; the row is as long as
    the longest bank's and ends in zeros for a shorter one.  It is in time order, not ring order: it does not depend on how the
    stream was cut, and chunks shorter than a delay work.

    What follows from it:

    * **Dry.**  ``wet1 = wet2 = 0`` with ``dry_gain = 1`` returns a finite input bit for bit.
    * **Batch.**  A bank's bits depend on its own item's samples alone -- not on the other items of the batch nor their count.
    * **Tail.**  ``tail_samples = n`` is ``torch.equal`` to the call on the signal padded with ``n`` zeros.
    * **Chunks.**  Feeding the returned state into the next call continues the network: chunks equal the one-shot result to
      float64 round-off (the damping scan's association follows the blocks, and the blocks the cut), not bit for bit.
    * **Non-finite input.**  Samples before an item's first NaN / Inf agree, to the same round-off, with the result for the
      signal zeroed from that sample on; items without non-finite samples are bit-identical to their result alone.  Nothing
      is claimed about the affected item from that sample on.

    Device tensors run ``csrc/reverb.hip``: one launch for ``C = 1`` or ``wet2 = 0``, else a second, elementwise launch mixes
    the two banks (:func:`torchfx_ext.freeverb_plan_info`).  Fractional or modulated delays, more than two channels, autograd
    and axes other than the last are not provided.  ``ValueError`` / ``TypeError`` for a channel count other than 1 or 2, a delay
    table of the wrong shape, type or range, a coefficient out of range, a negative ``tail_samples``, a non-float dtype and a
    state of the wrong shape."""
    _check_signal(x, "freeverb")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"freeverb: float32 or float64 signals only, got {x.dtype}")
    batch, channels, T = _shape(x)
    P = BankParams(channels, comb_delays, allpass_delays, feedback, damp, allpass_gain, input_gain, dry_gain, wet1, wet2)
    tail = _samples("tail_samples", tail_samples)
    banks, Tn = batch * channels, T + tail
    st = _check_state(state, banks, P.state_len, x.device)
    if Tn == 0 or x.numel() == 0 and batch == 0:
        y = x.new_empty(*x.shape[:-1], Tn)
        st = st.clone() if st is not None else torch.zeros((banks, P.state_len), dtype=torch.float64, device=x.device)
    elif x.is_cuda:
        from torchfx_amd import torchfx_ext

        with torch.cuda.device(x.device):
            y, st = torchfx_ext.freeverb_forward(x, P.comb, P.allpass, P.fb, P.d1, P.g, P.input_gain, P.dry, P.wet1, P.wet2, tail, st)
    else:
        s0 = np.zeros((batch, channels, P.state_len)) if st is None else st.numpy().reshape(batch, channels, P.state_len)
        yh, sh = _freeverb_host(x.detach().numpy().reshape(batch, channels, T), P, Tn, s0)
        y = torch.from_numpy(yh.reshape(*x.shape[:-1], Tn))
        st = torch.from_numpy(sh.reshape(banks, P.state_len))
    return (y, st) if return_state else y


@torch.no_grad()
def freeverb(x: Tensor, fs: int, room_size: float = 0.5, damping: float = 0.5, wet: float = 1.0 / 3.0, dry: float = 0.5,
             width: float = 1.0, tail: float = 0.0) -> Tensor:
    """Freeverb on ``x [T]``, ``[C, T]`` or ``[B, C, T]`` (``C`` 1 or 2) at ``fs``: :func:`freeverb_bank` with Freeverb's eight
    combs and four all-passes per channel (:func:`tunings`) and its constants -- ``feedback = 0.7 + 0.28 room_size``,
    ``damp = 0.4 damping``, ``allpass_gain = 0.5``, ``input_gain = 0.015``, ``dry_gain = 2 dry``,
    ``wet1 = 3 wet (width / 2 + 0.5)``, ``wet2 = 3 wet (1 - width) / 2``.  ``room_size``, ``damping``, ``wet``, ``dry`` and
    ``width`` are in ``[0, 1]``; ``tail`` (seconds, ``>= 0``) appends ``floor(tail fs + 0.5)`` samples of ring-out.
    ``wet = 0, dry = 0.5`` returns the input bit for bit."""
    _check_signal(x, "freeverb")
    F = FreeverbParams(fs, room_size, damping, wet, dry, width, tail)
    P = F.bank(_shape(x)[1])
    return freeverb_bank(x, P.comb, P.allpass, P.fb, P.d1, P.g, P.input_gain, P.dry, P.wet1, P.wet2, F.tail_samples)
