"""``FX`` base class and the elementwise effects that sit between filters in a pipeline.

Reference: ``src/torchfx/effect.py`` -- ``FX.__or__`` (:253-258, builds a ``FilterChain``),
``Gain`` (:261-383) and ``Normalize`` with its strategy objects (:386-531, :534-790).  These are
SURVEY.md 8f rank 3: they are not filters, but a ``wave | iir | gain | fir`` pipeline passes through
them, so they run as streaming HIP passes (``csrc/effects.hip``) and a clamp-free ``Gain`` can be
folded into a neighbouring filter's coefficients by the ``Wave`` planner (opt-in, ``fuse_gain``).
``Reverb`` is the reference's one-tap feed-forward comb over ``delay_line_forward``.  ``Delay`` is the reference's
BPM-synced multi-tap delay (``effect.py:934-1538``) with its mono and ping-pong strategies: on device float32 / float64
signals one HIP launch (``csrc/delay.hip``) replaces the strategy's ``2 * taps`` passes, the zero-pad copy and the
``torch.lerp``; CPU tensors, other dtypes and custom strategies run the reference's torch composition.
"""
from __future__ import annotations

import abc
import math
import typing as tp

import torch
from torch import Tensor, nn


class FX(nn.Module, abc.ABC):
    """Abstract base of every effect / filter: an ``nn.Module`` with ``forward(x)``."""

    def __init__(self) -> None:
        super().__init__()

    @abc.abstractmethod
    def forward(self, x: Tensor) -> Tensor: ...

    def __or__(self, other: nn.Module):
        # effect.py:253-258: NotImplemented for non-modules, else a flat chain
        if not isinstance(other, nn.Module):
            return NotImplemented
        from torchfx_amd.chain import FilterChain

        return FilterChain(self, other)


def _ext():
    from torchfx_amd import torchfx_ext

    return torchfx_ext


class Gain(FX):
    """Volume change: ``gain_type`` "amplitude" (factor), "db" (``10^(g/20)``) or "power"
    (``10*log10(g)`` dB); ``clamp=True`` clips the result to [-1, 1]  (``effect.py:261-383``)."""

    def __init__(self, gain: float, gain_type: str = "amplitude", clamp: bool = False) -> None:
        super().__init__()
        self.gain, self.gain_type, self.clamp = gain, gain_type, clamp
        if gain_type in ("amplitude", "power") and gain < 0:
            raise ValueError("If gain_type = amplitude or power, gain must be positive.")

    def linear_gain(self) -> float | None:
        """The factor the samples are multiplied by (None: unknown ``gain_type`` -> identity,
        0 dB -> identity as in ``_gain_db``, ``effect.py:132-136``)."""
        if self.gain_type == "amplitude":
            return float(self.gain)
        if self.gain_type == "db":
            db = self.gain
        elif self.gain_type == "power":
            db = 10 * math.log10(self.gain)
        else:
            return None
        return None if db == 0 else 10 ** (db / 20)

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        g = self.linear_gain()
        if g is None and not self.clamp:
            return waveform
        return _ext().gain_forward(waveform, 1.0 if g is None else g, self.clamp)


# ------------------------------------------------------------------------------- Normalize
class NormalizationStrategy(abc.ABC):
    """``(waveform, peak) -> waveform`` (``effect.py:534-611``)."""

    @abc.abstractmethod
    def __call__(self, waveform: Tensor, peak: float) -> Tensor: ...


class CustomNormalizationStrategy(NormalizationStrategy):
    """Wraps a user callable (``effect.py:614-675``); runs whatever the callable does."""

    def __init__(self, func: tp.Callable[[Tensor, float], Tensor]) -> None:
        assert callable(func), "func must be callable"
        self.func = func

    def __call__(self, waveform: Tensor, peak: float) -> Tensor:
        return self.func(waveform, peak)


class PeakNormalizationStrategy(NormalizationStrategy):
    """``x / max|x| * peak`` (unchanged if the signal is all zero) -- ``effect.py:678-698``."""

    def __call__(self, waveform: Tensor, peak: float) -> Tensor:
        return _ext().normalize_forward(waveform, peak, _ext().STAT_ABSMAX, per_row=False)


class RMSNormalizationStrategy(NormalizationStrategy):
    """``x / sqrt(mean(x^2)) * peak`` -- ``effect.py:700-721``."""

    def __call__(self, waveform: Tensor, peak: float) -> Tensor:
        return _ext().normalize_forward(waveform, peak, _ext().STAT_RMS, per_row=False)


class PercentileNormalizationStrategy(NormalizationStrategy):
    """``x / P_p(|x|) * peak`` (``effect.py:723-755``).  The percentile is a selection problem, not a sort: on float32 device
    signals it is a three-pass radix select (``torchfx_ext.quantile_abs`` -- the value ``torch.quantile(|x|, p / 100,
    interpolation="linear")`` returns, without its 16 M element limit), the threshold stays on the device and the scaling is the
    ``normalize_apply`` pass (unchanged signal when the threshold is not positive, as in the reference).  Other dtypes take
    ``torch.quantile`` like the reference."""

    def __init__(self, percentile: float = 99.0) -> None:
        assert 0 < percentile <= 100, "Percentile must be between 0 and 100."
        self.percentile = percentile

    def __call__(self, waveform: Tensor, peak: float) -> Tensor:
        if waveform.dtype == torch.float32 and waveform.numel() > 0:
            E = _ext()
            threshold = E.quantile_abs(waveform, self.percentile / 100)
            return E.normalize_apply(waveform, threshold, peak, E.STAT_ABSMAX, False)
        threshold = torch.quantile(torch.abs(waveform), self.percentile / 100, interpolation="linear")
        return waveform / threshold * peak if threshold > 0 else waveform


class PerChannelNormalizationStrategy(NormalizationStrategy):
    """Every channel to its own peak (``effect.py:757-786``): ``[C,T]`` or ``[B,C,T]``."""

    def __call__(self, waveform: Tensor, peak: float) -> Tensor:
        assert waveform.ndim >= 2, "Waveform must have at least 2 dimensions (channels, time)."
        if waveform.ndim not in (2, 3):
            raise ValueError("Waveform must have shape (C, T) or (B, C, T)")
        return _ext().normalize_forward(waveform, peak, _ext().STAT_ABSMAX, per_row=True)


class Normalize(FX):
    """Normalise to ``peak`` with a pluggable strategy, default peak (``effect.py:386-531``)."""

    def __init__(self, peak: float = 1.0,
                 strategy: NormalizationStrategy | tp.Callable[[Tensor, float], Tensor] | None = None) -> None:
        super().__init__()
        assert peak > 0, "Peak value must be positive."
        self.peak = peak
        if callable(strategy) and not isinstance(strategy, NormalizationStrategy):
            strategy = CustomNormalizationStrategy(strategy)
        self.strategy = strategy or PeakNormalizationStrategy()
        if not isinstance(self.strategy, NormalizationStrategy):
            raise TypeError("Strategy must be an instance of NormalizationStrategy.")

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        return self.strategy(waveform, self.peak)


class LoudnessNormalize(FX):
    """Normalise to a programme loudness: measure the integrated loudness ``L`` of the signal (ITU-R BS.1770-4 / EBU R128,
    :func:`torchfx_amd.loudness.integrated_loudness`) and multiply by ``10 ** ((target - L) / 20)``.

    ``target`` in LUFS (-23 = EBU R128 delivery, -14 / -16 = streaming services); ``channel_weights`` as for the measurement
    (default 1.0 per channel).  One measurement per ``[C, T]`` signal, one per batch item of ``[B, C, T]``, mono for ``[T]``.
    The gain stays on the signal's device: nothing is read back between measuring and applying.  A signal that measures
    ``-inf`` (silence, or shorter than 400 ms) is left unchanged, as ``Normalize`` leaves an all-zero signal; a NaN measurement
    gives NaN samples.  ``fs`` comes from the ``Wave`` the effect is piped into when it is None.  A whole-signal measurement:
    it is a step of its own in ``Wave.plan()`` and cannot run in a chunked stream.

    ``max_true_peak`` (dBTP, default None = no ceiling) caps the gain so that the programme true peak ``TP`` of the result
    -- the largest channel's reading of the ``[C, T]`` signal or batch item, :func:`torchfx_amd.loudness.true_peak` on the
    same input -- does not pass it: the gain in dB is ``min(target - L, max_true_peak - TP)``.  The ceiling only lowers
    the gain; it does not limit."""

    def __init__(self, target: float = -23.0, channel_weights: tp.Sequence[float] | None = None, fs: int | None = None,
                 max_true_peak: float | None = None) -> None:
        super().__init__()
        if not math.isfinite(target):
            raise ValueError(f"target must be a finite loudness in LUFS, got {target!r}")
        if max_true_peak is not None and not math.isfinite(max_true_peak):
            raise ValueError(f"max_true_peak must be None or a finite level in dBTP, got {max_true_peak!r}")
        self.max_true_peak = None if max_true_peak is None else float(max_true_peak)
        self.target = float(target)
        self.channel_weights = None if channel_weights is None else tuple(float(w) for w in channel_weights)
        self.fs = fs

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``scipy on host -- <reason>`` for the measurement of ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"scipy on host -- {x.device.type} tensor"
        if x.dtype not in (torch.float32, torch.float64):
            return f"refused -- {x.dtype} signal (float32 / float64 only)"
        from torchfx_amd.loudness import kweighting_sos

        n = int(x.shape[-1]) if length is None else int(length)
        rows = max(1, x.numel() // max(1, int(x.shape[-1]))) if x.dim() else 1
        try:
            info = _ext().sos_block_energy_plan_info(kweighting_sos(self.fs), rows, n, self.fs, 10)
        except (RuntimeError, ValueError) as e:
            return f"refused -- {e}"
        text = (f"native (sos_block_energy_kernel, {info['nblk']} sub-blocks of 100 ms, {info['nseg']} segment(s) per row; "
                "gating and gain on the device)")
        if self.max_true_peak is None:
            return text
        from torchfx_amd.loudness import default_oversample
        from torchfx_amd.resample import design_taps

        up = default_oversample(self.fs)
        if up == 1:
            return text + " + native (stat_forward, sample peak per row)"
        try:
            tp_info = _ext().true_peak_plan_info(rows, n, up, int(design_taps(up, 1, dtype=x.dtype).numel()), x.dtype)
        except (RuntimeError, ValueError) as e:
            return f"refused -- {e}"
        return text + f" + native (true_peak_kernel, {up}x oversampled, {tp_info['tiles']} tile(s) per row)"

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        if self.fs is None:
            raise ValueError("LoudnessNormalize needs the sample rate: pass fs or pipe a Wave into it (wave | LoudnessNormalize())")
        from torchfx_amd.loudness import integrated_loudness

        loud = integrated_loudness(waveform, self.fs, self.channel_weights)
        gain_db = self.target - loud
        if self.max_true_peak is not None:
            from torchfx_amd.loudness import true_peak

            peak = true_peak(waveform, self.fs)
            gain_db = torch.minimum(gain_db, self.max_true_peak - (peak.amax(-1) if peak.dim() else peak))
        gain = torch.pow(10.0, gain_db / 20.0)
        gain = torch.where(torch.isneginf(loud), torch.ones_like(gain), gain).to(waveform.dtype)
        return waveform * (gain.view(-1, 1, 1) if gain.dim() else gain)

    def extra_repr(self) -> str:
        ceiling = "" if self.max_true_peak is None else f", max_true_peak={self.max_true_peak}"
        return f"target={self.target}, channel_weights={self.channel_weights}, fs={self.fs}{ceiling}"


class Limiter(FX):
    """Look-ahead true-peak limiter: :func:`torchfx_amd.limiter.limit` with the same parameters -- ``ceiling_db`` (dBTP for
    ``detector="true_peak"``, dBFS for ``"sample"``), ``lookahead`` and ``hold`` in seconds, ``link`` (one gain curve per
    ``[C, T]`` signal or batch item), ``oversample``, ``taps`` and ``window``.  ``wave | LoudnessNormalize(-14) | Limiter(-1.0)``
    brings a programme to its target loudness and takes down the peaks that pass the ceiling.

    The sample ceiling ``|y| <= c (1 + u)^2`` always holds; the true peak of the result is measured, not guaranteed (within
    0.001 dB of the ceiling at the default 1.5 ms look-ahead on the material measured, more with a shorter one -- see
    :func:`~torchfx_amd.limiter.limit`).  ``fs`` comes from the ``Wave`` the effect is piped into when it is None.  The gain
    looks ``A - 1`` samples ahead: the limiter is a step of its own in ``Wave.plan()`` and cannot run in a chunked stream --
    :class:`torchfx_amd.realtime.StatefulLimiter` is the effect for that."""

    def __init__(self, ceiling_db: float = -1.0, lookahead: float = 1.5e-3, hold: float = 10e-3, detector: str = "true_peak",
                 link: bool = True, oversample: int | None = None, taps=None, window=None, fs: int | None = None) -> None:
        super().__init__()
        from torchfx_amd.limiter import LimiterParams

        LimiterParams(48000 if fs is None else fs, torch.float32, ceiling_db, 0.0, 0.0, detector, oversample)   # argument errors now
        for name, v in (("lookahead", lookahead), ("hold", hold)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"limit: {name} must be a finite time >= 0 in seconds, got {v!r}")
        self.ceiling_db, self.lookahead, self.hold = float(ceiling_db), float(lookahead), float(hold)
        self.detector, self.link, self.oversample, self.taps, self.window, self.fs = detector, bool(link), oversample, taps, window, fs

    def params(self, dtype: torch.dtype):
        """The call's :class:`torchfx_amd.limiter.LimiterParams` for a signal of ``dtype`` at ``self.fs``."""
        if self.fs is None:
            raise ValueError("Limiter needs the sample rate: pass fs or pipe a Wave into it (wave | Limiter())")
        from torchfx_amd.limiter import LimiterParams

        return LimiterParams(self.fs, dtype, self.ceiling_db, self.lookahead, self.hold, self.detector, self.oversample, self.taps,
                             self.window)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``numpy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"numpy on host -- {x.device.type} tensor"
        try:
            P = self.params(x.dtype)
            n = int(x.shape[-1]) if length is None else int(length)
            info = _ext().limiter_plan_info(n, P.A, P.H, P.up, 0 if P.taps is None else int(P.taps.numel()), x.dtype)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        det = f"{P.up}x oversampled detector" if P.up > 1 else "sample-peak detector"
        return (f"native (limiter_kernel, {det}, look-ahead {P.A} / hold {P.H} samples, {info['tiles']} tile(s) of {info['tile']} "
                "per group; one launch)")

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        if self.fs is None:
            raise ValueError("Limiter needs the sample rate: pass fs or pipe a Wave into it (wave | Limiter())")
        from torchfx_amd.limiter import limit

        return limit(waveform, self.fs, self.ceiling_db, self.lookahead, self.hold, self.detector, self.link, self.oversample,
                     self.taps, self.window)

    def extra_repr(self) -> str:
        return (f"ceiling_db={self.ceiling_db}, lookahead={self.lookahead}, hold={self.hold}, detector={self.detector!r}, "
                f"link={self.link}, fs={self.fs}")


class Compressor(FX):
    """Feed-forward compressor: :func:`torchfx_amd.dynamics.compress` with the same parameters -- ``threshold_db``, ``ratio``
    (``>= 1``, ``inf`` allowed), ``attack`` and ``release`` in seconds, ``knee_db`` (soft-knee width), ``makeup_db`` and ``link``
    (one gain curve per ``[C, T]`` signal or batch item).  ``wave | LoudnessNormalize(-14) | Compressor(-18, 3) | Limiter(-1.0)``
    is the mastering chain.

    The level detector is the smooth decoupled peak detector (log domain, float64 for both signal dtypes); the gain is causal
    with no latency.  ``fs`` comes from the ``Wave`` the effect is piped into when it is None.  Every call starts from silence:
    the compressor is a step of its own in ``Wave.plan()`` and a chunked stream needs
    :class:`torchfx_amd.realtime.StatefulCompressor`, which carries the detector's state from chunk to chunk."""

    def __init__(self, threshold_db: float = -20.0, ratio: float = 4.0, attack: float = 5e-3, release: float = 100e-3,
                 knee_db: float = 6.0, makeup_db: float = 0.0, link: bool = True, fs: int | None = None) -> None:
        super().__init__()
        from torchfx_amd.dynamics import CompressorParams

        CompressorParams(48000 if fs is None else fs, torch.float32, threshold_db, ratio, attack, release, knee_db, makeup_db)   # argument errors now
        self.threshold_db, self.ratio, self.attack, self.release = float(threshold_db), float(ratio), float(attack), float(release)
        self.knee_db, self.makeup_db, self.link, self.fs = float(knee_db), float(makeup_db), bool(link), fs

    def params(self, dtype: torch.dtype):
        """The call's :class:`torchfx_amd.dynamics.CompressorParams` for a signal of ``dtype`` at ``self.fs``."""
        if self.fs is None:
            raise ValueError("Compressor needs the sample rate: pass fs or pipe a Wave into it (wave | Compressor())")
        from torchfx_amd.dynamics import CompressorParams

        return CompressorParams(self.fs, dtype, self.threshold_db, self.ratio, self.attack, self.release, self.knee_db, self.makeup_db)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``numpy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"numpy on host -- {x.device.type} tensor"
        try:
            self.params(x.dtype)
            from torchfx_amd.limiter import _grouping

            n = int(x.shape[-1]) if length is None else int(length)
            groups, channels = _grouping(x, self.link)
            info = _ext().compressor_plan_info(n, groups, channels)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        launches = "one launch" if info["segments"] == 1 else "three launches"
        return (f"native (compressor_kernel, log-domain decoupled peak detector, {info['tiles']} tile(s) of {info['tile']} per group "
                f"in {info['segments']} segment(s); {launches})")

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        if self.fs is None:
            raise ValueError("Compressor needs the sample rate: pass fs or pipe a Wave into it (wave | Compressor())")
        from torchfx_amd.dynamics import compress

        return compress(waveform, self.fs, self.threshold_db, self.ratio, self.attack, self.release, self.knee_db, self.makeup_db,
                        self.link)

    def extra_repr(self) -> str:
        return (f"threshold_db={self.threshold_db}, ratio={self.ratio}, attack={self.attack}, release={self.release}, "
                f"knee_db={self.knee_db}, makeup_db={self.makeup_db}, link={self.link}, fs={self.fs}")


class Gate(FX):
    """Noise gate: :func:`torchfx_amd.gate.gate` with the same parameters -- ``threshold_db`` (the gate opens at or above it),
    ``hysteresis_db`` (it closes that far below), ``range_db`` (the closed gate's attenuation, ``inf`` for silence), ``attack``,
    ``hold`` and ``release`` in seconds and ``link`` (one gain curve per ``[C, T]`` signal or batch item).
    ``wave | Gate(-45) | Compressor(-18, 3) | Limiter(-1.0)`` is the practical chain: the gate goes first, so that no make-up
    gain lifts what lies between the phrases.

    The detector is the sample peak in float64 for both signal dtypes; the gain is causal with no latency.  ``fs`` comes from
    the ``Wave`` the effect is piped into when it is None.  Every call starts closed with its hold counter at zero: the gate is
    a step of its own in ``Wave.plan()`` and a chunked stream needs :class:`torchfx_amd.realtime.StatefulGate`, which carries
    the gain, the decision and the counter from chunk to chunk."""

    def __init__(self, threshold_db: float = -40.0, hysteresis_db: float = 6.0, range_db: float = math.inf, attack: float = 1e-3,
                 hold: float = 50e-3, release: float = 100e-3, link: bool = True, fs: int | None = None) -> None:
        super().__init__()
        from torchfx_amd.gate import GateParams

        GateParams(48000 if fs is None else fs, torch.float32, threshold_db, hysteresis_db, range_db, attack, hold, release)   # argument errors now
        self.threshold_db, self.hysteresis_db, self.range_db = float(threshold_db), float(hysteresis_db), float(range_db)
        self.attack, self.hold, self.release, self.link, self.fs = float(attack), float(hold), float(release), bool(link), fs

    def params(self, dtype: torch.dtype):
        """The call's :class:`torchfx_amd.gate.GateParams` for a signal of ``dtype`` at ``self.fs``."""
        if self.fs is None:
            raise ValueError("Gate needs the sample rate: pass fs or pipe a Wave into it (wave | Gate())")
        from torchfx_amd.gate import GateParams

        return GateParams(self.fs, dtype, self.threshold_db, self.hysteresis_db, self.range_db, self.attack, self.hold, self.release)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``numpy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"numpy on host -- {x.device.type} tensor"
        try:
            P = self.params(x.dtype)
            from torchfx_amd.limiter import _grouping

            n = int(x.shape[-1]) if length is None else int(length)
            groups, channels = _grouping(x, self.link)
            info = _ext().gate_plan_info(n, groups, channels)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        launches = "one launch" if info["segments"] == 1 else "three launches"
        return (f"native (gate_kernel, hysteresis decision and gain smoother as scans, hold H = {P.H} samples, {info['tiles']} tile(s) "
                f"of {info['tile']} per group in {info['segments']} segment(s); {launches})")

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        if self.fs is None:
            raise ValueError("Gate needs the sample rate: pass fs or pipe a Wave into it (wave | Gate())")
        from torchfx_amd.gate import gate

        return gate(waveform, self.fs, self.threshold_db, self.hysteresis_db, self.range_db, self.attack, self.hold, self.release,
                    self.link)

    def extra_repr(self) -> str:
        return (f"threshold_db={self.threshold_db}, hysteresis_db={self.hysteresis_db}, range_db={self.range_db}, "
                f"attack={self.attack}, hold={self.hold}, release={self.release}, link={self.link}, fs={self.fs}")


class ModulatedDelay(FX):
    """The modulated delay line as an effect: :func:`torchfx_amd.modulation.modulated_delay` with a voice table given in
    seconds.  ``voices`` holds 1 to 8 rows ``(delay, depth, rate, phase, gain)``: delay and depth in seconds, rate in Hz, phase
    in cycles; ``pad`` is added to every voice's delay in samples (the cubic interpolant's one sample of headroom).  ``dry``,
    ``spread`` (cycles of LFO phase per channel index), ``shape`` ("sine" / "triangle") and ``interpolation`` ("linear" /
    "cubic") as the function takes them.  :class:`Chorus`, :class:`Flanger` and :class:`Vibrato` only fill the table.

    ``fs`` comes from the ``Wave`` the effect is piped into when it is None.  Every call starts its LFO at position 0 and its
    delay line from silence: the effect is a step of its own in ``Wave.plan()`` (one launch, ``csrc/modulation.hip``), and a
    chunked stream needs the stateful classes of :mod:`torchfx_amd.realtime`, which carry the history and the position."""

    def __init__(self, voices, dry: float = 1.0, spread: float = 0.0, shape: str = "sine", interpolation: str = "linear",
                 fs: int | None = None, pad: float = 0.0) -> None:
        super().__init__()
        self.voices = [tuple(float(t) for t in v) for v in voices]
        self.dry, self.spread, self.shape, self.interpolation, self.fs, self.pad = float(dry), float(spread), shape, interpolation, fs, float(pad)
        self.params(torch.float32, 48000 if fs is None else fs)          # argument errors now

    def voice_table(self, fs: int) -> list[tuple]:
        """The voices as :func:`~torchfx_amd.modulation.modulated_delay` takes them at ``fs``: delay and depth in samples."""
        for v in self.voices:
            if len(v) != 5:
                raise ValueError(f"modulated_delay: a voice must be (delay, depth, rate, phase, gain), got {v!r}")
        return [(d * fs + self.pad, w * fs, r, p, g) for d, w, r, p, g in self.voices]

    def params(self, dtype: torch.dtype, fs: int | None = None):
        """The call's :class:`torchfx_amd.modulation.ModulationParams` for a signal of ``dtype`` at ``fs`` (default ``self.fs``)."""
        fs = self.fs if fs is None else fs
        if fs is None:
            raise ValueError(f"{type(self).__name__} needs the sample rate: pass fs or pipe a Wave into it (wave | {type(self).__name__}())")
        from torchfx_amd.modulation import ModulationParams, _check_fs

        return ModulationParams(fs, dtype, self.voice_table(_check_fs(fs)), self.dry, self.spread, self.shape, self.interpolation)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``numpy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"numpy on host -- {x.device.type} tensor"
        try:
            P = self.params(x.dtype)
            n = int(x.shape[-1]) if length is None else int(length)
            info = _ext().modulated_delay_plan_info(n, P.table, int(x.shape[0]) if x.dim() == 3 else 1,
                                                    int(x.shape[-2]) if x.dim() >= 2 else 1, P.interpolation)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        return (f"native (modulated_delay_kernel, {len(P.table)} voice(s), {P.shape} LFO, {P.interpolation} interpolation, "
                f"{info['tiles']} tile(s) of {info['tile']} per row, {info['batch_groups']} batch group(s) of up to "
                f"{info['batch_items']}; one launch)")

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        from torchfx_amd.modulation import _check_signal, modulate

        _check_signal(waveform, "modulated_delay")
        return modulate(waveform, self.params(waveform.dtype))

    def extra_repr(self) -> str:
        return (f"voices={len(self.voices)}, dry={self.dry}, spread={self.spread}, shape={self.shape!r}, "
                f"interpolation={self.interpolation!r}, fs={self.fs}")


def _seconds(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"modulated_delay: {name} must be a finite time >= 0 in seconds, got {v!r}")
    return float(v)


class Chorus(ModulatedDelay):
    """Chorus: ``voices`` copies of the signal, each delayed by ``delay`` seconds and swept by ``depth`` seconds at ``rate``
    Hz, the voices' LFOs spaced evenly over the cycle (voice ``v`` has phase ``v / voices``) and each mixed in with gain
    ``mix / voices`` next to ``dry = 1 - mix``.  ``spread`` shifts the LFO phase by that many cycles per channel index, which
    widens a stereo signal.  Feed-forward."""

    def __init__(self, rate: float = 1.5, depth: float = 3e-3, delay: float = 20e-3, voices: int = 3, mix: float = 0.5,
                 spread: float = 0.25, shape: str = "sine", interpolation: str = "cubic", fs: int | None = None) -> None:
        if isinstance(voices, bool) or not isinstance(voices, int) or not 1 <= voices <= 8:
            raise ValueError(f"modulated_delay: the number of voices must be in [1, 8], got {voices!r}")
        self.rate, self.depth, self.delay, self.mix = float(rate), _seconds("depth", depth), _seconds("delay", delay), float(mix)
        super().__init__([(self.delay, self.depth, self.rate, v / voices, self.mix / voices) for v in range(voices)],
                         1.0 - self.mix, spread, shape, interpolation, fs)

    def extra_repr(self) -> str:
        return f"rate={self.rate}, depth={self.depth}, delay={self.delay}, mix={self.mix}, " + super().extra_repr()


class Vibrato(ModulatedDelay):
    """Vibrato: the signal alone, read through a delay that swings by ``depth`` seconds around ``depth`` (plus one sample for
    the cubic interpolant) at ``rate`` Hz -- a periodic pitch change.  One voice, no dry part."""

    def __init__(self, rate: float = 5.0, depth: float = 1e-3, shape: str = "sine", interpolation: str = "cubic",
                 fs: int | None = None) -> None:
        self.rate, self.depth = float(rate), _seconds("depth", depth)
        super().__init__([(self.depth, self.depth, self.rate, 0.0, 1.0)], 0.0, 0.0, shape, interpolation, fs,
                         pad=1.0 if interpolation == "cubic" else 0.0)

    def extra_repr(self) -> str:
        return f"rate={self.rate}, depth={self.depth}, " + super().extra_repr()


class Flanger(ModulatedDelay):
    """Flanger: the signal plus one short, slowly swept copy of itself (``delay`` +- ``depth`` seconds at ``rate`` Hz) with
    gain ``mix`` (``-mix`` with ``invert``), which combs the spectrum.  This flanger is **feed-forward**: there is no
    regeneration path from the output back into the delay line."""

    def __init__(self, rate: float = 0.25, depth: float = 2e-3, delay: float = 3e-3, mix: float = 0.5, invert: bool = False,
                 spread: float = 0.0, shape: str = "sine", interpolation: str = "cubic", fs: int | None = None) -> None:
        self.rate, self.depth, self.delay, self.mix, self.invert = float(rate), _seconds("depth", depth), _seconds("delay", delay), float(mix), bool(invert)
        super().__init__([(self.delay, self.depth, self.rate, 0.0, -self.mix if self.invert else self.mix)], 1.0, spread, shape,
                         interpolation, fs)

    def extra_repr(self) -> str:
        return f"rate={self.rate}, depth={self.depth}, delay={self.delay}, mix={self.mix}, invert={self.invert}, " + super().extra_repr()


class Phaser(FX):
    """Phaser: :func:`torchfx_amd.phaser.phase_shift` as an effect -- ``stages`` first-order all-pass sections in series whose
    corner frequency an LFO sweeps exponentially between ``min_freq`` and ``max_freq`` Hz at ``rate`` Hz, mixed with the signal:
    ``dry = 1 - mix`` and ``wet = mix`` (``-mix`` with ``invert``, which moves the notches to where the peaks were).  ``spread``
    shifts the LFO phase by that many cycles per channel index; ``shape`` is "sine" or "triangle".  There is no feedback
    (regeneration) path around the chain.

    ``fs`` comes from the ``Wave`` the effect is piped into when it is None.  Every call starts its sweep at position 0 and its
    sections from silence: the effect is a step of its own in ``Wave.plan()`` (``csrc/phaser.hip``), and a chunked stream needs
    :class:`torchfx_amd.realtime.StatefulPhaser`, which carries the sections' states and the position."""

    def __init__(self, rate: float = 0.5, min_freq: float = 200.0, max_freq: float = 2000.0, stages: int = 4, mix: float = 0.5,
                 invert: bool = False, spread: float = 0.0, shape: str = "sine", fs: int | None = None) -> None:
        super().__init__()
        self.rate, self.min_freq, self.max_freq, self.stages = rate, min_freq, max_freq, stages
        self.mix, self.invert, self.spread, self.shape, self.fs = mix, bool(invert), spread, shape, fs
        self.params(torch.float32, 48000 if fs is None else fs)         # argument errors now

    def params(self, dtype: torch.dtype, fs: int | None = None):
        """The call's :class:`torchfx_amd.phaser.PhaserParams` for a signal of ``dtype`` at ``fs`` (default ``self.fs``)."""
        fs = self.fs if fs is None else fs
        if fs is None:
            raise ValueError(f"{type(self).__name__} needs the sample rate: pass fs or pipe a Wave into it (wave | {type(self).__name__}())")
        from torchfx_amd.phaser import PhaserParams, _real

        mix = _real("mix", self.mix)
        return PhaserParams(fs, dtype, self.stages, self.min_freq, self.max_freq, self.rate, 0.0, 1.0 - mix, -mix if self.invert else mix,
                            self.spread, self.shape)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``numpy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"numpy on host -- {x.device.type} tensor"
        try:
            P = self.params(x.dtype)
            n = int(x.shape[-1]) if length is None else int(length)
            info = _ext().phaser_plan_info(n, max(1, math.prod(x.shape[:-1])), int(x.shape[-2]) if x.dim() >= 2 else 1, P.stages)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        launches = "one launch" if info["segments"] == 1 else "two launches"
        return (f"native (phaser_kernel, {P.stages} stage(s), {P.shape} LFO, {info['tiles']} tile(s) of {info['tile']} per row in "
                f"{info['segments']} segment(s); {launches})")

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        from torchfx_amd.phaser import _check_signal, phase_shift_run

        _check_signal(waveform, "phase_shift")
        return phase_shift_run(waveform, self.params(waveform.dtype))[0]

    def extra_repr(self) -> str:
        return (f"rate={self.rate}, min_freq={self.min_freq}, max_freq={self.max_freq}, stages={self.stages}, mix={self.mix}, "
                f"invert={self.invert}, spread={self.spread}, shape={self.shape!r}, fs={self.fs}")


class Epilogued(FX):
    """Planner product (``Wave.plan()``, ``fuse_epilogue``): a filter followed by ``Gain`` and / or ``Normalize``
    whose elementwise work rides on the filter's own kernel.  ``producer`` is an SOS filter / cascade or an
    FFT-mode FIR; its kernel multiplies and clips the samples it stores exactly like the ``Gain`` pass would
    (bit-identical) and gathers the statistic ``Normalize`` needs, so the run costs the filter's 8 B/sample
    plus, with a ``Normalize``, one apply pass -- instead of 8 + 8 + 4 + 8.  Nothing on the member modules is
    modified; a lone stateful IIR keeps carrying its state on the user's object."""

    def __init__(self, producer: nn.Module, gain: "Gain | None", norm: "Normalize | None") -> None:
        super().__init__()
        self.producer, self.gain, self.norm = producer, gain, norm

    @staticmethod
    def norm_kind(norm: "Normalize") -> tuple[str, bool] | None:
        """(statistic, per_row) of the strategies with a streaming reduction; None for the others."""
        st = norm.strategy
        if type(st) is PeakNormalizationStrategy:
            return "absmax", False
        if type(st) is RMSNormalizationStrategy:
            return "sumsq", False
        if type(st) is PerChannelNormalizationStrategy:
            return "absmax", True
        return None

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        E = _ext()
        g = 1.0 if self.gain is None else self.gain.linear_gain()
        kind = self.norm_kind(self.norm) if self.norm is not None else None
        if kind is not None and kind[1]:
            assert x.ndim >= 2, "Waveform must have at least 2 dimensions (channels, time)."
            if x.ndim not in (2, 3):
                raise ValueError("Waveform must have shape (C, T) or (B, C, T)")
        ep = E.Epilogue(gain=1.0 if g is None else g, clamp=bool(self.gain is not None and self.gain.clamp),
                        stat=None if kind is None else kind[0], per_row=bool(kind and kind[1]))
        y = self.producer(x, epilogue=ep)
        if kind is not None:
            y = E.normalize_apply(y, ep.stat_value, self.norm.peak, E.STAT_ABSMAX if kind[0] == "absmax" else E.STAT_RMS, kind[1])
        return y


class Freeverb(FX):
    """Freeverb room reverb (Jezar at Dreampoint's Schroeder-Moorer network, public domain):
    :func:`torchfx_amd.reverb.freeverb` with the same parameters -- ``room_size``, ``damping``, ``wet``, ``dry`` and ``width`` in
    ``[0, 1]`` and ``tail`` in seconds (``>= 0``: that much ring-out is appended to the signal).  Per channel eight feedback combs
    with a damping low-pass in the loop, then four all-passes, at Freeverb's tunings scaled from 44.1 kHz to ``fs``; signals
    of one or two channels, all arithmetic in float64.  ``wet = 0, dry = 0.5`` returns the input bit for bit.

    ``fs`` comes from the ``Wave`` the effect is piped into when it is None.  Every call starts from silent delay lines: the
    reverb is a step of its own in ``Wave.plan()`` (``csrc/reverb.hip``: one workgroup per channel of a batch item) and a
    chunked stream needs :class:`torchfx_amd.realtime.StatefulFreeverb`, which carries the lines from chunk to chunk."""

    def __init__(self, room_size: float = 0.5, damping: float = 0.5, wet: float = 1.0 / 3.0, dry: float = 0.5, width: float = 1.0,
                 tail: float = 0.0, fs: int | None = None) -> None:
        super().__init__()
        from torchfx_amd.reverb import FreeverbParams

        FreeverbParams(48000 if fs is None else fs, room_size, damping, wet, dry, width, tail)      # argument errors now
        self.room_size, self.damping, self.wet, self.dry = float(room_size), float(damping), float(wet), float(dry)
        self.width, self.tail, self.fs = float(width), float(tail), fs

    def params(self):
        """The call's :class:`torchfx_amd.reverb.FreeverbParams` at ``self.fs``."""
        if self.fs is None:
            raise ValueError(f"{type(self).__name__} needs the sample rate: pass fs or pipe a Wave into it (wave | Freeverb())")
        from torchfx_amd.reverb import FreeverbParams

        return FreeverbParams(self.fs, self.room_size, self.damping, self.wet, self.dry, self.width, self.tail)

    def output_length(self, length: int) -> int:
        """Samples per row this effect returns for rows of ``length`` samples: ``length + floor(tail fs + 0.5)``."""
        return int(length) + (self.params().tail_samples if self.fs is not None else 0)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``numpy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"numpy on host -- {x.device.type} tensor"
        try:
            from torchfx_amd.reverb import _shape

            F = self.params()
            batch, channels, T = _shape(x)
            P = F.bank(channels)
            info = _ext().freeverb_plan_info(T if length is None else int(length), P.comb, P.allpass, batch, channels, P.wet2,
                                             self._call_tail(F))
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        where = "LDS" if info["placement"] == "lds" else "a global workspace"
        launches = "one launch" if info["launches"] == 1 else "two launches (banks, then the cross-channel mix)"
        return (f"native (freeverb_kernel, one workgroup per bank and one wave per comb, blocks of {info['block']} samples, "
                f"delay lines in {where}; {launches})")

    def _call_tail(self, F) -> int:
        return F.tail_samples

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        from torchfx_amd.reverb import freeverb

        self.params()
        return freeverb(waveform, self.fs, self.room_size, self.damping, self.wet, self.dry, self.width, self.tail)

    def extra_repr(self) -> str:
        return (f"room_size={self.room_size}, damping={self.damping}, wet={self.wet}, dry={self.dry}, width={self.width}, "
                f"tail={self.tail}, fs={self.fs}")


class Waveshaper(FX):
    """Oversampled waveshaping as an effect: :func:`torchfx_amd.waveshaper.waveshape` with the same parameters -- ``shape``
    ("hard", "cubic", "tanh"; default "tanh") or a ``curve`` table of 2 to 4096 points over ``[-1, 1]`` (WebAudio's
    ``WaveShaperNode`` rule), ``drive_db``, ``bias``, ``oversample`` (1, 2, 4 or 8), ``mix``, ``output_db`` and the resampling
    ``window``.  It needs no sample rate.  Every call zero-pads its edges: the effect is a step of its own in ``Wave.plan()``
    (one launch, ``csrc/waveshaper.hip``), and the stream processors take it with ``oversample=1`` only:
    :class:`torchfx_amd.realtime.StatefulWaveshaper` / ``StatefulDistortion`` are the effects for a chunked stream."""

    def __init__(self, shape: str | None = None, drive_db: float = 0.0, bias: float = 0.0, oversample: int = 4, mix: float = 1.0,
                 output_db: float = 0.0, curve=None, window=("kaiser", 5.0)) -> None:
        super().__init__()
        self.shape, self.drive_db, self.bias, self.oversample, self.mix = shape, drive_db, bias, oversample, mix
        self.output_db, self.curve, self.window = output_db, curve, window
        self.params()                                                    # argument errors now

    def params(self):
        """The call's :class:`torchfx_amd.waveshaper.ShaperParams`."""
        from torchfx_amd.waveshaper import ShaperParams

        return ShaperParams(self.shape, self.drive_db, self.bias, self.oversample, self.mix, self.output_db, self.curve, self.window)

    def route(self, x: Tensor, length: int | None = None) -> str:
        """``native (...)`` or ``scipy on host -- <reason>`` for ``x`` (rows of ``length`` samples, default x's)."""
        if not x.is_cuda:
            return f"scipy on host -- {x.device.type} tensor"
        if x.dtype not in (torch.float32, torch.float64):
            return f"refused -- {x.dtype} signal (float32 / float64 only)"
        try:
            P = self.params()
            up, dn = P.taps(x.dtype)
            n = int(x.shape[-1]) if length is None else int(length)
            info = _ext().waveshaper_plan_info(n, P.oversample, 0 if up is None else up.numel(), 0 if dn is None else dn.numel(),
                                               0 if P.curve is None else P.curve.size, x.dtype)
        except (RuntimeError, ValueError, TypeError) as e:
            return f"refused -- {e}"
        if P.oversample == 1:
            return f"native (waveshaper_plain_kernel, L = 1, {P.shape}, no filters; one launch)"
        return (f"native (waveshaper_kernel, L = {P.oversample}, {P.shape}, {info['taps_up']} taps per phase up and {info['taps_dn']} "
                f"taps down, {info['tiles']} tile(s) of {info['tile']} per row, {info['lds_bytes']} B of LDS; one launch)")

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        from torchfx_amd.waveshaper import shape_signal

        return shape_signal(waveform, self.params())

    def extra_repr(self) -> str:
        what = f"curve={len(self.curve)} points" if self.curve is not None else f"shape={self.params().shape!r}"
        return (f"{what}, drive_db={self.drive_db}, bias={self.bias}, oversample={self.oversample}, mix={self.mix}, "
                f"output_db={self.output_db}")


class Distortion(Waveshaper):
    """Distortion: a :class:`Waveshaper` with 12 dB of drive into ``tanh`` at 4x oversampling unless told otherwise."""

    def __init__(self, drive_db: float = 12.0, shape: str = "tanh", bias: float = 0.0, oversample: int = 4, mix: float = 1.0,
                 output_db: float = 0.0) -> None:
        super().__init__(shape, drive_db, bias, oversample, mix, output_db)


class Reverb(FX):
    """``y[n] = x[n] + mix * decay * x[n - delay]`` -- the reference's "reverb" is one feed-forward
    tap (``effect.py:789-931`` over ``delay_line_forward``, ``_csrc/cpu/delay_cpu.cpp:17-41``); a
    signal not longer than the delay is returned unchanged (the same tensor)."""

    def __init__(self, delay: int = 4410, decay: float = 0.5, mix: float = 0.5) -> None:
        super().__init__()
        assert delay > 0, "Delay must be positive."
        assert 0 < decay < 1, "Decay must be between 0 and 1."
        assert 0 <= mix <= 1, "Mix must be between 0 and 1."
        self.delay, self.decay, self.mix = delay, decay, mix

    @torch.no_grad()
    def forward(self, waveform: Tensor) -> Tensor:
        if waveform.size(-1) <= self.delay:
            return waveform
        from torchfx_amd._ops import delay_line_forward

        return delay_line_forward(waveform, self.delay, self.decay, self.mix)


# ------------------------------------------------------------------------------- Delay
class DelayStrategy(abc.ABC):
    """How the delayed copies are laid out (``effect.py:934-1023``): ``apply_delay(waveform, delay_samples, taps, feedback)``
    returns the wet signal, ``delay_samples * taps`` samples longer than the input, tap ``i`` delayed by ``i * delay_samples``
    with gain ``feedback ** (i - 1)``."""

    @abc.abstractmethod
    def apply_delay(self, waveform: Tensor, delay_samples: int, taps: int, feedback: float) -> Tensor: ...


def _tap_sum(dst: Tensor, src: Tensor, delay_samples: int, taps: int, feedback: float, tap_filter=None) -> None:
    """``dst[..., i*D : i*D + T] += src * feedback ** (i - 1)`` for the taps ``tap_filter`` accepts, in tap order -- one
    multiply and one add per tap, as the reference's strategies do."""
    T = src.size(-1)
    for i in range(1, taps + 1):
        if tap_filter is not None and not tap_filter(i):
            continue
        start = delay_samples * i
        n = min(T, dst.size(-1) - start)
        if n > 0:
            dst[..., start:start + n] += src[..., :n] * (1.0 if i == 1 else feedback ** (i - 1))


class MonoDelayStrategy(DelayStrategy):
    """Every channel delays itself (``effect.py:1026-1151``), any shape ``(..., time)``."""

    def apply_delay(self, waveform: Tensor, delay_samples: int, taps: int, feedback: float) -> Tensor:
        shape = list(waveform.shape)
        shape[-1] += delay_samples * taps
        delayed = torch.zeros(shape, dtype=waveform.dtype, device=waveform.device)
        _tap_sum(delayed, waveform, delay_samples, taps, feedback)
        return delayed


class PingPongDelayStrategy(DelayStrategy):
    """Echoes bounce between the channels of a stereo pair (``effect.py:1154-1305``): odd taps carry the left channel into
    the right one, even taps the right into the left.  Input that is not ``(..., 2, time)`` is delayed as mono."""

    def apply_delay(self, waveform: Tensor, delay_samples: int, taps: int, feedback: float) -> Tensor:
        if waveform.ndim < 2 or waveform.size(-2) != 2:
            return MonoDelayStrategy().apply_delay(waveform, delay_samples, taps, feedback)
        shape = list(waveform.shape)
        shape[-1] += delay_samples * taps
        delayed = torch.zeros(shape, dtype=waveform.dtype, device=waveform.device)
        _tap_sum(delayed[..., 1, :], waveform[..., 0, :], delay_samples, taps, feedback, lambda i: i % 2 == 1)
        _tap_sum(delayed[..., 0, :], waveform[..., 1, :], delay_samples, taps, feedback, lambda i: i % 2 == 0)
        return delayed


class Delay(FX):
    """Multi-tap delay with a dry/wet mix (``effect.py:1308-1538``)::

        delayed[n] = sum_{i=1..taps} feedback^(i-1) * x[n - i * delay_samples]
        y = torch.lerp(x zero-padded to the delayed length, delayed, mix)

    ``delay_samples`` directly, or ``bpm`` + ``delay_time`` (a :class:`~torchfx_amd.typing.MusicalTime` string such as
    ``"1/8"``, ``"1/4d"``, ``"1/8t"``) at ``fs``; with ``fs=None`` the rate comes from the ``Wave`` the effect is piped
    into and the delay is worked out at the first ``forward``.  The output is ``taps * delay_samples`` samples longer
    than the input.

    Device float32 / float64 signals with the stock strategies run one HIP launch (:func:`torchfx_ext.delay_forward`,
    bit-identical to the composition on the device); CPU tensors, other dtypes and custom strategies run the reference's
    torch composition (``strategy.apply_delay`` then ``torch.lerp``)."""

    def __init__(self, delay_samples: int | None = None, bpm: float | None = None, delay_time: str = "1/8",
                 fs: int | None = None, feedback: float = 0.3, mix: float = 0.2, taps: int = 3,
                 strategy: DelayStrategy | None = None) -> None:
        super().__init__()
        self.fs, self.bpm, self.delay_time = fs, bpm, delay_time
        if delay_samples is not None:
            assert delay_samples > 0, "Delay samples must be positive."
            self.delay_samples = delay_samples
            self._needs_calculation = False
        else:
            assert bpm is not None, "BPM must be provided if delay_samples is not set."
            assert bpm > 0, "BPM must be positive."
            if fs is not None:
                assert fs > 0, "Sample rate (fs) must be positive."
                self.delay_samples = self._calculate_delay_samples(bpm, delay_time, fs)
                self._needs_calculation = False
            else:
                self.delay_samples = None      # worked out at the first forward, once a Wave has set fs
                self._needs_calculation = True
        assert 0 <= feedback <= 0.95, "Feedback must be between 0 and 0.95."
        assert 0 <= mix <= 1, "Mix must be between 0 and 1."
        assert taps >= 1, "Taps must be at least 1."
        self.feedback, self.mix, self.taps = feedback, mix, taps
        self.strategy = strategy or MonoDelayStrategy()

    @staticmethod
    def _calculate_delay_samples(bpm: float, delay_time: str, fs: int) -> int:
        from torchfx_amd.typing import MusicalTime

        return int(MusicalTime.from_string(delay_time).duration_seconds(bpm) * fs)

    def _resolve(self) -> None:
        if self._needs_calculation:
            assert self.fs is not None, ("Sample rate (fs) is required for BPM-synced delay."
                                         "Either provide fs parameter or use with Wave pipeline (wave | delay).")
            assert self.fs > 0, "Sample rate (fs) must be positive."
            assert self.bpm is not None, "BPM must be set for BPM-synced delay."
            self.delay_samples = self._calculate_delay_samples(self.bpm, self.delay_time, self.fs)
            self._needs_calculation = False

    def native_refusal(self, x: Tensor) -> str | None:
        """None when ``x`` runs the HIP kernel, else why it takes the torch composition."""
        if type(self.strategy) not in (MonoDelayStrategy, PingPongDelayStrategy):
            return f"custom strategy {type(self.strategy).__name__}"
        if not x.is_cuda:
            return f"{x.device.type} tensor"
        if x.dtype not in (torch.float32, torch.float64):
            return f"{x.dtype} signal"
        if x.dim() == 0:
            return "0-d tensor"
        return None

    def pingpong(self, x: Tensor) -> bool:
        return isinstance(self.strategy, PingPongDelayStrategy) and x.dim() >= 2 and x.size(-2) == 2

    @torch.no_grad()
    def forward(self, waveform: Tensor, epilogue=None) -> Tensor:
        self._resolve()
        if self.native_refusal(waveform) is None:
            return _ext().delay_forward(waveform, self.delay_samples, self.taps, self.feedback, self.mix,
                                        self.pingpong(waveform), epilogue=epilogue)
        if epilogue is not None:
            raise RuntimeError(f"Delay: no fused epilogue on the torch composition ({self.native_refusal(waveform)})")
        delayed = self.strategy.apply_delay(waveform, self.delay_samples, self.taps, self.feedback)
        if waveform.size(-1) < delayed.size(-1):
            padded = torch.zeros(*waveform.shape[:-1], delayed.size(-1), dtype=waveform.dtype, device=waveform.device)
            padded[..., :waveform.size(-1)] = waveform
            waveform = padded
        return torch.lerp(waveform, delayed, self.mix)
