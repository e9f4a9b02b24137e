"""What the stream processors and Wave refuse, pinned word for word: every refusal's exception class and complete message
(``==``, not a pattern), which effect a message names when several qualify, and the order in which the refusals fire.  Host only:
every refusal comes from a constructor (or ``Wave.__or__``) before any signal is touched."""
import pytest
import torch
from torch import nn

from torchfx_amd import filter as F
from torchfx_amd.effect import (FX, Chorus, Compressor, Distortion, Flanger, Freeverb, Gain, Limiter, LoudnessNormalize, ModulatedDelay,
                                Vibrato, Waveshaper)
from torchfx_amd.realtime import (AudioBackend, RealtimeProcessor, StatefulDistortion, StatefulLimiter, StatefulResample,
                                  StatefulWaveshaper, StreamConfig, StreamProcessor)
from torchfx_amd.resample import Resample
from torchfx_amd.wave import Wave

FS = 48000
WHO = ("StreamProcessor", "RealtimeProcessor")


class Wrap(FX):
    """An effect that holds another one inside an ``nn.Sequential``: not a top-level effect of the chain."""

    def __init__(self, *inner):
        super().__init__()
        self.inner = nn.Sequential(Gain(0.5), *inner)

    def forward(self, x):
        return self.inner(x)


class Null(AudioBackend):
    def open_stream(self, config, callback=None):
        raise AssertionError("the refusal comes before a stream is opened")

    def start(self): ...
    def stop(self): ...
    def close(self): ...


class Sweep(ModulatedDelay):
    """A bare ModulatedDelay subclass: none of Chorus, Flanger, Vibrato."""

    def __init__(self):
        super().__init__([(5e-3, 1e-3, 0.5, 0.0, 1.0)])


class Fold(Waveshaper):
    """A Waveshaper subclass that is not Distortion."""


def build(who, effects, **kw):
    if who == "StreamProcessor":
        return StreamProcessor(effects, device="cpu", **kw)
    return RealtimeProcessor(effects, Null(), StreamConfig(), device="cpu", **kw)


def modulation(name, stateful):
    return (f"{name} cannot run in {{who}}: every call starts its LFO at position 0 and its delay line from silence, so a chunked "
            f"stream would restart the sweep and drop the delayed samples at every chunk start; use {stateful} in its place, or run "
            f"the whole signal (wave | {name}(...)) before or after streaming")


def waveshaper(name, stateful):
    return (f"{name} with oversample=2 cannot run in {{who}}: every call zero-pads the edges of its resampling filters, so a chunked "
            f"stream would click at every chunk seam; use {stateful}(...) in its place, oversample=1 (memoryless), or run the whole "
            f"signal (wave | {name}(...)) before or after streaming")


LIMITER = ("Limiter cannot run in {who}: its gain looks A - 1 samples ahead (the look-ahead), which a chunked stream has not seen yet; "
           "a streaming limiter that carries that history is not provided by Limiter itself -- use StatefulLimiter(...) in its place, "
           "or limit the whole signal (wave | Limiter(...)) before or after streaming")

# (id, constructor of the plain effect, the message with {who} left open)
PLAIN = [
    ("zero_phase", lambda: F.ZeroPhase(F.LoButterworth(1000, fs=FS)),
     "ZeroPhase cannot run in {who}: zero-phase filtering is non-causal -- its backward pass starts at the end of the signal, which a "
     "chunked stream has not seen yet; filter the whole signal (wave | ZeroPhase(...) or sosfiltfilt) before or after streaming"),
    ("loudness", lambda: LoudnessNormalize(-14.0),
     "LoudnessNormalize cannot run in {who}: integrated loudness is a measurement of the whole signal (its relative gate depends on "
     "every block), which a chunked stream has not seen yet; normalise the whole signal (wave | LoudnessNormalize(...)) before or "
     "after streaming"),
    ("limiter", lambda: Limiter(-1.0, fs=FS), LIMITER),
    ("compressor", lambda: Compressor(fs=FS),
     "Compressor cannot run in {who}: every call starts its level detector from silence, so a chunked stream would drop the envelope "
     "at every chunk start; use StatefulCompressor(...) in its place, or compress the whole signal (wave | Compressor(...)) before or "
     "after streaming"),
    ("chorus", lambda: Chorus(fs=FS), modulation("Chorus", "StatefulChorus(...)")),
    ("flanger", lambda: Flanger(fs=FS), modulation("Flanger", "StatefulFlanger(...)")),
    ("vibrato", lambda: Vibrato(fs=FS), modulation("Vibrato", "StatefulVibrato(...)")),
    ("modulated_delay_subclass", Sweep, modulation("Sweep", "a stateful class (StatefulChorus, StatefulFlanger, StatefulVibrato)")),
    ("freeverb", lambda: Freeverb(fs=FS),
     "Freeverb cannot run in {who}: every call starts from silent delay lines, so a chunked stream would cut the room's tail at every "
     "chunk start; use StatefulFreeverb(...) in its place, or run the whole signal (wave | Freeverb(...)) before or after streaming"),
    ("waveshaper", lambda: Waveshaper("hard", oversample=2), waveshaper("Waveshaper", "StatefulWaveshaper")),
    ("distortion", lambda: Distortion(oversample=2), waveshaper("Distortion", "StatefulDistortion")),
    ("waveshaper_subclass", lambda: Fold("hard", oversample=2), waveshaper("Fold", "StatefulWaveshaper")),
]
RESAMPLE = ("Resample cannot run in StreamProcessor: resampling each chunk on its own leaves a seam at every chunk boundary; use "
            "StatefulResample as a top-level effect of the chain, or resample the whole signal (Wave.resample) before or after "
            "streaming")
NO_STATEFUL_RESAMPLE = ("StatefulResample cannot run in RealtimeProcessor: a sound card's output block has the input block's length "
                        "and sample rate; resample with StreamProcessor or Wave.resample instead")
TOP_LEVEL = ("{label} must be a top-level effect of the chain in {who}: the processor flushes what it holds back at the end of the "
             "stream")
SHAPERS = "StatefulWaveshaper / StatefulDistortion"
OVERLAP = ("A chain with a {name} needs overlap = 0, got 1: the effect holds outputs back, so a chunk's dropped overlap samples have "
           "no counterpart in its output")


def refused(exc, text, fn):
    with pytest.raises(exc) as info:
        fn()
    assert type(info.value) is exc
    assert str(info.value) == text


@pytest.mark.parametrize("who", WHO)
@pytest.mark.parametrize("nested", [False, True], ids=["top_level", "nested"])
@pytest.mark.parametrize("make, text", [p[1:] for p in PLAIN], ids=[p[0] for p in PLAIN])
def test_a_plain_effect_is_refused(oracle_backend, make, text, nested, who):
    effects = [F.HiButterworth(100, fs=FS), Wrap(make())] if nested else [make()]
    refused(TypeError, text.format(who=who), lambda: build(who, effects))


@pytest.mark.parametrize("who", WHO)
@pytest.mark.parametrize("nested", [False, True], ids=["top_level", "nested"])
def test_a_plain_resample_is_refused(oracle_backend, nested, who):
    """RealtimeProcessor has no text of its own for it: the refusal is that of the StreamProcessor it runs its blocks through."""
    effects = [Gain(0.5), Wrap(Resample(16000))] if nested else [Gain(0.5), Resample(16000)]
    refused(TypeError, RESAMPLE, lambda: build(who, effects))


@pytest.mark.parametrize("who", WHO)
@pytest.mark.parametrize("make, label", [(StatefulLimiter, "StatefulLimiter"), (StatefulWaveshaper, SHAPERS), (StatefulDistortion, SHAPERS)],
                         ids=["limiter", "waveshaper", "distortion"])
def test_a_nested_hold_back_effect_is_refused(oracle_backend, make, label, who):
    refused(TypeError, TOP_LEVEL.format(label=label, who=who), lambda: build(who, [Gain(0.5), Wrap(make())]))
    refused(TypeError, TOP_LEVEL.format(label=label, who=who), lambda: build(who, [Wrap(make(aligned=False))]))


def test_a_nested_stateful_resample_is_refused(oracle_backend):
    refused(TypeError, RESAMPLE, lambda: build("StreamProcessor", [Gain(0.5), Wrap(StatefulResample(16000))]))
    refused(TypeError, NO_STATEFUL_RESAMPLE, lambda: build("RealtimeProcessor", [Gain(0.5), Wrap(StatefulResample(16000))]))


@pytest.mark.parametrize("make, name", [(lambda: StatefulResample(16000), "StatefulResample"), (StatefulLimiter, "StatefulLimiter"),
                                        (StatefulWaveshaper, "StatefulWaveshaper"), (StatefulDistortion, "StatefulDistortion")],
                         ids=["resample", "limiter", "waveshaper", "distortion"])
def test_overlap_with_one_hold_back_effect(make, name):
    refused(ValueError, OVERLAP.format(name=name), lambda: StreamProcessor([Gain(0.5), make()], chunk_size=1000, overlap=1, device="cpu"))


def test_overlap_names_a_resampler_before_a_limiter_before_a_shaper():
    def chain(*effects):
        return lambda: StreamProcessor(list(effects), chunk_size=1000, overlap=1, device="cpu")

    refused(ValueError, OVERLAP.format(name="StatefulResample"), chain(StatefulDistortion(), StatefulLimiter(), StatefulResample(16000)))
    refused(ValueError, OVERLAP.format(name="StatefulLimiter"), chain(StatefulWaveshaper(), StatefulLimiter()))
    refused(ValueError, OVERLAP.format(name="StatefulDistortion"), chain(StatefulDistortion(), StatefulWaveshaper()))


def test_the_realtime_processor_refuses_aligned_streams(oracle_backend):
    refused(TypeError,
            "StatefulLimiter(aligned=True) cannot run in RealtimeProcessor: it returns the outputs a block completes, none for the "
            "first blocks, and a sound card's output block has the input block's length; construct it with aligned=False (constant "
            "latency: the result delayed by StatefulLimiter.latency samples)",
            lambda: build("RealtimeProcessor", [Gain(0.5), StatefulLimiter()]))
    for make in (StatefulWaveshaper, StatefulDistortion):
        refused(TypeError,
                f"{make.__name__}(aligned=True) cannot run in RealtimeProcessor: it returns the outputs a block completes, fewer for "
                "the first block, and a sound card's output block has the input block's length; construct it with aligned=False "
                "(constant latency: the result delayed by its `latency` samples)",
                lambda make=make: build("RealtimeProcessor", [Gain(0.5), make()]))
    p = build("RealtimeProcessor", [StatefulLimiter(aligned=False), StatefulWaveshaper(aligned=False), StatefulDistortion(aligned=False)])
    assert len(p.effects) == 3


def test_the_realtime_processor_refuses_a_stateful_resample(oracle_backend):
    refused(TypeError, NO_STATEFUL_RESAMPLE, lambda: build("RealtimeProcessor", [Gain(1.0), StatefulResample(16000)]))


@pytest.mark.parametrize("make, text", [
    (lambda: StatefulResample(16000),
     "StatefulResample is for chunked streams (StreamProcessor): a Wave is a whole signal, and a stream's forward holds back its last "
     "outputs; pipe it through Resample or call Wave.resample instead"),
    (StatefulLimiter,
     "StatefulLimiter is for chunked streams (StreamProcessor, RealtimeProcessor): a Wave is a whole signal, and a stream's forward "
     "holds back its last outputs; pipe it through Limiter instead"),
    (StatefulWaveshaper,
     "StatefulWaveshaper / StatefulDistortion are for chunked streams (StreamProcessor, RealtimeProcessor): a Wave is a whole signal, "
     "and a stream's forward holds back its last outputs; pipe it through Waveshaper or Distortion instead"),
    (StatefulDistortion,
     "StatefulWaveshaper / StatefulDistortion are for chunked streams (StreamProcessor, RealtimeProcessor): a Wave is a whole signal, "
     "and a stream's forward holds back its last outputs; pipe it through Waveshaper or Distortion instead"),
], ids=["resample", "limiter", "waveshaper", "distortion"])
def test_wave_refuses_the_stream_classes(make, text):
    w = Wave(torch.zeros(2, 100), FS, device="cpu")
    refused(TypeError, text, lambda: w | make())
    refused(TypeError, text, lambda: w | nn.Sequential(Gain(0.5), make()))


def test_wave_names_a_resampler_before_a_limiter_before_a_shaper():
    w = Wave(torch.zeros(2, 100), FS, device="cpu")
    with pytest.raises(TypeError) as info:
        w | nn.Sequential(StatefulDistortion(), StatefulLimiter(), StatefulResample(16000))
    assert str(info.value).startswith("StatefulResample is for chunked streams (StreamProcessor): ")
    with pytest.raises(TypeError) as info:
        w | nn.Sequential(StatefulDistortion(), StatefulLimiter())
    assert str(info.value).startswith("StatefulLimiter is for chunked streams (StreamProcessor, RealtimeProcessor): ")


@pytest.mark.parametrize("who", WHO)
def test_the_refusals_fire_in_a_fixed_order(oracle_backend, who):
    """Zero-phase, loudness, limiter, compressor, modulation, freeverb, waveshaper, resample: a limiter next to a compressor in one
    effect raises the limiter's text, whichever comes first inside it."""
    refused(TypeError, LIMITER.format(who=who), lambda: build(who, [Wrap(Compressor(fs=FS), Limiter(-1.0, fs=FS))]))
    refused(TypeError, LIMITER.format(who=who), lambda: build(who, [Wrap(Limiter(-1.0, fs=FS), Compressor(fs=FS))]))
    refused(TypeError, TOP_LEVEL.format(label="StatefulLimiter", who=who), lambda: build(who, [Wrap(Compressor(fs=FS), StatefulLimiter())]))
    refused(TypeError, PLAIN[3][2].format(who=who), lambda: build(who, [Wrap(StatefulDistortion(), Compressor(fs=FS))]))


@pytest.mark.parametrize("who", WHO)
def test_what_is_not_a_refusal(oracle_backend, who):
    """A memoryless waveshaper streams as it is, and the stream classes are taken at the top level."""
    p = build(who, [Waveshaper("hard", oversample=1), Wrap(Distortion(oversample=1))])
    assert len(p.effects) == 2
    p = build(who, [Gain(0.5), StatefulLimiter(aligned=False), StatefulDistortion(aligned=False)])
    assert len(p.effects) == 3


def test_effects_must_be_fx():
    refused(TypeError, "All effects must inherit from FX when used in StreamProcessor", lambda: build("StreamProcessor", [nn.Identity()]))
    refused(TypeError, "All effects must inherit from FX when used in RealtimeProcessor", lambda: build("RealtimeProcessor", [nn.Identity()]))
