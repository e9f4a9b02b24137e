"""The BPM-synced multi-tap Delay without a GPU: MusicalTime, the effect's validation and lazy sample rate, the CPU
composition against the reference's own output (tests/golden/delay_fx.npz, tools/make_delay_golden.py), the op's Meta
shape, the C ABI's argument checks and the planner's treatment of a Delay."""
import ctypes
import os

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("s,num,den,mod,frac", [("1/4", 1, 4, "", 0.25), ("1/8", 1, 8, "", 0.125), ("3/16", 3, 16, "", 0.1875),
                                                ("1/8d", 1, 8, "d", 0.1875), ("1/4d", 1, 4, "d", 0.375),
                                                ("1/8t", 1, 8, "t", 0.125 / 3)])
def test_musical_time_fraction(s, num, den, mod, frac):
    from torchfx_amd.typing import MusicalTime
    mt = MusicalTime.from_string(s)
    assert (mt.numerator, mt.denominator, mt.modifier) == (num, den, mod)
    assert mt.fraction() == pytest.approx(frac)


@pytest.mark.parametrize("s,bpm,sec", [("1/4", 120, 0.5), ("1/8", 120, 0.25), ("1/8d", 120, 0.375), ("1/1", 60, 4.0)])
def test_musical_time_duration(s, bpm, sec):
    from torchfx_amd.typing import MusicalTime
    assert MusicalTime.from_string(s).duration_seconds(bpm) == pytest.approx(sec)
    assert MusicalTime.from_string(s).duration_seconds(bpm, beats_per_bar=3) == pytest.approx(sec * 3 / 4)


@pytest.mark.parametrize("bad", ["invalid", "1/x", "1-4", "1/8x", "", "1/8dd", " 1/8"])
def test_musical_time_rejects(bad):
    from torchfx_amd.typing import MusicalTime
    with pytest.raises(ValueError, match="Invalid musical time string"):
        MusicalTime.from_string(bad)


def test_musical_time_bad_modifier_and_bpm():
    from torchfx_amd.typing import MusicalTime
    with pytest.raises(ValueError, match="Invalid time duration modifier"):
        MusicalTime(1, 4, "x").fraction()
    with pytest.raises(AssertionError, match="BPM must be positive"):
        MusicalTime(1, 4).duration_seconds(0)


@pytest.mark.parametrize("kw,msg", [
    (dict(delay_samples=0), "Delay samples must be positive."),
    (dict(delay_samples=-5), "Delay samples must be positive."),
    (dict(), "BPM must be provided if delay_samples is not set."),
    (dict(bpm=0), "BPM must be positive."),
    (dict(bpm=120, fs=0), r"Sample rate \(fs\) must be positive."),
    (dict(delay_samples=10, feedback=0.96), "Feedback must be between 0 and 0.95."),
    (dict(delay_samples=10, feedback=-0.1), "Feedback must be between 0 and 0.95."),
    (dict(delay_samples=10, mix=1.5), "Mix must be between 0 and 1."),
    (dict(delay_samples=10, mix=-0.5), "Mix must be between 0 and 1."),
    (dict(delay_samples=10, taps=0), "Taps must be at least 1."),
])
def test_delay_validation(kw, msg):
    from torchfx_amd import Delay
    with pytest.raises(AssertionError, match=msg):
        Delay(**kw)


def test_delay_invalid_time_string():
    from torchfx_amd import Delay
    with pytest.raises(ValueError, match="Invalid musical time string"):
        Delay(bpm=120, delay_time="invalid", fs=44100)


def test_delay_lazy_fs():
    from torchfx_amd import Delay, Wave
    d = Delay(bpm=120, delay_time="1/8")
    assert d.delay_samples is None and d.fs is None
    w = Wave(torch.randn(2, 44100), 44100) | d
    assert d.fs == 44100
    y = w.ys
    assert d.delay_samples == 11025 and y.shape == (2, 44100 + 3 * 11025)
    with pytest.raises(AssertionError, match=r"Sample rate \(fs\) is required"):
        Delay(bpm=120, delay_time="1/8")(torch.randn(2, 100))
    assert Delay(bpm=120, delay_time="1/8", fs=48000).delay_samples == 12000


def _golden_cases():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "delay_fx.npz"))
    return g, sorted({k.split("/")[0] for k in g.files})


def golden_delay(g, name):
    """(input, expected output, Delay built the way the case was)."""
    from torchfx_amd import Delay
    from torchfx_amd.effect import PingPongDelayStrategy
    p = g[f"{name}/params"]
    D, taps, fb, mix, pp, fs, bpm = float(p[0]), int(p[1]), float(p[2]), float(p[3]), bool(p[4]), int(p[5]), float(p[6])
    strat = PingPongDelayStrategy() if pp else None
    if bpm > 0:
        d = Delay(bpm=bpm, delay_time=str(g[f"{name}/delay_time"]), fs=fs, taps=taps, feedback=fb, mix=mix, strategy=strat)
        assert d.delay_samples == int(D)
    else:
        d = Delay(delay_samples=int(D), taps=taps, feedback=fb, mix=mix, strategy=strat)
    return g[f"{name}/x"], g[f"{name}/y"], d


def test_cpu_composition_equals_reference():
    g, names = _golden_cases()
    assert len(names) >= 13
    for name in names:
        x, y, d = golden_delay(g, name)
        got = d(torch.from_numpy(x)).numpy()
        assert got.dtype == y.dtype and got.shape == y.shape, name
        assert np.array_equal(got, y), name


def test_delay_custom_strategy_runs_on_cpu():
    from torchfx_amd import Delay
    from torchfx_amd.effect import DelayStrategy

    class Silent(DelayStrategy):
        def apply_delay(self, waveform, delay_samples, taps, feedback):
            return torch.zeros(*waveform.shape[:-1], waveform.size(-1) + delay_samples * taps, dtype=waveform.dtype)

    x = torch.randn(2, 50)
    y = Delay(delay_samples=5, taps=2, mix=0.25, strategy=Silent())(x)
    assert y.shape == (2, 60)
    assert torch.equal(y[:, :50], torch.lerp(x, torch.zeros_like(x), 0.25)) and not y[:, 50:].any()


def test_meta_shapes():
    from torchfx_amd import native
    native.ops()
    op = torch.ops.torchfx_hip
    x = torch.empty(3, 2, 100, device="meta")
    assert op.delay_forward(x, 10, [1.0, 0.5], 0.2, True).shape == (3, 2, 120)
    assert op.delay_forward(torch.empty(7, device="meta"), 0, [1.0, 0.3, 0.09], 0.5, False).shape == (7,)
    y, st = op.delay_forward_ep(torch.empty(4, 1000, device="meta", dtype=torch.float64), 300, [1.0] * 3, 0.5, False,
                                1.0, False, 1, True)
    assert y.shape == (4, 1900) and y.dtype == torch.float64 and st.shape == (4,) and st.dtype == torch.float64
    with pytest.raises(RuntimeError, match="ROCm device"):
        op.delay_forward(torch.zeros(2, 10), 1, [1.0], 0.5, False)


def test_capi_rejects_bad_arguments_without_device():
    from torchfx_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    amps = ctypes.cast((ctypes.c_double * 4)(1.0, 0.5, 0.25, 0.125), ctypes.c_void_p)

    class Ep(ctypes.Structure):
        _fields_ = [("gain", ctypes.c_double), ("clamp", ctypes.c_int), ("stat_mode", ctypes.c_int),
                    ("stat_per_row", ctypes.c_int), ("stat_out", ctypes.c_void_p)]
    ep_bad = Ep(1.0, 0, 0, 0, None)
    # x, y, dtype, rows, T, delay, taps, amps, mix, pingpong, epilogue
    cases = {
        "null x": (None, p, 0, 2, 4, 1, 2, amps, 0.5, 0, None),
        "null y": (p, None, 0, 2, 4, 1, 2, amps, 0.5, 0, None),
        "null amps": (p, p, 0, 2, 4, 1, 2, None, 0.5, 0, None),
        "taps < 1": (p, p, 0, 2, 4, 1, 0, amps, 0.5, 0, None),
        "negative delay": (p, p, 0, 2, 4, -1, 2, amps, 0.5, 0, None),
        "odd rows ping-pong": (p, p, 0, 3, 4, 1, 2, amps, 0.5, 1, None),
        "bad dtype": (p, p, 7, 2, 4, 1, 2, amps, 0.5, 0, None),
        "negative rows": (p, p, 0, -2, 4, 1, 2, amps, 0.5, 0, None),
        "NaN mix": (p, p, 0, 2, 4, 1, 2, amps, float("nan"), 0, None),
        "stat without buffer": (p, p, 0, 2, 4, 1, 2, amps, 0.5, 0, ctypes.cast(ctypes.pointer(ep_bad), ctypes.c_void_p)),
        "overflowing length": (p, p, 0, 2, 4, 1 << 62, 4, amps, 0.5, 0, None),
    }
    for what, a in cases.items():
        rc = lib.tfx_delay_forward(*a, None)
        assert rc != 0, what
        assert b"delay_forward" in lib.tfx_last_error(), what
    r = ctypes.c_int(-1)
    assert lib.tfx_delay_plan_info(12000, 8, 0, 0, ctypes.byref(r)) == 0 and r.value == 1
    assert lib.tfx_delay_plan_info(37, 4, 0, 1, ctypes.byref(r)) == 0 and r.value == 0
    assert lib.tfx_delay_plan_info(0, 3, 1, 0, ctypes.byref(r)) == 0 and r.value == 0
    assert lib.tfx_delay_plan_info(3, 5000, 1, 1, ctypes.byref(r)) == 0 and r.value == 2
    assert lib.tfx_delay_plan_info(10, 0, 0, 0, ctypes.byref(r)) != 0


def test_delay_amplitudes_are_pythons_powers():
    from torchfx_amd import torchfx_ext
    a = torchfx_ext.delay_amplitudes(70, 0.95)
    assert a[0] == 1.0 and all(a[i] == 0.95 ** i for i in range(1, 70))
    assert torchfx_ext.delay_amplitudes(3, 0) == [1.0, 0.0, 0.0]


def test_planner_wraps_stock_delay_in_epilogue():
    from torchfx_amd import Delay, Gain, Normalize, Wave
    from torchfx_amd.effect import DelayStrategy, Epilogued, MonoDelayStrategy, PingPongDelayStrategy

    def plan(*mods, dtype=torch.float32):
        w = Wave(torch.zeros(2, 1000, dtype=dtype), 48000)
        w.fuse_epilogue = True
        for m in mods:
            w = w | m
        return w.plan()

    for strat in (None, PingPongDelayStrategy()):
        p = plan(Delay(delay_samples=100, strategy=strat), Gain(0.5), Normalize(0.9))
        assert [type(m).__name__ for m in p] == ["Epilogued"] and type(p[0].producer).__name__ == "Delay"
    p = plan(Delay(delay_samples=100), Gain(0.5), Normalize(0.9), dtype=torch.float16)
    assert [type(m).__name__ for m in p] == ["Delay", "Gain", "Normalize"]

    class Custom(DelayStrategy):
        def apply_delay(self, waveform, delay_samples, taps, feedback):
            return MonoDelayStrategy().apply_delay(waveform, delay_samples, taps, feedback)
    p = plan(Delay(delay_samples=100, strategy=Custom()), Gain(0.5), Normalize(0.9))
    assert [type(m).__name__ for m in p] == ["Delay", "Gain", "Normalize"]
    assert not any(isinstance(m, Epilogued) for m in p)


def test_planner_keys_and_barrier():
    from torchfx_amd import Delay, Wave
    from torchfx_amd import filter as F
    d = Delay(delay_samples=100, taps=3)
    w = Wave(torch.zeros(2, 5000), 48000)
    w.fuse_epilogue, w.fuse_fir, w.fuse_gain = False, True, True
    f1, f2 = F.FIR(np.hanning(31)), F.FIR(np.hanning(17))
    w2 = w | f1 | d | f2
    assert [type(m).__name__ for m in w2.plan()] == ["FIR", "Delay", "FIR"]      # nothing merges across the Delay
    first = w2.plan()
    d.taps = 4
    assert w2.plan() is not first and [type(m).__name__ for m in w2.plan()] == ["FIR", "Delay", "FIR"]
    from torchfx_amd.wave import _member_key
    for attr, val in (("delay_samples", 101), ("taps", 5), ("feedback", 0.5), ("mix", 0.7), ("fs", 44100)):
        dd = Delay(delay_samples=100, taps=3)
        k0 = _member_key(dd, [])
        setattr(dd, attr, val)
        assert _member_key(dd, []) != k0, attr
    dd = Delay(delay_samples=100)
    k0 = _member_key(dd, [])
    from torchfx_amd.effect import PingPongDelayStrategy
    dd.strategy = PingPongDelayStrategy()
    assert _member_key(dd, []) != k0
    lines = (Wave(torch.zeros(2, 100), 48000) | Delay(delay_samples=10)).explain()
    assert lines == ["Delay: torch composition -- cpu tensor"]
