"""Feedback (regeneration) of the modulated delay line without a device: the NumPy host path against the per-sample loop of
tests/modulation_feedback_reference.py within its derived bound -- every case of its tables, so that host and device are held
to one reference --, the plan each case was built for (packing, packing cut by LDS, the rpw == 1 fallback, the lane seams 32 / 33,
64, 128 / 129, eight voices), every argument rule feedback adds, the plan query, the routes."""
import math

import numpy as np
import pytest
import torch

import torchfx_amd as f
from tests import modulation_feedback_reference as F


@pytest.mark.parametrize("name", list(F.TABLES))
@pytest.mark.parametrize("interpolation,lfo,dtype", [("linear", "sine", torch.float32), ("cubic", "triangle", torch.float64),
                                                      ("cubic", "sine", torch.float32), ("linear", "triangle", torch.float64)])
def test_host_path_against_the_definition(interpolation, lfo, dtype, name):
    F.assert_plan(name, interpolation)
    x = torch.from_numpy(np.array(F.case(name, interpolation, lfo)[0])).to(dtype)
    kw = dict(dry=F.DRY, spread=F.SPREAD, shape=lfo, interpolation=interpolation, position=F.POSITION, feedback=F.TABLES[name][1])
    B = F.TABLES[name][2]
    for n in (F.T, 0, 1, B - 1, B, B + 1):                             # the reference is causal: a prefix is the shorter call
        y = f.modulated_delay(x[..., :n].contiguous(), F.FS, F.voices(name, interpolation), **kw)
        F.check(y.numpy(), name, interpolation, lfo, f"host {name} {interpolation} {lfo} T = {n}", length=n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_host_path_on_the_longest_ring(dtype):
    """B1long: block 1 with a ring of 8192 samples that wraps -- rows_per_wave falls back to 1 and the launch takes 64 KiB."""
    interpolation, lfo = F.LONG_PAIR
    assert F.assert_plan("B1long", interpolation)["steps"] == F.shape_of("B1long")[1]
    x = torch.from_numpy(np.array(F.case("B1long", interpolation, lfo)[0])).to(dtype)
    y = f.modulated_delay(x, F.FS, F.voices("B1long", interpolation), dry=F.DRY, spread=F.SPREAD, shape=lfo, interpolation=interpolation,
                          position=F.POSITION, feedback=F.table("B1long")[1])
    F.check(y.numpy(), "B1long", interpolation, lfo, f"host B1long {interpolation} {lfo} {dtype}")


@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
def test_the_plans_the_cases_were_built_for(interpolation):
    """Every row of the case table reports the geometry it was chosen to reach, and the geometry follows the batch."""
    for name in list(F.TABLES) + list(F.LONG_TABLES):
        q = F.assert_plan(name, interpolation)
        batch, n = F.shape_of(name)
        assert q["steps"] == -(-n // q["block"]) and q["workgroups"] == 2 * -(-batch // q["rows_per_wave"])
        assert q["lds_bytes"] <= 65536 and q["ring"] & (q["ring"] - 1) == 0
    # the stride between a wave's rings: ring + B when packed, the ring alone when the wave holds one row
    assert F.plan("B16", interpolation)["lds_bytes"] == 4 * (64 + 16) * 8
    assert F.plan("B5long", interpolation)["lds_bytes"] == 7 * (1024 + 5) * 8
    assert F.plan("B1long", interpolation)["lds_bytes"] == 8192 * 8               # not (8192 + 1) * 8: that would not fit
    assert F.plan("B33", interpolation)["lds_bytes"] == F.plan("B33", interpolation)["ring"] * 8
    # waves: B16 4 + 1, B32 2 + 2 + 1, B5long 7 + 2; a batch of rows_per_wave + 1 opens the second wave
    for name, rpw in (("B16", 4), ("B32", 2), ("B5long", 7), ("V8", 8)):
        assert F.plan(name, interpolation, batch=rpw)["workgroups"] == 2 and F.plan(name, interpolation, batch=rpw + 1)["workgroups"] == 4


def test_feedback_zero_is_the_call_without_it_and_the_effects_carry_the_loop_gain():
    x = torch.from_numpy(np.array(F.case("B5", "linear", "sine")[0]))
    v = F.voices("B5", "linear")
    assert torch.equal(f.modulated_delay(x, F.FS, v, feedback=0.0), f.modulated_delay(x, F.FS, v))
    assert torch.equal(f.Flanger(fs=48000, feedback=0.0)(x), f.Flanger(fs=48000)(x))
    long = torch.cat([x, x, x], -1)                                    # the chorus' first echo comes back after 2 * 816 samples
    for eff, plain, raw, loop in ((f.Flanger(fs=48000, feedback=0.7), f.Flanger(fs=48000), 1.4, 0.7),
                                  (f.Chorus(fs=48000, feedback=0.4), f.Chorus(fs=48000), 0.8, 0.4),
                                  (f.Flanger(fs=48000, feedback=0.7, invert=True, mix=0.25), f.Flanger(fs=48000, invert=True, mix=0.25), -2.8, 0.7)):
        P = eff.params(torch.float32)
        assert P.feedback == pytest.approx(raw) and P.feedback * P.table[:, 4].sum() == pytest.approx(loop)
        assert not torch.equal(eff(long), plain(long))
    assert f.Flanger(fs=48000, feedback=0.7).params(torch.float32).block == 47
    assert (f.Wave(x[0], 48000) | f.Flanger(feedback=0.7)).explain()[-1] == "Flanger: numpy on host -- cpu tensor"


def test_argument_errors_name_their_argument_and_the_plan_answers_without_a_device():
    from torchfx_amd import realtime as RT

    x = torch.zeros(2, 64)
    bad = [
        (dict(feedback=2.0), "feedback: the loop is not stable"),                                  # 2 * 0.5 = 1
        (dict(feedback=1.7, interpolation="cubic"), "feedback: the loop is not stable"),           # 1.7 * 0.5 * 1.25 > 1
        (dict(feedback=math.nan), "feedback must be a finite number"),
        (dict(feedback=math.inf), "feedback must be a finite number"),
        (dict(feedback=0.5, voices=[(2.5, 2.0, 100.0, 0.0, 0.5)]), "delay - depth\\) must be >= 1"),
        (dict(feedback=0.5, voices=[(3.5, 2.0, 100.0, 0.0, 0.5)], interpolation="cubic"), "delay - depth\\) must be >= 2"),
        (dict(feedback=0.5, voices=[(8000.0, 200.0, 100.0, 0.0, 0.5)]), "delay \\+ depth\\) \\+ 2 \\+ min\\(block, 64\\) = 8266"),
    ]
    for kw, match in bad:
        a = dict(dict(voices=[(10.0, 2.0, 100.0, 0.0, 0.5)]), **kw)
        with pytest.raises(ValueError, match=match):
            f.modulated_delay(x, F.FS, a.pop("voices"), **a)
    f.modulated_delay(x, F.FS, [(8000.0, 126.0, 100.0, 0.0, 0.5)], feedback=0.5)                   # 8126 + 2 + 64 = 8192 fits
    with pytest.raises(ValueError, match="mix must not be 0 with feedback"):
        f.Flanger(mix=0.0, feedback=0.5)
    with pytest.raises(ValueError, match="feedback: the loop is not stable"):
        f.Chorus(feedback=0.8)                                                                     # 0.8 * 1.25 = 1
    f.Chorus(feedback=0.8, interpolation="linear")
    with pytest.raises(TypeError, match="feedback"):
        f.Vibrato(feedback=0.5)
    for stateful in (RT.StatefulChorus, RT.StatefulFlanger):
        with pytest.raises(ValueError, match="feedback must be 0.*stream of the recursive line is not provided"):
            stateful(feedback=0.3)
        eff = stateful(fs=48000)
        eff.feedback = 0.3
        with pytest.raises(ValueError, match="feedback must be 0"):
            eff(x)
    from torchfx_amd import torchfx_ext as E

    table = [(b, d, r / F.FS, p, g) for b, d, r, p, g in F.voices("B5", "linear")]
    q = E.modulated_delay_feedback_plan_info(F.T, table, 0.8, batch=5, channels=2)
    assert q == dict(block=5, rows_per_wave=12, ring=32, lds_bytes=12 * (32 + 5) * 8, workgroups=2, steps=300)
    with pytest.raises(RuntimeError, match="feedback must not be 0"):
        E.modulated_delay_feedback_plan_info(100, table, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.modulated_delay_forward(torch.zeros(2, 8), table, feedback=0.5)
