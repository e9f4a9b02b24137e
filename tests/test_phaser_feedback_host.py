"""Phaser feedback (resonance) without a device: the argument rule, the C entries, the plan query, feedback = 0, the NumPy host
path against the per-sample loop of tests/phaser_feedback_reference.py within 16 E_REF and its end state within 16 E_REF_S -- at
1, 4 and 12 stages, at the lane-bucket edges 2, 3, 6 and 7 and with the triangle LFO --, and StatefulPhaser's chunks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import torchfx_amd as f
from tests import phaser_feedback_reference as F

FS = 48000
KW = dict(rate=30.0, phase=0.1, dry=0.6, wet=0.5, spread=0.25)


def signal(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32))


@pytest.mark.parametrize("bad", [1.0, -1.0, math.nan, math.inf])
def test_argument_errors_name_feedback(bad):
    for make in (lambda: f.phase_shift(torch.zeros(2, 64), FS, feedback=bad), lambda: f.Phaser(feedback=bad)):
        with pytest.raises(ValueError, match="feedback must be finite with \\|feedback\\| < 1"):
            make()


def test_c_entries_refuse_bad_arguments_and_the_plan_answers_without_a_device():
    from torchfx_amd import _lib
    from torchfx_amd import torchfx_ext as E

    lib = _lib.load()
    buf, out = [(ctypes.c_float * 256)() for _ in range(2)]
    vp = lambda b: None if b is None else ctypes.cast(b, ctypes.c_void_p)      # noqa: E731
    ok = dict(x=buf, y=out, rows=2, T=32, stages=4, fb=0.5, segments=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tfx_phaser_feedback_forward(vp(a["x"]), vp(a["y"]), None, 0, a["rows"], 2, a["T"], a["stages"], 48000.0, 0.5, 200.0, 2000.0,
                                               0.0, 0.0, 0.5, 0.5, a["fb"], 0, 0, None, None, None, None, a["segments"], None, None)
    for kw in (dict(x=None), dict(y=None), dict(y=buf), dict(rows=-1), dict(rows=3), dict(T=-1), dict(stages=13), dict(fb=1.0),
               dict(fb=math.nan), dict(segments=-1), dict(T=3 * 2048, segments=2)):
        assert call(**kw) != 0 and b"phaser_feedback_forward" in lib.tfx_last_error(), kw
    assert call(rows=0) == 0
    refs = [ctypes.byref(ctypes.c_int64()) for _ in range(7)]
    assert lib.tfx_phaser_feedback_plan_info(2, 2, 5000, 4, 0, 0.5, None, *refs[1:]) != 0 and b"null output" in lib.tfx_last_error()
    assert E.phaser_feedback_plan_info(5000, 0.7, rows=2, channels=2, stages=4) == dict(
        run=64, tile=2048, segments=3, launches=2, lds_bytes=60000, workgroups=6, scratch_bytes=2 * 3 * 5 * 6 * 8)
    assert [E.phaser_feedback_plan_info(100, -0.9, stages=n)["run"] for n in (1, 2, 3, 6, 7, 12)] == [32, 32, 64, 64, 128, 128]
    assert E.phaser_feedback_plan_info(5000, 0.7, rows=256)["launches"] == 1
    for kw in (dict(feedback=1.0), dict(stages=13), dict(length=-1)):
        with pytest.raises(RuntimeError, match="phaser_feedback_plan_info"):
            E.phaser_feedback_plan_info(**dict(dict(length=100, feedback=0.5), **kw))
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.phaser_forward(torch.zeros(2, 8), 4, FS, 3.0, 200.0, 2000.0, feedback=0.5)
    assert (f.Wave(torch.zeros(2, 64), FS) | f.Phaser(feedback=0.7)).explain()[-1] == "Phaser: numpy on host -- cpu tensor"


def test_feedback_zero_is_the_call_without_it():
    x = signal((2, 700), 1)
    assert torch.equal(f.phase_shift(x, FS, feedback=0.0, **KW), f.phase_shift(x, FS, **KW))
    assert torch.equal(f.Phaser(fs=FS, feedback=0.0)(x), f.Phaser(fs=FS)(x))


def host_against_the_definition(stages, feedback, dtype, shape="sine"):
    x = signal((2, 2, 1117), 10 + stages)                               # 1117: whole runs of 32, 64 and 128 and a shorter last one
    state = np.random.default_rng(3).uniform(-1.0, 1.0, (4, stages + 1))
    y, coef, st = f.phase_shift(x.to(dtype), FS, stages, feedback=feedback, state=torch.from_numpy(state), return_coef=True,
                                return_state=True, shape=shape, **KW)
    F.check_coef(coef.numpy(), FS, 200.0, 2000.0, KW["rate"], KW["phase"], KW["spread"], shape)
    ref = F.reference(x.numpy().reshape(4, -1), coef.numpy(), stages, KW["dry"], KW["wet"], feedback, 2, state)
    yld, e_ref = ref.y, ref.e_ref
    F.check(y.numpy().reshape(yld.shape), yld, e_ref, f"host N={stages} fb={feedback} {shape}")
    assert st.shape == (4, stages + 1) and np.allclose(st.numpy(), ref.state.astype(np.float64), rtol=0, atol=1e-6)
    F.check_state(st.numpy(), ref.state, ref.e_ref_s, f"host N={stages} fb={feedback} {shape}", "host")   # the state's own bound
    plain = f.phase_shift(x.to(dtype), FS, stages, state=torch.from_numpy(state), shape=shape, **KW)
    gap = np.abs(plain.numpy().astype(np.float64) - yld.reshape(x.shape).astype(np.float64)).max(-1)
    assert (gap > 100.0 * (16.0 * e_ref + 2.0 ** -24 * np.abs(yld).max())).all(), "feedback is not at work"


@pytest.mark.parametrize("stages,feedback,dtype", [(1, 0.7, torch.float32), (4, -0.9, torch.float64), (12, 0.7, torch.float64)])
def test_host_path_against_the_definition(stages, feedback, dtype):
    host_against_the_definition(stages, feedback, dtype)


@pytest.mark.parametrize("stages,feedback,dtype,shape", [
    (2, 0.7, torch.float64, "sine"), (3, -0.9, torch.float32, "sine"), (6, 0.7, torch.float64, "sine"), (7, -0.9, torch.float64, "sine"),
    (7, 0.7, torch.float64, "triangle")])
def test_host_path_at_the_bucket_edges_and_with_the_triangle(stages, feedback, dtype, shape):
    """N + 2 = 4 and 8 fill a chunk's lanes, 3 and 7 open the next bucket; the NumPy path has the same run and chunk structure."""
    host_against_the_definition(stages, feedback, dtype, shape)


def test_stateful_phaser_chunks_equal_the_one_shot_call():
    from torchfx_amd.realtime import StatefulPhaser

    x = signal((2, 4000), 20)
    eff = StatefulPhaser(rate=30.0, stages=4, spread=0.25, fs=FS, feedback=0.7, mix=0.5)
    cuts = np.cumsum([0, 300, 1, 2049, 7, 1643])
    y = torch.cat([eff(x[:, a:b].contiguous()) for a, b in zip(cuts[:-1], cuts[1:])], -1)
    _, coef = f.phase_shift(x, FS, rate=30.0, spread=0.25, feedback=0.7, return_coef=True)
    yld, _, e_ref, *_ = F.reference(x.numpy(), coef.numpy(), 4, 0.5, 0.5, 0.7, 2)
    F.check(y.numpy(), yld, e_ref, "StatefulPhaser(feedback=0.7) chunks")
    F.check(f.Phaser(rate=30.0, stages=4, spread=0.25, fs=FS, feedback=0.7)(x).numpy(), yld, e_ref, "Phaser(feedback=0.7)")
