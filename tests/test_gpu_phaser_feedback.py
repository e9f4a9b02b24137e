"""Phaser feedback on the device (csrc/phaser.hip, phaser_feedback_kernel) against the per-sample loop of
tests/phaser_feedback_reference.py fed the kernel's own coefficient bits: within 16 E_REF of the long-double loop (+ 2^-24 |ref|
for float32), E_REF the case's own |loop64 - loop_ld|; and the exact properties with torch.equal.  Rows (2, 2), T = 3 tile + 17,
LFO 30 Hz with spread 0.25, so the sweep moves inside the signal and the rows differ."""
import functools

import numpy as np
import pytest
import torch

from tests import phaser_feedback_reference as F
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 48000
DTYPES = {"f32": torch.float32, "f64": torch.float64}
SWEEP = (FS, 30.0, 200.0, 2000.0, 0.1, 0.25, 0.6, 0.5, "sine")      # fs, rate, min, max, phase, spread, dry, wet, shape


@functools.lru_cache(maxsize=None)
def length():
    return 3 * ext().phaser_feedback_plan_info(1, 0.5)["tile"] + 17


@functools.lru_cache(maxsize=None)
def signal():
    x = np.random.default_rng(7).uniform(-1.0, 1.0, (2, 2, length())).astype(np.float32)
    x.setflags(write=False)
    return x


def run(x, N, fb, dt="f64", segments=1, state=None, position=0):
    """The op on x (array) -> (y, coef, new state) as device tensors."""
    t = torch.from_numpy(np.array(x)).to(DEV, DTYPES[dt])
    y, coef, st, _ = ext().phaser_forward(t, N, *SWEEP, position, None, state, True, segments, fb)
    return y, coef, st


@functools.lru_cache(maxsize=None)
def reference(N, fb):
    """(long-double result [2, 2, T], E_REF, the coefficient track it was computed from), once per case."""
    coef = run(signal(), N, fb)[1].cpu().numpy()
    F.check_coef(coef, FS, SWEEP[2], SWEEP[3], SWEEP[1], SWEEP[4], SWEEP[5], what=f"N={N}")
    yld, _, e_ref = F.reference(signal().reshape(4, -1), coef, N, SWEEP[6], SWEEP[7], fb, 2)
    return yld.reshape(signal().shape), e_ref, coef


def test_route_and_explain_name_the_plan():
    import torchfx_amd as f

    w = f.Wave(torch.from_numpy(np.array(signal()[0])).to(DEV), FS, device=DEV) | f.Phaser(rate=30.0, stages=12, feedback=0.7)
    assert w.explain() == ["Phaser: native (phaser_feedback_kernel, 12 stage(s), sine LFO, feedback 0.7: runs of 128 in tiles of 2048, "
                           "4 segment(s), 8 workgroup(s), 60000 B of LDS; two launches)"]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("fb", [0.7, -0.9])
@pytest.mark.parametrize("N", [1, 4, 12])
@pytest.mark.parametrize("segments", [1, 3])
def test_accuracy_feedback_at_work_and_the_route(segments, N, fb, dt):
    yld, e_ref, coef0 = reference(N, fb)
    y, coef, st = run(signal(), N, fb, dt, segments)
    F.check(y.cpu().numpy(), yld, e_ref, f"N={N} fb={fb} {dt} segments={segments}")
    plain, track, _ = run(signal(), N, 0.0, dt, segments)
    assert torch.equal(coef, track) and np.array_equal(coef.cpu().numpy(), coef0)
    gap = (y.double() - plain.double()).abs().amax(-1)
    assert bool((gap > 100.0 * (16.0 * e_ref + 2.0 ** -24 * float(np.abs(yld).max()))).all()), "feedback is not at work"
    t = torch.from_numpy(np.array(signal())).to(DEV, DTYPES[dt])
    old = ext().phaser_forward(t, N, *SWEEP, 0, None, None, True, segments)
    assert torch.equal(plain, old[0]) and torch.equal(track, old[1])


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N", [1, 4, 12])
def test_independence_causality_and_the_state_hand_off(N, dt):
    fb, x = 0.7, signal()
    yld, e_ref, _ = reference(N, fb)
    whole = {s: run(x, N, fb, dt, s)[0] for s in (1, 3)}
    for s in (1, 3):                                                    # both cuts within the bound of the one reference
        F.check(whole[s].cpu().numpy(), yld, e_ref, f"N={N} {dt}: segments={s}")
    tile = (length() - 17) // 3
    for s, m in ((1, 2 * tile + 5), (3, tile - 3)):                    # 3 segments: a prefix inside the first segment of both cuts
        assert torch.equal(whole[s][..., :m], run(x[..., :m], N, fb, dt, s)[0])
        # a row alone (item 1's channel 0 as a [1, T] signal of channel index 0) has the bits it has in the batch
        assert torch.equal(run(x[1, :1], N, fb, dt, s)[0][0], whole[s][1, 0])
    ya, _, sa = run(x[..., :700], N, fb, dt)
    yb, _, _ = run(x[..., 700:], N, fb, dt, state=sa, position=700)
    F.check(torch.cat([ya, yb], -1).cpu().numpy(), yld, e_ref, f"N={N} {dt}: split at 700")


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("N", [1, 4, 12])
def test_a_planted_nan_travels_forward_only(N, segments):
    m = 1000                                                            # mid-tile, mid-run for every run length
    planted = np.array(signal()).reshape(4, -1)
    planted[1, m] = np.nan
    for dt in DTYPES:
        clean, _, _ = run(signal().reshape(4, -1), N, 0.7, dt, segments)
        y, _, st = run(planted, N, 0.7, dt, segments)
        assert torch.equal(y[1, :m], clean[1, :m]) and torch.equal(y[[0, 2, 3]], clean[[0, 2, 3]])
        assert not torch.isfinite(y[1, m:]).any() and not torch.isfinite(st[1]).any() and torch.isfinite(st[[0, 2, 3]]).all()
