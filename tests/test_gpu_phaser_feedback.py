"""Phaser feedback on the device (csrc/phaser.hip, phaser_feedback_kernel) against the per-sample loop of
tests/phaser_feedback_reference.py fed the kernel's own coefficient bits: within 16 E_REF of the long-double loop (+ 2^-24 |ref|
for float32), E_REF the case's own |loop64 - loop_ld|; the end state within 16 E_REF_S of the long-double state; and the exact
properties with torch.equal.  Rows (2, 2), T = 3 tile + 17, LFO 30 Hz with spread 0.25, so the sweep moves inside the signal and
the rows differ.  Every case asserts the run length of its stage count first (phaser_feedback_plan_info): the stage counts sit at
the lane-bucket edges (N + 2 = 4 and 8 fill a chunk's lanes, N = 3 and 7 open the next bucket), both LFO shapes run both passes,
the lengths sit below, at and over a run and a tile, the end state is compared with the reference and handed on at those seams
through one and through three segments, with the host position and with the device position of a stream."""
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
RUNS = {1: 32, 2: 32, 3: 64, 4: 64, 6: 64, 7: 128, 12: 128}         # stages -> samples one lane runs: N + 2 <= 4, 8, 16 lanes
TILE = 2048


def sweep(shape="sine", spread=0.25):
    return SWEEP[:5] + (spread,) + SWEEP[6:8] + (shape,)


@functools.lru_cache(maxsize=None)
def length():
    return 3 * ext().phaser_feedback_plan_info(1, 0.5)["tile"] + 17


@functools.lru_cache(maxsize=None)
def signal():
    x = np.random.default_rng(7).uniform(-1.0, 1.0, (2, 2, length())).astype(np.float32)
    x.setflags(write=False)
    return x


def run_length(N, fb=0.7):
    """The plan's run for N stages, asserted against the bucket the case was chosen for."""
    info = ext().phaser_feedback_plan_info(length(), fb, rows=4, channels=2, stages=N)
    assert info["run"] == RUNS[N] and info["tile"] == TILE, f"N={N}: the plan says {info}"
    return info["run"]


def run(x, N, fb, dt="f64", segments=1, state=None, position=0, sw=SWEEP, pos=None):
    """The op on x (array) -> (y, coef, new state) as device tensors."""
    t = torch.from_numpy(np.array(x)).to(DEV, DTYPES[dt])
    y, coef, st, _ = ext().phaser_forward(t, N, *sw, position, pos, state, True, segments, fb)
    return y, coef, st


@functools.lru_cache(maxsize=None)
def full(N, fb, shape="sine"):
    """(the reference.Ref of the whole signal as 4 rows, the coefficient track it was computed from), once per case."""
    coef = run(signal(), N, fb, sw=sweep(shape))[1].cpu().numpy()
    F.check_coef(coef, FS, SWEEP[2], SWEEP[3], SWEEP[1], SWEEP[4], SWEEP[5], shape, what=f"N={N} {shape}")
    return F.reference(signal().reshape(4, -1), coef, N, SWEEP[6], SWEEP[7], fb, 2), coef


def reference(N, fb, shape="sine"):
    """(long-double result [2, 2, T], E_REF, the coefficient track)."""
    ref, coef = full(N, fb, shape)
    return ref.y.reshape(signal().shape), ref.e_ref, coef


def test_route_and_explain_name_the_plan():
    import torchfx_amd as f

    w = f.Wave(torch.from_numpy(np.array(signal()[0])).to(DEV), FS, device=DEV) | f.Phaser(rate=30.0, stages=12, feedback=0.7)
    assert w.explain() == ["Phaser: native (phaser_feedback_kernel, 12 stage(s), sine LFO, feedback 0.7: runs of 128 in tiles of 2048, "
                           "4 segment(s), 8 workgroup(s), 60000 B of LDS; two launches)"]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("fb", [0.7, -0.9])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 6, 7, 12])
@pytest.mark.parametrize("segments", [1, 3])
def test_accuracy_feedback_at_work_and_the_route(segments, N, fb, dt):
    """The stage counts at the lane-bucket edges: runs of 32, 32, 64, 64, 64, 128, 128."""
    run_length(N, fb)
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
@pytest.mark.parametrize("N", [2, 7])
@pytest.mark.parametrize("segments", [1, 3])
def test_the_triangle_lfo_in_both_passes(segments, N, dt):
    """The TRI instantiations of pass C (one segment) and of passes A and C (three); the track by the reference's triangle rule."""
    run_length(N)
    yld, e_ref, coef0 = reference(N, 0.7, "triangle")
    y, coef, st = run(signal(), N, 0.7, dt, segments, sw=sweep("triangle"))
    assert np.array_equal(coef.cpu().numpy(), coef0) and not np.array_equal(coef0, reference(N, 0.7)[2])
    F.check(y.cpu().numpy(), yld, e_ref, f"triangle N={N} {dt} segments={segments}")
    F.check_state(st.cpu().numpy(), full(N, 0.7, "triangle")[0].state, full(N, 0.7, "triangle")[0].e_ref_s,
                  f"triangle N={N} {dt} segments={segments}", f"device {dt}")


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


def lengths(N):
    L = RUNS[N]
    return [1, L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, 2 * TILE]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N", [2, 6, 12])
def test_lengths_around_a_run_and_a_tile_and_the_end_state(N, dt):
    """T below a run, a run, one over, a tile less one, a tile, one over, two tiles (an exact multiple: the last tile is full and
    the end state is still taken at T - 1).  The loop is causal, so the prefix of the one reference is the shorter call's, and the
    end state is the long-double state after sample T - 1, within 16 E_REF_S."""
    run_length(N)
    ref, _ = full(N, 0.7)
    for n in lengths(N):
        tiles = -(-n // TILE)
        for segments in (1, 2) if tiles >= 2 else (1,):
            assert ext().phaser_feedback_plan_info(n, 0.7, rows=4, channels=2, stages=N, segments=segments)["segments"] == segments
            y, _, st = run(signal()[..., :n], N, 0.7, dt, segments)
            what = f"N={N} {dt} T={n} segments={segments}"
            F.check(y.cpu().numpy().reshape(4, n), ref.y[:, :n], ref.e_ref, what)
            F.check_state(st.cpu().numpy(), ref.states[:, n - 1], ref.e_ref_s, what, f"device {dt}")


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("N", [2, 6, 12])
def test_the_state_hand_off_at_the_seams(N, segments):
    """Chunk A up to the cut, chunk B from A's state at position = cut, through one segment and through three, where a non-zero
    state_in travels through pass C's summary chain and its (seg & 1) copy."""
    L, n = run_length(N), length()
    ref, _ = full(N, 0.7)
    x = signal()
    for cut in (1, L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, n - 1):
        ya, _, sa = run(x[..., :cut], N, 0.7)
        want = min(segments, -(-(n - cut) // TILE))                    # the plan clamps the request to the tiles of the rest
        assert ext().phaser_feedback_plan_info(n - cut, 0.7, rows=4, channels=2, stages=N, segments=segments)["segments"] == want
        yb, _, sb = run(x[..., cut:], N, 0.7, segments=segments, state=sa, position=cut)
        what = f"N={N}: cut at {cut}, the rest in {segments} segment(s)"
        F.check(torch.cat([ya, yb], -1).cpu().numpy().reshape(4, n), ref.y, ref.e_ref, what)
        F.check_state(sa.cpu().numpy(), ref.states[:, cut - 1], ref.e_ref_s, what + ", state at the cut", "device f64")
        F.check_state(sb.cpu().numpy(), ref.state, ref.e_ref_s, what + ", end state", "device f64")


def test_spread_zero_shares_one_coefficient_row_and_a_single_channel():
    """spread == 0 with two channels: coef_rows == 1, the track is one row, and the channels of an item fed one signal are equal
    bit for bit.  (3, 1, T): one channel, three items."""
    N, fb = 4, 0.7
    run_length(N)
    rows = signal().reshape(4, -1)
    x = np.stack([np.stack([rows[0], rows[0]]), np.stack([rows[1], rows[1]])])         # (2, 2, T), both channels alike
    for dt in ("f64", "f32"):
        for segments in (1, 3):
            y, coef, st = run(x, N, fb, dt, segments, sw=sweep(spread=0.0))
            assert coef.shape == (1, length())
            assert torch.equal(y[:, 0], y[:, 1]) and torch.equal(st[0], st[1]) and torch.equal(st[2], st[3])
            if dt == "f64" and segments == 1:
                c0 = coef.cpu().numpy()
                F.check_coef(c0, FS, SWEEP[2], SWEEP[3], SWEEP[1], SWEEP[4], 0.0, what="spread 0")
                ref = F.reference(x.reshape(4, -1), c0, N, SWEEP[6], SWEEP[7], fb, 2)
            else:
                assert np.array_equal(coef.cpu().numpy(), c0)
            F.check(y.cpu().numpy().reshape(4, -1), ref.y, ref.e_ref, f"spread 0 {dt} segments={segments}")
            F.check_state(st.cpu().numpy(), ref.state, ref.e_ref_s, f"spread 0 {dt} segments={segments}", f"device {dt}")
    x1 = np.array(rows[:3]).reshape(3, 1, -1)
    for dt in ("f64", "f32"):
        for segments in (1, 3):
            y, coef, st = run(x1, N, fb, dt, segments)
            assert coef.shape == (1, length())
            if dt == "f64" and segments == 1:
                c1 = coef.cpu().numpy()
                ref1 = F.reference(x1.reshape(3, -1), c1, N, SWEEP[6], SWEEP[7], fb, 1)
            else:
                assert np.array_equal(coef.cpu().numpy(), c1)
            F.check(y.cpu().numpy().reshape(3, -1), ref1.y, ref1.e_ref, f"one channel {dt} segments={segments}")
            F.check_state(st.cpu().numpy(), ref1.state, ref1.e_ref_s, f"one channel {dt} segments={segments}", f"device {dt}")


def test_automatic_segments_are_the_plans_and_the_class_takes_them():
    """segments = 0, the path the Phaser class takes: the plan's own count, named by the route, bit for bit the explicit call."""
    import torchfx_amd as f

    N, fb = 12, 0.7
    info = ext().phaser_feedback_plan_info(length(), fb, rows=4, channels=2, stages=N)
    assert info["segments"] > 1 and info["launches"] == 2 and info["workgroups"] == 4 * info["segments"]
    yld, e_ref, _ = reference(N, fb)
    for dt in DTYPES:
        y0 = run(signal(), N, fb, dt, 0)[0]
        F.check(y0.cpu().numpy(), yld, e_ref, f"automatic segments {dt}")
        assert torch.equal(y0, run(signal(), N, fb, dt, info["segments"])[0])
        eff = f.Phaser(rate=30.0, stages=N, spread=0.25, feedback=fb, fs=FS)
        t = torch.from_numpy(np.array(signal())).to(DEV, DTYPES[dt])
        assert eff.route(t) == (f"native (phaser_feedback_kernel, 12 stage(s), sine LFO, feedback 0.7: runs of 128 in tiles of 2048, "
                                f"{info['segments']} segment(s), {info['workgroups']} workgroup(s), 60000 B of LDS; two launches)")
        sw = (FS, 30.0, 200.0, 2000.0, 0.0, 0.25, 0.5, 0.5, "sine")
        assert torch.equal(eff(t), run(signal(), N, fb, dt, info["segments"], sw=sw)[0])


@pytest.mark.parametrize("fb", [0.99, -0.99, 1e-3])
@pytest.mark.parametrize("segments", [1, 3])
def test_feedback_strength(segments, fb):
    """A loop close to the rule's edge on either side, and one that barely acts: the bound is E_REF's and adapts on its own."""
    N = 12
    run_length(N, fb)
    ref, _ = full(N, fb)
    y, _, st = run(signal(), N, fb, "f64", segments)
    F.check(y.cpu().numpy().reshape(4, -1), ref.y, ref.e_ref, f"N={N} fb={fb} segments={segments}")
    F.check_state(st.cpu().numpy(), ref.state, ref.e_ref_s, f"N={N} fb={fb} segments={segments}", "device f64")


@pytest.mark.parametrize("N", [2, 12])
def test_zero_in_zero_out_and_a_state_alone(N):
    """A zero signal from a zero state is zero exactly, end state included; a zero signal from a random state through three
    segments is the M columns alone, within the bound of the loop from that state."""
    run_length(N)
    zero = np.zeros((2, 2, length()), np.float32)
    for dt in ("f64", "f32"):
        for segments in (1, 3):
            y, _, st = run(zero, N, 0.7, dt, segments)
            assert torch.equal(y, torch.zeros_like(y)) and torch.equal(st, torch.zeros_like(st))
    state = np.random.default_rng(N).uniform(-1.0, 1.0, (4, N + 1))
    coef = full(N, 0.7)[1]
    ref = F.reference(zero.reshape(4, -1), coef, N, SWEEP[6], SWEEP[7], 0.7, 2, state)
    assert float(np.abs(ref.y[:, :64]).max()) > 1e-3                    # the state is heard
    for dt in DTYPES:
        y, c, st = run(zero, N, 0.7, dt, 3, state=torch.from_numpy(state).to(DEV))
        assert np.array_equal(c.cpu().numpy(), coef)
        F.check(y.cpu().numpy().reshape(4, -1), ref.y, ref.e_ref, f"N={N} {dt}: a state alone, 3 segments")
        F.check_state(st.cpu().numpy(), ref.state, ref.e_ref_s, f"N={N} {dt}: a state alone, 3 segments", f"device {dt}")


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


@pytest.mark.parametrize("m,bad", [(TILE - 1, np.nan), (TILE, np.nan), (TILE, np.inf)], ids=["last-of-tile", "first-of-tile", "inf"])
@pytest.mark.parametrize("N", [2, 12])
def test_a_non_finite_value_at_a_tile_seam_travels_forward_only(N, m, bad):
    """Three segments over four tiles: the value sits on the last sample of the first tile or on the first of the next.  Nothing before it and nothing in the other rows changes, everything from it on and its row's end state is non-finite."""
    run_length(N)
    planted = np.array(signal()).reshape(4, -1)
    planted[1, m] = bad
    for dt in DTYPES:
        clean, _, sc = run(signal().reshape(4, -1), N, 0.7, dt, 3)
        y, _, st = run(planted, N, 0.7, dt, 3)
        assert torch.equal(y[1, :m], clean[1, :m]) and torch.equal(y[[0, 2, 3]], clean[[0, 2, 3]])
        assert not torch.isfinite(y[1, m:]).any() and not torch.isfinite(st[1]).any()
        assert torch.isfinite(clean).all() and torch.equal(st[[0, 2, 3]], sc[[0, 2, 3]])


@pytest.mark.parametrize("segments", [1, 3])
@pytest.mark.parametrize("N", [2, 12])
def test_a_nan_in_one_rows_state_stays_in_that_row(N, segments):
    run_length(N)
    state = torch.from_numpy(np.random.default_rng(N).uniform(-1.0, 1.0, (4, N + 1))).to(DEV)
    bad = state.clone()
    bad[2, 0] = float("nan")
    x = signal().reshape(4, -1)
    for dt in DTYPES:
        clean, _, sc = run(x, N, 0.7, dt, segments, state=state)
        y, _, st = run(x, N, 0.7, dt, segments, state=bad)
        assert torch.equal(y[[0, 1, 3]], clean[[0, 1, 3]]) and torch.equal(st[[0, 1, 3]], sc[[0, 1, 3]]) and torch.isfinite(clean).all()
        assert not torch.isfinite(y[2]).any() and not torch.isfinite(st[2]).any()


def test_zz_report():
    from tests import phaser_reference as R

    for name, ratio in sorted(R.RATIOS.items()):
        print(f"phaser feedback on the device, {name}: largest deviation / bound {ratio:.3f}")
    assert all(r <= 1.0 for r in R.RATIOS.values())
    for name, ratio in sorted(F.STATE_RATIOS.items()):
        print(f"phaser feedback on the device, end state, {name}: largest deviation / bound {ratio:.3f}")
    assert all(r <= 1.0 for r in F.STATE_RATIOS.values())
