"""The compressor edge tests' cases without a GPU (tests/compressor_cases.py): the geometry against the host-only plan query,
the census -- computed from the per-sample reference's v and y1 on the very signals the GPU tests use -- of which operand of the
release stage's `max` wins at every lane, stride, wave, tile and segment boundary, and every family and corner through the CPU
path of compress() (a second, differently associated scan) against the per-sample loop within the module's bounds.  This pins
the cases and the reference before anything runs on a device."""
import numpy as np
import pytest
import torch

from tests import compressor_cases as C
from tests import compressor_reference as R

DT = pytest.mark.parametrize("dt", C.DTYPES)
HOST_CORNERS = [(f, c) for f, c in C.FAMILY_CORNERS if c != "tiny"]          # compress() takes times, not coefficients


def host(x, **kw):
    import torchfx_amd

    y, g, st = torchfx_amd.compress(torch.from_numpy(np.array(x)), C.FS, return_gain=True, return_state=True, **kw)
    return y.numpy(), g.numpy(), st.numpy()


def test_the_geometry_is_what_the_plan_says():
    C.geometry()
    for segments, split in C.LONG_SPLITS.items():
        assert C.long_split(segments) == split, segments
    assert len(C.P) == 26 and C.P[0] == 0 and C.P[-1] == C.T_SEAMS - 1
    a = {n - C.TILE for n in C.P if C.in_tile_1(n)}
    assert {0, 7, 8, 15, 2047} <= a and {8 * 2 ** j - e for j in range(1, 6) for e in (0, 1)} <= a
    assert {w * C.WAVE - e for w in (1, 2, 3) for e in (0, 1)} <= a
    cls = C.boundary_classes()
    for j in range(6):                                                 # lane 2^j of wave 0 of tile 1 starts at a planted position
        assert C.TILE + 8 * 2 ** j in cls["stride%d" % j] and C.TILE + 8 * 2 ** j in C.P
    assert set(cls["wave"][C.in_tile_1(cls["wave"])]) <= set(C.P) and set(cls["segment"]) | set(cls["tile"]) <= set(C.P)


def test_the_corners_are_what_they_claim():
    from torchfx_amd.dynamics import CompressorParams

    hold = CompressorParams(C.FS, torch.float32, **C.CORNERS["hold"])
    assert hold.alpha_r == 1.0 and hold.alpha_a == 0.0 and R.alphas(C.FS, 0.0, 1e300) == (0.0, 1.0)
    fast = CompressorParams(C.FS, torch.float32, **C.CORNERS["fast"])
    assert abs(fast.alpha_a - 0.5) <= 1e-15 and fast.alpha_a == fast.alpha_r and fast.alpha_r ** C.TILE == 0.0
    assert C.reduced(C.CORNERS["tiny"])[3:5] == (1e-200, 1e-200) and 1e-200 ** 8 == 0.0
    assert CompressorParams(C.FS, torch.float32, **C.CORNERS["ratio1"]).s == 0.0
    edge = 10.0 ** ((C.TH - C.W / 2) / 20.0)
    for dt in C.DTYPES:
        assert np.abs(C.family("click_silent", dt)).min(1).max() <= 0.06 < edge       # all but the clicks: v = 0
        assert np.abs(C.family("click_loud", dt)).min() >= 0.0999


@DT
def test_census_a_clicks_carry_is_live_to_the_end_of_the_row(dt):
    for name, corner in [("click_silent", "defaults")] + [("click_loud", c) for c in C.LIVE_CORNERS]:
        ref = C.reference(name, corner, dt)
        for k, n0 in enumerate(C.P):
            lv = C.live(ref["v"][k], ref["y1"][k])
            assert not lv[n0] and lv[n0 + 1:].all(), (name, corner, k, n0)
    silent = C.reference("click_silent", "defaults", dt)
    aR = R.alphas(C.FS, 5e-3, 100e-3)[1]
    for k, n0 in enumerate(C.P):                                       # everything after the click is carry: y1 = v0 aR^m
        m = np.arange(C.T_SEAMS - n0)
        assert np.all(silent["v"][k][:n0] == 0) and np.all(silent["v"][k][n0 + 1:] == 0)
        assert np.abs(silent["y1"][k][n0:] - silent["v"][k][n0] * aR ** m).max() <= 1e-11


@DT
def test_census_the_staircase_beats_the_carry_at_every_step_and_nowhere_else(dt):
    cls = C.boundary_classes()
    planted = np.zeros(C.T_SEAMS, bool)
    planted[list(C.P)] = True
    for corner in C.LIVE_CORNERS:
        ref = C.reference("staircase", corner, dt)
        v, lv = ref["v"][0], C.live(ref["v"][0], ref["y1"][0])
        assert np.all(np.diff(v[list(C.P)]) > 0) and np.all(v[~planted] == 0)
        assert not lv[planted].any(), corner
        for name, pos in cls.items():
            rest = pos[~planted[pos]]
            assert lv[rest].all(), (corner, name)


@DT
def test_census_every_boundary_class_has_a_live_and_a_dead_carry(dt):
    """Over all families at the defaults: in tile 1 (the second tile of segment 0) for the lanes, strides and waves, at tile 1's
    first sample for the tile carry, and at each of the two segment seams."""
    cls = C.boundary_classes()
    seen = {name: {True: set(), False: set()} for name in cls}
    for name in ("click_silent", "click_loud", "staircase"):
        ref = C.reference(name, "defaults", dt)
        for v, y1 in zip(ref["v"], ref["y1"]):
            lv = C.live(v, y1)
            for c, pos in cls.items():
                pos = pos[C.in_tile_1(pos)] if c not in ("tile", "segment") else pos
                for state in (True, False):
                    seen[c][state] |= set(pos[lv[pos] == state].tolist())
    for c, s in seen.items():
        print(c, "live at", len(s[True]), "positions, dead at", len(s[False]))
        assert s[True] and s[False], c
    assert seen["segment"][True] == seen["segment"][False] == {2 * C.TILE, 3 * C.TILE}
    # the long-segment case: a live carry across every cut of 6 + 5 and 3 + 3 + 3 + 2, and a dead one at the burst across tile 6
    ref = C.reference("long", "defaults", dt)
    for v, y1 in zip(ref["v"], ref["y1"]):
        lv = C.live(v, y1)
        assert lv[[3 * C.TILE, 9 * C.TILE]].all() and not lv[6 * C.TILE - 40:6 * C.TILE + 60].all()


@DT
def test_every_case_keeps_the_gain_normal_in_float32(dt):
    for name, corner in C.FAMILY_CORNERS:
        ref = C.reference(name, corner, dt)
        assert ref["g"].min() >= C.G_MIN and np.isfinite(ref["y"]).all(), (name, corner)
    for name in ("click_loud", "staircase"):
        assert np.all(C.reference(name, "ratio1", dt)["v"] == 0) and np.all(C.reference(name, "ratio1", dt)["g"] == 1.0)
        g = C.reference(name, "ratio1_makeup", dt)["g"]
        assert np.abs(g / 10 ** (4.5 / 20) - 1).max() <= 1e-15


@DT
def test_hold_records_are_far_enough_apart_to_count(dt):
    """check_hold counts distinct gains: two successive records of the reference must differ by more than float32 resolves."""
    for name in ("click_loud", "staircase"):
        ref = C.reference(name, "hold", dt)
        assert np.array_equal(ref["y1"], C.running_maximum(ref["v"]))                 # no rounding anywhere
        for g in ref["g"]:
            steps = np.unique(g)
            assert np.all(np.diff(steps) / steps[1:] > 2.0 ** -21), name
        C.check_hold(ref["g"], ref["v"], name)
        C.check_hold(ref["g"].astype(np.float32), ref["v"], name)


@DT
@pytest.mark.parametrize("name,corner", HOST_CORNERS, ids=["%s-%s" % fc for fc in HOST_CORNERS])
def test_the_cpu_path_meets_the_bounds_on_every_family_and_corner(name, corner, dt):
    x = C.family(name, dt)
    ref = C.reference(name, corner, dt)
    got = host(x, **C.CORNERS[corner])
    C.check(f"host {name} {corner}", got, C.ref_tuple(ref), C.DTYPES[dt], key=("host", name, corner, dt))
    if corner == "hold":
        C.check_hold(got[1], ref["v"], name)
    if corner == "ratio1":
        assert np.array_equal(C.bits(got[0]), C.bits(x)) and np.all(got[1] == 1.0) and np.all(got[2] == 0.0)


@DT
@pytest.mark.parametrize("corner", C.NONFINITE_CORNERS)
def test_the_cpu_path_and_the_reference_hand_a_non_finite_sample_on_from_every_position(corner, dt):
    kw = C.NONFINITE_CORNERS[corner]
    for channels in (2, 5):
        clean, bad, pos = C.nonfinite_input(dt, channels)
        C.check_nonfinite(host(clean, **kw), host(bad, **kw), pos, f"host {corner} channels={channels}")
    clean, bad, pos = C.nonfinite_input(dt, 5)                          # the definition itself, on the small case
    ref_c, ref_b = R.compress_ref(clean, C.FS, **kw), R.compress_ref(bad, C.FS, **kw)
    C.check_nonfinite(ref_c, ref_b, pos, f"reference {corner}")


@DT
@pytest.mark.parametrize("knee_db", [C.W, 0.0])
def test_the_cpu_path_meets_the_static_curves_bounds(knee_db, dt):
    x = C.curve_row(dt)
    assert x.shape[-1] > 2 * C.TILE and np.signbit(x[0, 0, 1]) and x[0, 0, 2] > 0 and x[0, 0, 2] / x.dtype.type(2) == 0
    C.check_curve(f"host curve knee={knee_db}", host(x, knee_db=knee_db, **C.CURVE_KW), dt, knee_db, key=("host", "curve", knee_db, dt))
    v = np.array([R.curve(abs(float(p)), C.TH, 0.75, knee_db) for p in x.reshape(-1)])
    if knee_db:                                                        # all three branches are sampled, and both knee edges closely
        o = 20 * np.log10(np.abs(x.reshape(-1).astype(np.float64)) + 1e-320) - C.TH
        assert (2 * o <= -knee_db).sum() > 100 and (2 * o >= knee_db).sum() > 100 and (np.abs(2 * o) < knee_db).sum() > 100
    assert (v == 0).sum() > C.TILE and v.max() > 500


@DT
def test_the_cpu_path_meets_the_bounds_on_the_channel_group_and_state_cases(dt):
    dtype = C.DTYPES[dt]
    for channels in (3, 5):
        x = C.channel_case(channels, dt)
        for k in range(channels):                                      # the loudest sample: negative, in channel k alone
            n = np.abs(x[k]).max(0).argmax()
            assert x[k, k, n] == -1.5 and np.abs(np.delete(x[k], k, 0)).max() <= 0.2
        C.check(f"host channels={channels}", host(x), R.compress_ref(x, C.FS), dtype, key=("host", "channels", channels, dt))
    x = C.many_groups(dt)[list(C.MANY_PICK)]
    C.check("host picked groups", host(x), R.compress_ref(x, C.FS), dtype, key=("host", "groups", dt))
    x, ref = C.state_case(dt)
    for cut in C.STATE_CUTS:
        ya, ga, sa = host(x[..., :cut])
        yb, gb, sb = host(x[..., cut:], state=torch.from_numpy(sa))
        C.check(f"host cut={cut}", (np.concatenate([ya, yb], -1), np.concatenate([ga, gb], -1), sb), ref, dtype, key=("host", "cuts", dt))


def test_zz_report_largest_deviations():
    """Not a check: prints the largest deviations of the CPU path per family, corner and dtype."""
    C.report()
