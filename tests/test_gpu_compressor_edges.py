"""The compressor on the device at the edges of its scan (csrc/compressor.hip through torchfx_ext.compressor_forward) against
the per-sample float64 definition (tests/compressor_reference.py), with the cases of tests/compressor_cases.py: a maximum or a
non-finite sample planted at every lane, stride, wave, tile and segment seam, one group per position in one launch; the hold,
fast, tiny, slow and ratio = 1 corners; long segments; the static curve over the dtype's whole range; channel counts, many
groups, state cuts, the empty chunk and strided views.  tests/test_compressor_cases_host.py proves on the CPU that the cases
plant what they claim (which operand of each `max` wins where).  The bounds are the module's (tests/test_gpu_compressor.py),
restated in tests/compressor_cases.py; nothing here is wider."""
import numpy as np
import pytest
import torch

from tests import compressor_cases as C
from tests import compressor_reference as R
from tests.gpu_common import DEV, dev, ext

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dt", C.DTYPES)
TILE, T_SEAMS, FS = C.TILE, C.T_SEAMS, C.FS


def run(x, kw=None, channels=2, state=None, segments=0):
    """The low-level op on a device copy of ``x`` -> NumPy ``(y, g, state)``."""
    st = None if state is None else dev(np.asarray(state, dtype=np.float64))
    y, g, s = ext().compressor_forward(dev(x), *C.reduced(kw or {}), channels, st, True, segments)
    return y.cpu().numpy(), g.cpu().numpy(), s.cpu().numpy()


def test_the_plan_gives_the_geometry_the_cases_assume():
    C.geometry()
    for segments, split in C.LONG_SPLITS.items():
        assert C.long_split(segments) == split, segments
    info = ext().compressor_plan_info
    assert info(C.MANY_T, C.MANY_GROUPS, 1)["segments"] == 1 and info(C.MANY_T, C.MANY_GROUPS, 1)["tiles"] == 2
    assert info(10 * TILE, 512, 1)["segments"] == 1 and info(10 * TILE, 511, 1)["segments"] == 3      # ceil(1024 / 511)
    assert info(10 * TILE, 513, 2)["segments"] == 1 and info(10 * TILE, 341, 1)["segments"] == 4
    assert info(C.MANY_T, 100, 1)["segments"] == 2                     # ceil(1024 / 100) = 11 is clamped to the 2 tiles
    assert info(T_SEAMS, 1, 2)["segments"] == 4


@DT
@pytest.mark.parametrize("name,corner", C.FAMILY_CORNERS, ids=["%s-%s" % fc for fc in C.FAMILY_CORNERS])
def test_planted_families_at_every_corner(name, corner, dt):
    dtype, kw = C.DTYPES[dt], C.CORNERS[corner]
    x, ref = C.family(name, dt), C.reference(name, corner, dt)
    outs = {}
    for segments in ((0, 1, 2, 4, 11) if name == "long" else (1, C.SEGMENTS)):
        outs[segments] = run(x, kw, segments=segments)
        C.check(f"{name} {corner} segments={segments}", outs[segments], C.ref_tuple(ref), dtype, key=(name, corner, dt))
        if corner == "hold":
            C.check_hold(outs[segments][1], ref["v"], f"{name} segments={segments}")
        if corner == "ratio1":                                         # s = 0 gives v = +0: loud input comes back bit for bit
            y, g, st = outs[segments]
            assert np.array_equal(C.bits(y), C.bits(x)) and np.all(g == 1.0) and np.all(st == 0.0)
    for segments in outs:
        if segments != 1:
            C.between(f"{name} {corner} segments={segments} vs 1", outs[segments], outs[1], dtype)


@DT
@pytest.mark.parametrize("corner", C.NONFINITE_CORNERS)
def test_non_finite_at_every_position(corner, dt):
    kw = C.NONFINITE_CORNERS[corner]
    clean, bad, pos = C.nonfinite_input(dt)
    assert len(pos) == len(C.P) and len(clean) == len(pos) + 2
    for segments in (1, C.SEGMENTS):
        C.check_nonfinite(run(clean, kw, segments=segments), run(bad, kw, segments=segments), pos, f"{corner} segments={segments}")


@DT
def test_non_finite_in_each_of_five_channels(dt):
    clean, bad, pos = C.nonfinite_input(dt, 5)
    for segments in (1, C.SEGMENTS):
        C.check_nonfinite(run(clean, channels=5, segments=segments), run(bad, channels=5, segments=segments), pos, f"segments={segments}")


@DT
@pytest.mark.parametrize("knee_db", [C.W, 0.0])
def test_static_curve_over_the_whole_range(knee_db, dt):
    x = C.curve_row(dt)
    for segments in (0, 1):
        got = run(x, dict(C.CURVE_KW, knee_db=knee_db), channels=1, segments=segments)
        C.check_curve(f"curve knee={knee_db} segments={segments}", got, dt, knee_db, key=("curve", knee_db, dt))


@DT
@pytest.mark.parametrize("channels", [3, 5])
def test_the_loudest_channel_is_each_index_in_turn(channels, dt):
    x = C.channel_case(channels, dt)
    ref = R.compress_ref(x, FS)
    for segments in (1, C.SEGMENTS):
        C.check(f"channels={channels} segments={segments}", run(x, channels=channels, segments=segments), ref, C.DTYPES[dt],
                key=("channels", channels, dt))


@DT
def test_many_groups_each_equal_to_the_group_alone(dt):
    x = C.many_groups(dt)
    pick = list(C.MANY_PICK)
    ref = R.compress_ref(x[pick], FS)
    for segments in (0, 2):
        y, g, st = run(x, channels=1, segments=segments)
        C.check(f"600 groups segments={segments}", (y[pick], g[pick], st[pick]), ref, C.DTYPES[dt], key=("groups", dt))
        for k in pick:
            yk, gk, sk = run(x[k:k + 1], channels=1, segments=segments or 1)      # 0 is one segment at 600 groups
            assert np.array_equal(C.bits(y[k:k + 1]), C.bits(yk)) and np.array_equal(C.bits(g[k:k + 1]), C.bits(gk)), (segments, k)
            assert np.array_equal(st[k:k + 1], sk), (segments, k)


@DT
def test_state_cut_at_every_seam(dt):
    x, ref = C.state_case(dt)
    for cut in C.STATE_CUTS:
        ya, ga, sa = run(x[..., :cut])
        for segments in (1, C.SEGMENTS):
            yb, gb, sb = run(x[..., cut:], state=sa, segments=segments)
            C.check(f"cut={cut} segments={segments}", (np.concatenate([ya, yb], -1), np.concatenate([ga, gb], -1), sb), ref,
                    C.DTYPES[dt], key=("cuts", dt))


@DT
def test_silence_with_a_state_decays_as_the_definition_says(dt):
    x = np.zeros((2, 2, T_SEAMS), C.DTYPES[dt])
    st0 = np.array([[12.0, 7.0], [0.25, 30.0]])
    ref = R.compress_ref(x, FS, state=st0)
    aR = R.alphas(FS, 5e-3, 100e-3)[1]
    for segments in (1, C.SEGMENTS):
        got = run(x, state=st0, segments=segments)
        C.check(f"silence segments={segments}", got, ref, C.DTYPES[dt], key=("silence", dt))
        assert np.abs(got[2][:, 0] - st0[:, 0] * aR ** T_SEAMS).max() <= 1e-10


@DT
def test_a_non_finite_state_reaches_every_sample_of_its_group(dt):
    """A NaN in y1 or in yL of the incoming state: with y1 every combine in front of a sample hands it on (the segment loop
    included), with yL the attack stage's; the third group's bits do not move."""
    x = np.concatenate([C.state_case(dt)[0], C.state_case(dt)[0][:1]])
    st0 = np.array([[np.nan, 1.0], [2.0, np.nan], [2.0, 1.0]])
    for kw in C.NONFINITE_CORNERS.values():
        for segments in (1, C.SEGMENTS):
            y, g, st = run(x, kw, state=st0, segments=segments)
            yc, gc, sc = run(x[2:], kw, state=st0[2:], segments=segments)
            assert np.isnan(y[:2]).all() and np.isnan(g[:2]).all() and np.isnan(st[0]).all() and np.isnan(st[1, 1]), (kw, segments)
            assert np.isfinite(st[1, 0]) and np.array_equal(C.bits(y[2:]), C.bits(yc)) and np.array_equal(C.bits(g[2:]), C.bits(gc))
            assert np.array_equal(st[2:], sc)


@DT
def test_empty_chunk_moves_the_state_on_unchanged(dt):
    x = dev(C.state_case(dt)[0])[..., :0]
    st0 = dev(np.array([[12.0, 7.0], [-0.0, 1e-310]]))
    for state, want in ((st0, st0), (None, torch.zeros_like(st0))):
        y, g, st = ext().compressor_forward(x, *C.reduced({}), 2, state, True, 0)
        assert y.shape == (2, 2, 0) and g.shape == (2, 0) and y.dtype == g.dtype == x.dtype
        assert st.data_ptr() != st0.data_ptr() and np.array_equal(C.bits(st.cpu().numpy()), C.bits(want.cpu().numpy()))


@DT
def test_strided_views_through_the_public_function(dt):
    import torchfx_amd as fx

    x, ref = C.state_case(dt)
    xt = dev(np.ascontiguousarray(x[0].T)).transpose(0, 1)              # [2, T] with strides (1, 2)
    wide = dev(np.concatenate([np.full((2, 2, 5), 9.0, x.dtype), x, np.full((2, 2, 3), 9.0, x.dtype)], -1))
    xs = wide[..., 5:5 + T_SEAMS]                                      # a slice of longer rows
    assert not xt.is_contiguous() and not xs.is_contiguous()
    y, g, st = fx.compress(xt, FS, return_gain=True, return_state=True)
    C.check("transposed", (y.cpu().numpy(), g.cpu().numpy(), st.cpu().numpy()), tuple(a[:1] for a in ref), C.DTYPES[dt],
            key=("strided", dt))
    y, g, st = fx.compress(xs, FS, return_gain=True, return_state=True)
    C.check("sliced", (y.cpu().numpy(), g.cpu().numpy(), st.cpu().numpy()), ref, C.DTYPES[dt], key=("strided", dt))


def test_zz_report_largest_deviations():
    """Not a check: prints the largest deviations the tests above saw per family, corner and dtype."""
    C.report()
