"""The tables of tests/waveshaper_cases.py against the real plan queries, without a GPU: which tap counts reach which register
bucket of waveshaper_kernel, that equal stages always give a tile origin I0 = 0 and the unequal pairs do not, that neither plan
refuses a pair of tap counts, that the stream's geometry does not depend on the chunk length, that the exact tap probes of
tests/test_gpu_waveshaper_edges.py expect representable values, read every tap and tell a reversed, shifted or swapped tap array
from the right one, that the signals of its bound test put the transfer function to work, and the refusal of gains that are
not finite in the signal's dtype.

The wet part.  The bound test's second run has wet = 0.3 * 10^(-6/20) = 0.150, and |z| <= (1 + |c0|) * (the largest sum of |h_dn|
over the taps that meet a non-zero shaped sample).  With a one-tap up-sampler only every L-th shaped sample is non-zero, so the
pair (1, 64 L) cannot show more than wet (1 + |c0|) max_phase sum|h_dn[phase::L]|, about 0.17 / L: 0.043 at L = 4, 0.022 at L = 8,
under the 0.05 asked of every other run.  Those runs are held to half of that ceiling instead (`wet_floor`)."""
import numpy as np
import pytest
import torch

from tests import waveshaper_cases as C
from tests import waveshaper_reference as R
from torchfx_amd import torchfx_ext as E
from torchfx_amd import waveshape

raw_geometry = C.geometry.__wrapped__


@pytest.mark.parametrize("L", C.LS)
def test_every_bucket_is_reached_and_equal_stages_start_at_the_first_output(L):
    by_bucket = {}
    for nh in range(1, 64 * L + 1):
        for dtype in C.DTYPES:
            g = raw_geometry(L, nh, nh, dtype)
            assert g["I0"] == 0, (L, nh, g)
            by_bucket.setdefault(g["bucket"], set()).add(nh)
    assert tuple(sorted(by_bucket)) == C.BUCKETS
    for b in C.BUCKETS:
        assert (min(by_bucket[b]), max(by_bucket[b])) == C.nh_range(L, b), (L, b)
        assert by_bucket[b] == set(range(min(by_bucket[b]), max(by_bucket[b]) + 1))
        assert sorted(nh for l, bb, nh in C.EQUAL if (l, bb) == (L, b)) == sorted(set(C.nh_range(L, b)))
    assert by_bucket[72] == {64 * L}
    assert raw_geometry(L, C.nh_range(L, 8)[0], 1, torch.float32)["Lp_up"] == 2
    for b in C.BUCKETS[:-1]:
        assert raw_geometry(L, C.nh_range(L, b)[1], C.nh_range(L, b)[1], torch.float32)["Lp_up"] == b
    for dtype in C.DTYPES:                                           # the rotations of the GPU tests lose no bucket
        assert sorted({C.geometry(*c, dtype)["bucket"] for c in C.equal_cases(dtype)}) == list(C.BUCKETS)
        assert [C.geometry(*c, dtype)["bucket"] for c in C.smallest_cases(dtype)] == list(C.BUCKETS)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DT_ID.get)
@pytest.mark.parametrize("L", C.LS)
def test_unequal_stages_move_the_tile_origin(L, dtype):
    got = {(c.nh_up, c.nh_dn): C.geometry(*c, dtype) for c in C.UNEQUAL if c.L == L}
    print({k: (g["bucket"], g["I0"], g["reach_before"], g["reach_after"]) for k, g in got.items()})
    assert (got[(1, 64 * L)]["bucket"], got[(1, 64 * L)]["I0"]) == (8, -32)
    assert (got[(64 * L, 1)]["bucket"], got[(64 * L, 1)]["I0"]) == (72, 32)
    assert got[(64 * L - 1, 2)]["bucket"] == 64 and got[(64 * L - 1, 2)]["I0"] > 0
    assert got[(3 * L + 1, 40 * L)]["bucket"] == 8 and got[(3 * L + 1, 40 * L)]["I0"] < 0
    assert got[(40 * L, 3 * L + 2)]["bucket"] == 48 and got[(40 * L, 3 * L + 2)]["I0"] > 0
    for g in got.values():                                           # what the stream's dry sample and the window rely on
        assert g["I0"] <= g["bucket"] - 1 and g["reach_before"] >= 1 and g["reach_after"] >= 0


@pytest.mark.parametrize("L", C.LS)
def test_neither_plan_refuses_a_pair_of_tap_counts(L):
    top = 64 * L
    grid = range(1, top + 1) if L == 2 else sorted(set(range(1, top + 1, 7 if L == 4 else 5)) | {1, 2, top - 1, top})
    n = 0
    for dtype in C.DTYPES:
        for a in grid:
            for b in grid:
                g = raw_geometry(L, a, b, dtype, 5000)               # raises on a refusal
                assert g["tile"] >= (1024 if dtype == torch.float32 else 512) and -32 <= g["I0"] <= 32, (L, a, b, g)
                n += 1
    print(f"L = {L}: {n} plans, none refused")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DT_ID.get)
def test_reach_latency_and_history_do_not_depend_on_the_length(dtype):
    cases = [C.Case(L, nh, nh) for L, b, nh in C.EQUAL] + C.UNEQUAL + [C.probe_case(p) for p in C.PROBES]
    for c in cases:
        a, b = raw_geometry(*c, dtype, 1), raw_geometry(*c, dtype, 3000)
        assert a == b, (c, a, b)


def reference_forward(dtype):
    wide = dtype == torch.float64
    return lambda x, L, hu, hd: R.ref(x, L, hu, hd, "hard", wide=wide).astype(C.NP[dtype])


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DT_ID.get)
@pytest.mark.parametrize("p", C.PROBES, ids=C.probe_id)
def test_probes_expect_representable_values_and_read_every_tap(p, dtype):
    """run_probe asserts that every expected output survives the cast to the dtype and back and equals the closed form."""
    seen, clipped = C.run_probe(p, dtype, reference_forward(dtype))
    assert seen == set(range(p.nh)), sorted(set(range(p.nh)) - seen)[:8]
    assert clipped or p.stage == "dn"                                # some |a h_up| > 1 came out as exactly +-1
    assert C.geometry(*C.probe_case(p), dtype)["bucket"] == (C.bucket_of(-(-(p.nh + 1) // p.L)) if p.stage == "up" else 8)
    x, sites = C.probe_input(p, dtype)
    g = C.geometry(*C.probe_case(p), dtype)
    assert sites[2] + 1 == sites[3] == g["tile"] and sites[4] == x.shape[-1] - 1 and x.shape[-1] % 2 == 1


WRONG = {
    "reversed": lambda p: (lambda hu, hd: (hu[::-1].copy(), hd) if p.stage == "up" else (hu, hd[::-1].copy())),
    "shifted": lambda p: (lambda hu, hd: (np.roll(hu, 1), hd) if p.stage == "up" else (hu, np.roll(hd, 1))),
    "swapped": lambda p: (lambda hu, hd: (hd, hu)),
}


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DT_ID.get)
@pytest.mark.parametrize("how", sorted(WRONG))
@pytest.mark.parametrize("p", C.UP_PROBES[:3] + C.DN_PROBES, ids=C.probe_id)
def test_the_probe_tells_wrong_taps_from_right_ones(p, how, dtype):
    with pytest.raises(AssertionError, match="nh"):
        C.run_probe(p, dtype, reference_forward(dtype), wrong=WRONG[how](p))


def wet_floor(c, dtype, kw, shape, curve):
    """0.05, or half of the ceiling where the geometry cannot show 0.05 at all (the module docstring)."""
    hu, hd = C.stage_taps(c, dtype)
    drive, b, dry, wet = R.params(C.NP[dtype], **kw)
    top = 1.0 + abs(R.c0_of(C.NP[dtype], shape, kw.get("bias", 0.0), curve))
    reach = max(np.abs(hd[ph::c.L]).sum() for ph in range(c.L)) if c.nh_up == 1 else np.abs(hd).sum()
    ceiling = wet * top * float(reach)
    return 0.05 if ceiling > 0.05 else 0.5 * ceiling


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DT_ID.get)
def test_the_bound_tests_signals_put_the_shapes_to_work(dtype):
    lowered = []
    for c in C.equal_cases(dtype) + C.UNEQUAL:
        g = C.geometry(*c, dtype)
        x = C.signal(3, C.two_tile_length(g), 7, dtype)
        hu, hd = C.stage_taps(c, dtype)
        for name, kw in (("hard", C.KW_HARD), (C.soft_shape(c), C.KW_SOFT)):
            shape, curve = C.shape_args(name)
            y, u, v, w, z, (drive, b, dry, wet, c0) = R.ref(x, c.L, hu, hd, shape, curve=curve, parts=True, **kw)
            if name == "hard":
                share = float((np.abs(v) > 1).mean())
                assert 0.05 <= share <= 0.95, (c, share)
            floor = wet_floor(c, dtype, kw, shape, curve)
            if floor < 0.05:
                lowered.append((tuple(c), name, round(floor, 4)))
            if c.nh_up == 1 and c.nh_dn > 1:
                print(f"wet part of {tuple(c)} {name}: {np.abs(y - dry * x.astype(np.float64)).max():.4f} (floor {floor:.4f})")
            part = float(np.abs(y - dry * x.astype(np.float64)).max())
            assert part > floor, (c, name, part, floor)
    print("runs held to half of their ceiling instead of 0.05:", lowered)
    assert {(k[0][0], k[0][1], k[0][2]) for k in lowered} <= {(4, 1, 256), (8, 1, 512)} and all(k[1] != "hard" for k in lowered)


def test_gains_that_are_not_finite_in_the_signals_dtype_are_refused():
    lib = E.L.load()

    def call(dtype_code, drive=1.0, bias=0.0, dry=0.0, wet=1.0):          # rows = 0: argument checks only, no device
        return lib.tfx_waveshaper_forward(None, None, dtype_code, 0, 16, 1, 2, None, 0, drive, bias, dry, wet, None, 0, None, 0, None)

    assert call(0) == 0 and call(1) == 0
    for kw in (dict(drive=1e39), dict(bias=-1e39), dict(dry=1e39), dict(wet=1e300)):
        assert call(0, **kw) != 0, kw
        assert b"must be finite in float32" in lib.tfx_last_error()
        assert call(1, **kw) == 0, kw
    assert call(1, drive=float("inf")) != 0 and b"must be finite in float64" in lib.tfx_last_error()
    assert lib.tfx_waveshaper_stream_forward(None, None, 0, 0, 16, 16, 0, 1, 2, None, 0, 1e39, 0.0, 0.0, 1.0, None, 0, None, 0, None, None,
                                             None) != 0
    assert b"waveshaper_stream_forward: drive, bias, dry and wet must be finite in float32" in lib.tfx_last_error()
    assert lib.tfx_waveshaper_stream_forward(None, None, 1, 0, 16, 16, 0, 1, 2, None, 0, 1e39, 0.0, 0.0, 1.0, None, 0, None, 0, None, None,
                                             None) == 0
    with pytest.raises(ValueError, match="drive must be finite in the signal's dtype torch.float32"):
        waveshape(torch.zeros(8), drive_db=800.0)
    with pytest.raises(ValueError, match="wet must be finite in the signal's dtype torch.float32"):
        waveshape(torch.zeros(2, 0), output_db=800.0)
    y = waveshape(torch.zeros(8, dtype=torch.float64), drive_db=800.0)
    assert y.dtype == torch.float64 and float(y.abs().max()) == 0.0
    from torchfx_amd.realtime import StatefulWaveshaper

    with pytest.raises(ValueError, match="drive must be finite in the signal's dtype torch.float32"):
        StatefulWaveshaper("tanh", drive_db=800.0)(torch.zeros(2, 8))
