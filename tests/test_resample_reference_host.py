"""CPU: the resampler's reference (tests/resample_reference.py) meets every condition tests/test_gpu_resample_edges.py imposes
on the HIP kernels, for the case table and the row lengths used there (imported, not restated) -- so those tests cannot fail
by their own construction -- and every entry of the table lands in the class it is listed for, with the tile counts its lengths
were chosen for, according to the host-only tiling query."""
import numpy as np
import pytest
import scipy.signal as ss
import torch

from tests import resample_reference as R
from tests import test_gpu_resample_edges as G

ENTRIES = G.unique(G.CASES)


def scipy_window(c, dtype):
    w = G.window_of(c)
    return w.astype(dtype) if isinstance(w, np.ndarray) else w


# ---- 1. the reference is SciPy's operation
@pytest.mark.parametrize("c", ENTRIES, ids=G.case_id)
def test_ref_agrees_with_scipy_in_float64(c):
    """float64 signal and taps at the shortest two-tile length: SciPy inside the float64 bound of the long-double reference,
    the float64 reference too, and the shape is ceil(T * up / down)."""
    from torchfx_amd.resample import design_taps
    T = G.lengths(c)["above"]
    p = G.plan(c, T)
    x = np.random.default_rng(c.up + c.down).standard_normal((1, T))
    h = design_taps(c.up, c.down, G.window_of(c), torch.float64).numpy()
    got = ss.resample_poly(x, c.up, c.down, axis=-1, window=scipy_window(c, np.float64))
    wide = R.ref(x, h, c.up, c.down, wide=True)
    assert got.shape == wide.shape == (1, -(-T * c.up // c.down)) == (1, p["n_out"]) and wide.dtype == np.longdouble
    bnd = R.bound(x, h, c.up, c.down, p["Lp"])
    G.check_bound(got, wide, bnd, f"scipy {G.case_id(c)}")
    G.check_bound(R.ref(x, h, c.up, c.down), wide, bnd, f"ref {G.case_id(c)}")


# ---- 2. a float32 evaluation of the same sum stays inside the bound on the staircase
@pytest.mark.parametrize("c", [c for c in ENTRIES if c.dt == "f32" and c.kernel != G.GATHER], ids=G.case_id)
def test_scipy_float32_stays_inside_the_bound_on_staircases(c):
    worst = 0.0
    for T in G.all_lengths(c):
        s = G.stair_case(c, T)
        got = ss.resample_poly(s["x"], c.up, c.down, axis=-1, window=scipy_window(c, np.float32))
        assert got.dtype == np.float32
        worst = max(worst, G.check_bound(got, s["ref"], s["bnd"], f"{G.case_id(c)} T={T}"))
        G.close(got, s["ref"].astype(np.float32), G.TOL[c.dt], f"{G.case_id(c)} T={T}")
    assert worst < 1.0


@pytest.mark.parametrize("c", [c for c in ENTRIES if c.dt == "f64" or c.kernel == G.GATHER], ids=G.case_id)
def test_staircase_references_exist_for_the_other_entries(c):
    """The float64 and gather entries: the staircase has its quiet stretch on the seam and SciPy (in the entry's dtype) meets
    both bars at the shortest two-tile length."""
    T = G.lengths(c)["above"]
    s, p = G.stair_case(c, T), G.plan(c, T)
    assert s["ref"].dtype == (np.longdouble if c.dt == "f64" else np.float64) and s["x"].dtype == G.DT[c.dt]
    a, b = np.abs(s["x"][:, p["seam"] - 64:p["seam"]]).max(), np.abs(s["x"][:, p["seam"]:p["seam"] + 64]).max()
    assert max(a, b) / min(a, b) > 100, "no amplitude step on the seam"
    got = ss.resample_poly(s["x"], c.up, c.down, axis=-1, window=scipy_window(c, G.DT[c.dt]))
    assert got.dtype == G.DT[c.dt]
    G.check_bound(got, s["ref"], s["bnd"], G.case_id(c))
    G.close(got, s["ref"].astype(got.dtype), G.TOL[c.dt], G.case_id(c))


# ---- 3. the reach rule is SciPy's
@pytest.mark.parametrize("c", G.REACH_CASES, ids=G.case_id)
def test_reach_mask_is_scipys_non_finite_pattern(c):
    T = G.lengths(c)["above"]
    pos = G.reach_positions(c, T)
    p = G.plan(c, T)
    assert pos == [0, T - 1, p["seam"], p["seam"] - p["Lp"]] and all(0 <= q < T for q in pos) and len(set(pos)) == 4
    for q in pos:
        r = G.reach_case(c, T, q)
        assert np.isnan(r["x"][0, q]) and r["x"][1, q] == np.inf and r["x"][2, q] == -np.inf and np.isfinite(r["x"][3]).all()
        with np.errstate(all="ignore"):
            got = ss.resample_poly(r["x"], c.up, c.down, axis=-1, window=scipy_window(c, G.DT[c.dt]))
        assert np.array_equal(~np.isfinite(got), r["mask"]), f"{G.case_id(c)} bad input {q}"
        assert r["mask"][:3].any(axis=1).all() and not r["mask"][3].any()
        G.check_bound(got, r["ref0"], r["bnd"], f"{G.case_id(c)} bad input {q}", where=~r["mask"])


# ---- 4. the table reaches its classes, the lengths their tile counts
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_entry_lands_in_its_class(c):
    L = G.lengths(c)
    for kind, T in G.seam_lengths(c):
        G.check_seam(c, kind, T)
    assert L["below"] < L["above"] <= G.MAX_T and L["short"][:2] == [1, 2]
    p = G.plan(c, L["above"])
    assert L["short"][2] == p["Lp"] and p["tile_out"] == c.up * p["G"] * p["E"]
    near = max(1, -(-c.up // c.down))                    # outputs one more input adds
    assert p["tile_out"] - near < G.plan(c, L["below"])["n_out"] <= p["tile_out"], "not as close to tile_out as the ratio allows"


def test_every_class_is_reached_in_the_dtypes_the_table_lists():
    reached = {(c.cls, c.dt) for c in G.CASES}
    classes = {c.cls for c in G.CASES}
    assert classes == {"gather, up > 1", "lds, G halved, up > 1", "lds, G halved, E == 1", "lds, up > 1, full G", "reg, G halved",
                       "reg, up >= 511", "reg, E == 64", "reg, baseline"}
    assert all((cls, "f32") in reached for cls in classes)
    for cls in ("gather, up > 1", "lds, G halved, up > 1", "reg, G halved", "reg, E == 64", "reg, baseline"):
        assert (cls, "f64") in reached, cls
    assert {c.up for c in G.CASES if c.cls == "reg, up >= 511"} == {511, 512, 513}
    halved = [(c, G.plan(c, G.lengths(c)["above"])) for c in G.CASES if c.cls == "lds, G halved, up > 1"]
    assert any(p["G"] % 2 == 1 and (c.up * p["G"]) % 64 for c, p in halved)          # an odd G, up*G no multiple of a wave
    assert len(G.REACH_CASES) == 3 and {c.kernel for c in G.REACH_CASES} == {G.REG, G.LDS, G.GATHER} and all(c.up > 1 for c in G.REACH_CASES)
    assert any(G.lengths(c)["three"] for c in G.CASES if c.kernel == G.GATHER and c.dt == "f32")
    assert any(G.lengths(c)["three"] for c in G.CASES if c.kernel == G.GATHER and c.dt == "f64")
    for c in ENTRIES:                                    # nothing larger than the file allows
        assert max(G.all_lengths(c)) <= G.MAX_T


# ---- 5. impulses
@pytest.mark.parametrize("c", ENTRIES, ids=G.case_id)
def test_reference_impulse_responses_are_the_taps(c):
    """The expected rows are what the definition gives (one non-zero product per output: exact in float64 and in the signal
    dtype), every listed position is in some row, and the taps it meets are normal numbers or zeros."""
    T = G.lengths(c)["above"]
    p, h = G.plan(c, T), G.taps(c)
    tiny = np.finfo(G.DT[c.dt]).tiny
    assert ((np.abs(h) >= 8 * tiny) | (h == 0)).all(), "a subnormal product would not be exact"
    placed = []
    for x, exp in G.impulse_case(c, T):
        assert x.shape[0] <= G.MAX_ROWS and x.dtype == exp.dtype == G.DT[c.dt]
        y = R.ref(x, h, c.up, c.down)
        assert np.array_equal(y.astype(G.DT[c.dt]).astype(np.float64), y), "the definition's value is not exact in the signal dtype"
        G.check_impulses(y.astype(G.DT[c.dt]), exp, G.case_id(c))
        for row in x:
            q = np.flatnonzero(row)
            assert (np.diff(q) > p["Lp"] + 1).all()
            placed += q.tolist()
            assert set(row[q].tolist()) <= set(G.AMPS)
    listed = G.impulse_inputs(c, T)
    assert listed[:8] == [0, 1, T - 2, T - 1, p["seam"] - p["Lp"], p["seam"] - 1, p["seam"], p["seam"] + 1]
    want = {q for q in listed if 0 <= q < T}
    assert sorted(placed) == sorted(want) and {0, 1, T - 2, T - 1, p["seam"] - 1, p["seam"]} <= want
    # the last four are the ends of the windows at the seam: the first output of tile 1 reaches back to listed[9] and
    # no further, the last output of tile 0 forward to listed[10] and no further
    if 0 <= listed[9] < T:
        m = R.reach_mask(T, p["n_out"], c.up, c.down, p["n_pre_remove"], p["Lp"], [(0, listed[9])])[0]
        assert m[p["tile_out"]] and (listed[9] == 0 or not R.reach_mask(T, p["n_out"], c.up, c.down, p["n_pre_remove"], p["Lp"],
                                                                       [(0, listed[9] - 1)])[0, p["tile_out"]])
    if 0 <= listed[10] < T:
        m = R.reach_mask(T, p["n_out"], c.up, c.down, p["n_pre_remove"], p["Lp"], [(0, listed[10])])[0]
        assert m[p["tile_out"] - 1] and (listed[11] >= T or not R.reach_mask(T, p["n_out"], c.up, c.down, p["n_pre_remove"], p["Lp"],
                                                                             [(0, listed[11])])[0, p["tile_out"] - 1])
    assert any(np.count_nonzero(e) for _, e in G.impulse_case(c, T))


def test_rows_of_the_batch_case_differ():
    c = ENTRIES[-1]
    x = G.batch_case(c, 500)
    assert x.shape == (3, 500) and not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])


# ---- the helpers themselves
def test_ref_is_the_definition():
    g = np.random.default_rng(0)
    for up, down, nh, T in [(3, 7, 25, 40), (7, 3, 30, 17), (1, 4, 9, 33), (5, 1, 11, 6), (4, 9, 2, 50), (2, 3, 1, 9)]:
        x, h = g.standard_normal((2, T)), g.standard_normal(nh)
        half = (nh - 1) // 2
        n_out = -(-T * up // down)
        exp = np.zeros((2, n_out))
        for m in range(n_out):
            for i in range(T):
                k = m * down + half - i * up
                if 0 <= k < nh:
                    exp[:, m] += x[:, i] * h[k]
        got = R.ref(x, h, up, down)
        assert got.shape == exp.shape and np.allclose(got, exp, rtol=1e-13, atol=1e-13), (up, down)
        assert np.allclose(got, ss.resample_poly(x, up, down, axis=-1, window=h / up), rtol=1e-12, atol=1e-12), (up, down)
        assert np.array_equal(R.ref(x[0], h, up, down), got[0])
    assert R.ref(x, h, 2, 3, wide=True).dtype == np.longdouble
    assert np.finfo(np.longdouble).nmant >= 63, "float64 kernels are judged against a wider accumulation"
    assert R.ref(np.zeros((2, 0)), h, 2, 3).shape == (2, 0)


def test_bound_is_the_stated_formula():
    g = np.random.default_rng(1)
    x, h = g.standard_normal((1, 40)).astype(np.float32), g.standard_normal(9).astype(np.float32)
    s = R.ref(np.abs(x).astype(np.float64), np.abs(h).astype(np.float64), 2, 3)
    u = 2.0 ** -24
    assert np.allclose(R.bound(x, h, 2, 3, 5), 6 * u / (1 - 6 * u) * s + 5 * 2.0 ** -126, rtol=1e-12, atol=0)
    u = 2.0 ** -53
    assert np.allclose(R.bound(x.astype(np.float64), h, 2, 3, 5), 6 * u / (1 - 6 * u) * s + 5 * 2.0 ** -1022, rtol=1e-12, atol=0)
    assert (R.bound(np.zeros((1, 8), np.float32), h, 2, 3, 5) == 5 * 2.0 ** -126).all()


def test_reach_mask_impulses_and_staircase():
    # up 2, down 3, pre_remove 1, Lp 2: output m sees inputs n // 2 - {0, 1}, n = (m + 1) * 3
    m = R.reach_mask(10, 7, 2, 3, 1, 2, [(0, 0), (1, 4), (1, 5)], rows=3)
    assert m[0].tolist() == [True] + [False] * 6                      # n = 3: inputs 1, 0
    assert m[1].tolist() == [False, False, True, True, False, False, False]      # n = 9: 4, 3; n = 12: 6, 5
    assert not m[2].any()
    x = R.impulses(9, [0, 8], [1.0, -0.5], np.float64)
    assert x.tolist() == [1.0] + [0.0] * 7 + [-0.5] and R.impulses(3, [], []).dtype == np.float32
    h = np.arange(1.0, 8.0)
    # half = 3: y[m] = 0.125 * h[m + 3 - 2]
    assert R.impulse_response(4, h, 2, 1, [1], [0.125]).tolist() == [0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 0.0, 0.0]
    assert R.staircase is __import__("tests.fir_reference", fromlist=["staircase"]).staircase


def test_tiling_query_is_the_launch_plan():
    """tfx_resample_tiling_info: same checks and same plan as tfx_resample_plan_info, the geometry the kernel comment states,
    zeros for the copy, and an error code (not a crash) for a null output or bad arguments."""
    import ctypes

    from torchfx_amd import _lib, torchfx_ext
    for c in ENTRIES:
        for T in G.all_lengths(c):
            p = G.plan(c, T)                             # asserts kernel and tiles against resample_plan_info
            assert p["tile_out"] == c.up * p["G"] * p["E"] and 1 <= p["G"] <= p["G_initial"] == max(1, 512 // c.up)
            assert 1 <= p["E"] <= 64 and p["LP"] >= p["Lp"] and (p["LP"] == p["Lp"]) == (p["kernel"] != G.REG or p["Lp"] in (8, 16, 24, 32, 48, 64))
            esz = 4 if c.dt == "f32" else 8
            assert p["span"] * esz == p["lds_bytes"] <= 49152 and (p["span"] == 0) == (p["kernel"] == G.GATHER)
    assert torchfx_ext.resample_tiling_info(1000, 6, 4, 61) == torchfx_ext.resample_tiling_info(1000, 3, 2, 61)      # reduced by the gcd
    assert torchfx_ext.resample_tiling_info(1000, 7, 7, 1) == dict(kernel="copy", G=0, G_initial=0, E=0, tile_out=0, span=0, LP=0, tiles=0)
    assert torchfx_ext.resample_tiling_info(0, 3, 2, 61)["tiles"] == 0
    with pytest.raises(RuntimeError, match="up and down must be >= 1"):
        torchfx_ext.resample_tiling_info(10, 0, 3, 5)
    lib = _lib.load()
    o, k = ctypes.c_int64(), ctypes.c_int()
    assert lib.tfx_resample_tiling_info(10, 2, 3, 5, 0, ctypes.byref(k), *[ctypes.byref(o)] * 7) == 0
    assert lib.tfx_resample_tiling_info(10, 2, 3, 5, 0, None, *[ctypes.byref(o)] * 7) != 0
    assert b"null output" in lib.tfx_last_error()
    assert lib.tfx_resample_tiling_info(10, 2, 3, 5, 7, ctypes.byref(k), *[ctypes.byref(o)] * 7) != 0
