"""CPU: the Delay's reference (tests/delay_reference.py) against the torch composition the kernels promise to equal, and the case
table of tests/test_gpu_delay_edges.py (imported, not restated) against the host-only tiling query -- so those tests cannot
fail by their own construction: the exact inputs are exact, the bound holds for the composition, `reach` is the composition's
NaN / Inf map, and every entry lands in the class it is listed for."""
import ctypes

import numpy as np
import pytest
import torch

from tests import delay_reference as R
from tests import test_gpu_delay_edges as G

PAIRS = [(256, 8), (300, 8), (37, 4), (1, 5), (0, 3), (3, 70), (3, 5000), (300, 16)]


def cpu_composition(x, D, taps, feedback, mix, pp):
    t = torch.from_numpy(np.ascontiguousarray(x))
    t = t.view(t.shape[0] // 2, 2, t.shape[-1]) if pp else t
    return G.composition(t, D, taps, feedback, mix, pp).reshape(x.shape[0], x.shape[-1] + taps * D).numpy()


def assert_exact(got, ref, dtype, what):
    """`ref` (float64) is representable in `dtype` and `got` equals it."""
    assert got.dtype == dtype and np.array_equal(ref.astype(dtype).astype(np.float64), ref), f"{what}: the reference needs more bits"
    G.check_exact(got, ref, what)


# ---- 1. the exact inputs are exact
@pytest.mark.parametrize("pp", [False, True], ids=["mono", "pp"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("D,taps", PAIRS)
def test_composition_equals_the_reference_on_integer_signals(D, taps, dt, pp):
    """Integers in [-1000, 1000], feedback 0.5 up to 8 taps and 1.0 above, the five mixes: every product, sum and lerp is exactly
    representable, so torch on the CPU and the float64 definition agree bit for bit."""
    rows, T = (4 if pp else 2), 3000
    x = np.random.default_rng(D + taps).integers(-1000, 1001, (rows, T)).astype(G.DT[dt])
    fb = 0.5 if taps <= 8 else 1.0
    for mix in G.MIXES:
        y, S = R.delay_ref(x, D, taps, fb, mix, pp)
        assert y.shape == S.shape == (rows, T + taps * D) and y.dtype == np.float64
        assert_exact(cpu_composition(x, D, taps, fb, mix, pp), y, G.DT[dt], f"D={D} taps={taps} {dt} pp={pp} mix={mix}")


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_exact_inputs_of_the_table_are_exact(c):
    """The signals test_exact_echoes and the T = 1 test run, at the entry's own shape."""
    fb = G.feedback_of(c)
    for mix in (0.25, 0.75):
        for x in (G.int_signal(c, 1), G.int_signal(c, 3, T=1)):
            assert x.shape == (G.rows_of(c), x.shape[1]) and np.abs(x).max() <= 1000 and np.array_equal(x, np.round(x))
            y, _ = R.delay_ref(x, c.D, c.taps, fb, mix, c.pp)
            assert_exact(cpu_composition(x, c.D, c.taps, fb, mix, c.pp), y, G.DT[c.dt], f"{G.case_id(c)} T={x.shape[1]} mix={mix}")
    assert not np.array_equal(G.int_signal(c, 1), G.int_signal(c, 2))


# ---- 2. the bound holds for the composition
def test_bound_holds_for_the_composition_on_noise():
    worst = 0.0
    for D, taps in [(37, 4), (300, 16), (513, 8), (3, 70), (1200, 3)]:
        for dt in ("f32", "f64"):
            for pp in (False, True):
                x = np.random.default_rng(D * taps).uniform(-1, 1, (4 if pp else 2, 3000)).astype(G.DT[dt])
                dry, wet, S = R.wet_dry(x, D, taps, 0.7, pp)
                bnd = R.bound(S, taps, G.DT[dt])
                for mix in (0.0, 0.3, 0.5, 0.65, 1.0):
                    got = cpu_composition(x, D, taps, 0.7, mix, pp)
                    worst = max(worst, G.check_bound(got, R.mix_of(dry, wet, mix), bnd, f"D={D} taps={taps} {dt} pp={pp} mix={mix}"))
    print(f"\ndelay err/bound of the CPU composition: {worst:.4f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_bound_holds_for_the_composition_on_the_tables_noise(c):
    """The signals, feedback and mixes of test_noise_within_the_bound, at the entry's own shape."""
    n = G.noise_case(c)
    bnd = R.bound(n["S"], c.taps, G.DT[c.dt])
    assert n["x"].dtype == G.DT[c.dt] and n["x"].shape == (G.rows_of(c), c.T) and np.abs(n["x"]).max() <= 1
    for mix in (0.3, 0.65):
        got = cpu_composition(n["x"], c.D, c.taps, G.noise_feedback(c), mix, c.pp)
        G.check_bound(got, R.mix_of(n["dry"], n["wet"], mix), bnd, f"{G.case_id(c)} mix={mix}")


def test_bound_is_zero_exactly_where_nothing_arrives():
    """Ping-pong: row 0 hears nothing before 2 D; S = 0 there and the bound asks for an exact 0."""
    x = np.ones((2, 10), np.float32)
    y, S = R.delay_ref(x[:, :0], 7, 3, 0.5, 0.3, True)
    assert y.shape == (2, 21) and not y.any() and not S.any()
    y, S = R.delay_ref(x, 20, 3, 0.5, 0.3, True)
    assert (S[0, 10:40] == 0).all() and (S[0, 40:50] == 0.5).all() and (S[1, 20:30] == 1).all() and (S[1, 60:70] == 0.25).all()
    assert (R.bound(S, 3, np.float32)[0, 10:40] == 0).all() and R.bound(S, 3, np.float32)[0, 0] == R.gamma(9, 2.0 ** -24)


# ---- 3. reach is the composition's NaN / Inf map
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_reach_is_the_compositions_non_finite_map(c):
    for pos in G.reach_positions(c):
        r = G.reach_case(c, pos)
        bad = G.bad_samples(c, pos)
        assert len({q for _, q in bad}) == len(bad) and r["mask"].any(axis=1).all(), bad
        got = cpu_composition(r["x"], c.D, c.taps, 0.5, 0.3, c.pp)
        assert np.array_equal(~np.isfinite(got), r["mask"]), f"{G.case_id(c)} bad samples {bad}"
        clean = cpu_composition(r["x0"], c.D, c.taps, 0.5, 0.3, c.pp)
        keep = ~r["mask"]
        assert np.isfinite(clean).all() and np.array_equal(G.bits(got)[keep], G.bits(clean)[keep])


def test_reach_positions_sit_on_the_seams():
    """A three-chunk lattice entry gets the last input of chunk 0 and the first of chunk 1; a span entry both sides of tile 1."""
    c = next(c for c in G.CASES if (c.D, c.taps, c.dt, c.pp) == (513, 8, "f32", False))
    assert G.reach_positions(c) == [0, 40 * 513 - 1, 16 * 513 - 1, 16 * 513, 16 * 513 + 512]
    c = next(c for c in G.CASES if (c.D, c.taps, c.dt, c.pp) == (37, 4, "f32", True))
    assert G.reach_positions(c) == [0, 2052, 1023, 1024]
    c = next(c for c in G.CASES if (c.D, c.taps, c.T) == (4097, 2, 300))
    assert G.reach_positions(c) == [0, 299]


# ---- 4. the table against the plan
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_every_entry_lands_in_its_class(c):
    from torchfx_amd import torchfx_ext
    for T in (c.T, 0, 1):
        p = G.check_class(c, T)
        assert p["regime"] == torchfx_ext.delay_regime(c.D, c.taps, G.TDT[c.dt], c.pp)
        assert p["lds_bytes"] == ((2 if c.pp else 1) * (c.taps * c.D + G.TILE) * (4 if c.dt == "f32" else 8) if c.cls == G.SPAN else 0)
        assert p["lds_bytes"] <= 65536


def test_table_covers_every_class_and_selection_edge():
    from torchfx_amd import torchfx_ext
    seen = {(c.cls, c.dt, c.pp) for c in G.CASES}
    assert seen == {(k, dt, pp) for k in (G.SPAN, G.LATTICE, G.GATHER) for dt, pp in G.VARIANTS}
    assert {(c.dt, c.pp) for c in G.CASES if c.cls == G.LATTICE and dict(c.want).get("nchunks") == 3} == set(G.VARIANTS)
    assert {c.cls for c in G.EPILOGUE_CASES} == {G.SPAN, G.LATTICE, G.GATHER} and any(c.pp and c.cls == G.LATTICE for c in G.EPILOGUE_CASES)
    reg = torchfx_ext.delay_regime
    for dt, pp in G.VARIANTS:
        t = G.TDT[dt]
        # the 64 KiB fit: LDS_EDGE is the largest D that is span with 16 taps
        D = G.LDS_EDGE[dt, pp]
        assert reg(D, 16, t, pp) == G.SPAN and reg(D + 1, 16, t, pp) == G.GATHER
        assert torchfx_ext.delay_tiling_info(2, 100, D, 16, t, pp)["lds_bytes"] == 65536
        # taps = 8 / 9 at a span past four tiles: the ring holds 8
        assert reg(600, 8, t, pp) == G.LATTICE and reg(600, 9, t, pp) == (G.GATHER if (dt, pp) == ("f64", True) else G.SPAN)
        # S = 4 tiles: 512 x 8 is the last span, 513 x 8 the first lattice (float64 pairs: 4096 samples do not fit)
        assert reg(512, 8, t, pp) == (G.LATTICE if (dt, pp) == ("f64", True) else G.SPAN) and reg(513, 8, t, pp) == G.LATTICE
        # D = 256: below it, taps <= 8 gives S <= 2040, which is span in every variant -- the edge is only seen above 8 taps
        assert reg(255, 8, t, pp) == reg(256, 8, t, pp) == G.SPAN
        assert reg(0, 3, t, pp) == G.SPAN


def test_tiling_query():
    """tfx_delay_tiling_info: the checks of tfx_delay_forward that need no pointer, the regime of tfx_delay_plan_info, the
    chunking of the full-size workload, and null outputs refused."""
    from torchfx_amd import _lib as L
    from torchfx_amd import torchfx_ext
    q = torchfx_ext.delay_tiling_info
    T = 60 * 48000
    steps = -(-(T + 8 * 12000) // 12000)
    assert q(64, T, 12000, 8) == dict(regime="lattice", units=64, tiles=47, kc=128, nchunks=-(-steps // 128), groups=47 * 2,
                                      nwg=64 * 47 * 2, lds_bytes=0)
    assert q(64, T, 12000, 8, torch.float32, True) == dict(regime="lattice", units=32, tiles=47, kc=64, nchunks=4, groups=47 * 4,
                                                           nwg=32 * 47 * 4, lds_bytes=0)
    assert q(2, 2053, 37, 4) == dict(regime="span", units=2, tiles=3, kc=0, nchunks=0, groups=3, nwg=6, lds_bytes=(148 + 1024) * 4)
    assert q(4, 2053, 37, 4, torch.float64, True)["lds_bytes"] == 2 * (148 + 1024) * 8
    assert q(4, 2053, 100, 200, torch.float32, True) == dict(regime="gather", units=4, tiles=22, kc=0, nchunks=0, groups=22, nwg=88,
                                                             lds_bytes=0)
    assert q(0, 100, 37, 4)["nwg"] == 0 and q(2, 0, 0, 3)["nwg"] == 0
    for bad in ((3, 10, 5, 2, torch.float32, True), (2, 10, 5, 0), (2, 10, -1, 2), (-2, 10, 5, 2), (2, -1, 5, 2), (2, 4, 1 << 62, 4)):
        with pytest.raises(RuntimeError, match="delay_tiling_info"):
            q(*bad)
    lib = L.load()
    k, o = ctypes.c_int(), ctypes.c_int64()
    assert lib.tfx_delay_tiling_info(2, 10, 5, 2, 0, 0, ctypes.byref(k), *[ctypes.byref(o)] * 7) == 0
    assert lib.tfx_delay_tiling_info(2, 10, 5, 2, 0, 0, None, *[ctypes.byref(o)] * 7) != 0
    assert b"delay_tiling_info" in lib.tfx_last_error()
    assert lib.tfx_delay_tiling_info(2, 10, 5, 2, 7, 0, ctypes.byref(k), *[ctypes.byref(o)] * 7) != 0
