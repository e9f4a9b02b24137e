"""CPU: the oracle's direct FIR meets every condition tests/test_gpu_fir_edges.py imposes on the HIP kernels, for every
parametrisation used there (the case lists and builders are imported, not restated) -- so those tests cannot fail by
their own construction -- and `ref64` agrees with the oracle, which is pinned to the reference by the golden vectors."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import test_gpu_fir_edges as G
from tests.fir_reference import bound, reach_mask, ref64, staircase
from tests.gpu_common import TOL_CONV_F32, TOL_CONV_F64


def oracle_direct(x, kf, hist=None):
    if hist is None:
        return O.fir_direct(x, kf)
    H = hist.shape[1]
    return O.fir_direct(np.concatenate([hist, x], axis=1), kf)[:, H:]


def finite_case(c, tol, what, hist=None):
    y = oracle_direct(c["x"], c["kf"], hist)
    assert y.dtype == c["x"].dtype
    G.bound_and_close(y, c, tol, what)


def reach_holds(c, what, nonzero=slice(None)):
    assert np.all(c["kf"][nonzero] != 0), what + ": the reach assumes non-zero taps"
    y = O.fir_direct(c["x"], c["kf"])
    G.check_maps(y, c["ref"], c["mask"], what)
    y0 = O.fir_direct(c["x0"], c["kf"])
    assert np.array_equal(G.bits(y[-1]), G.bits(y0[-1]))
    G.check_bound(y, c["ref0"], c["bnd"], what, where=~c["mask"])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("K", G.KS)
def test_oracle_meets_the_one_shot_reach_conditions(K, dt):
    for bad in G.BADS:
        reach_holds(G.reach_case(K, bad, dt), f"{dt} K={K} {bad}")


def test_oracle_reach_counts_zero_valued_taps():
    for bad in G.BADS:
        c = G.reach_case(129, bad, "f32", True)
        assert np.all(c["kf"][:2] == 0) and np.all(c["kf"][-2:] == 0)
        reach_holds(c, f"zero end taps {bad}", slice(2, -2))


@pytest.mark.parametrize("K,chunks", G.STREAM_CASES)
def test_oracle_meets_the_streaming_reach_conditions(K, chunks):
    for bad in G.BADS:
        c = G.stream_case(K, chunks, bad)
        assert np.all(c["kf"] != 0)
        G.check_maps(O.fir_direct(c["x"], c["kf"]), c["ref"], c["mask"], f"K={K} {bad}")
        offs = np.cumsum((0,) + chunks)
        assert any(p == offs[1] - 1 for _, p in c["bad"]) and any(p == offs[1] for _, p in c["bad"])
        assert any(offs[2] <= p < offs[3] for _, p in c["bad"]) and {n < 4096 for n in chunks} == {True, False}


@pytest.mark.parametrize("T", G.CHUNK_T)
@pytest.mark.parametrize("K", G.CHUNK_TAPS)
def test_oracle_meets_the_fused_chunk_conditions(K, T):
    from torchfx_amd import torchfx_ext
    for bad in G.BADS:
        c = G.chunk_case(K, T, bad)
        assert np.all(c["kf"] != 0)
        assert torchfx_ext.chunk_supported(c["x"].shape[0], T, 0, K)
        raw = O.fir_direct(c["x"], c["kf"])
        raw0 = O.fir_direct(c["x0"], c["kf"])
        for gain, clamp in G.CHUNK_EPI:
            what = f"chunk K={K} T={T} gain={gain} clamp={clamp} {bad}"
            with np.errstate(all="ignore"):
                y = raw if gain is None else raw * np.float32(gain)
                y0 = raw0 if gain is None else raw0 * np.float32(gain)
            if clamp:
                y, y0 = np.clip(y, -1.0, 1.0), np.clip(y0, -1.0, 1.0)
            assert y.dtype == np.float32
            exp = G.epilogue64(c["ref"], gain, clamp)
            G.check_maps(y, exp, c["mask"] if (bad == "nan" or not clamp) else None, what)
            turned = np.isinf(c["ref"]) & np.isfinite(exp)
            assert turned.any() == (clamp and bad != "nan")
            assert np.array_equal(y[turned], exp[turned].astype(np.float32))
            g = 1.0 if gain is None else abs(float(np.float32(gain)))
            G.check_bound(y, G.epilogue64(c["ref0"], gain, clamp), g * c["bnd"] * (1 + 2.0 ** -23) + 2.0 ** -24 * np.abs(g * c["ref0"]),
                          what, where=~c["mask"])
    assert sorted({(K - 1) % 4 for K in G.CHUNK_TAPS}) == [0, 1, 2, 3]


@pytest.mark.parametrize("dt,tol", [("f32", TOL_CONV_F32), ("f64", TOL_CONV_F64)])
@pytest.mark.parametrize("T", G.STAIR_T)
@pytest.mark.parametrize("K", G.STAIR_K)
def test_oracle_stays_inside_the_bound_on_staircases(K, T, dt, tol):
    finite_case(G.stair_case(K, T, dt), tol, f"staircase {dt} K={K} T={T}")


@pytest.mark.parametrize("quiet_hist", [True, False])
@pytest.mark.parametrize("K,T", G.STAIR_STREAM)
def test_oracle_stays_inside_the_bound_with_a_history(K, T, quiet_hist):
    c = G.stair_stream_case(K, T, quiet_hist)
    finite_case(c, TOL_CONV_F32, f"stream K={K} T={T}", c["hist"])


@pytest.mark.parametrize("C,T,K,dt,tol", [(C, T, K, "f64", TOL_CONV_F64) for C, T, K in G.F64_GRID] +
                         [(C, T, G.K_TILE_MAP, "f32", TOL_CONV_F32) for C, T in G.TILE_MAP] +
                         [(C, T, G.K_DISPATCH, "f32", TOL_CONV_F32) for C, T in G.DISPATCH])
def test_oracle_stays_inside_the_bound_on_noise(C, T, K, dt, tol):
    finite_case(G.noise_case(C, T, K, dt), tol, f"noise {dt} C={C} T={T} K={K}")


@pytest.mark.parametrize("K", G.KS + G.CHUNK_TAPS)
def test_oracle_impulse_response_is_the_taps(K):
    for T in [G.T_REACH] if K in G.KS else [3 * t for t in G.CHUNK_T]:
        x, kf, pos = G.impulse_case(K, T)
        G.check_impulse(O.fir_direct(x, kf), kf, pos, f"K={K} T={T}")


# ---- the helpers themselves
def test_ref64_is_the_definition():
    g = np.random.default_rng(0)
    x, kf, hist = g.standard_normal((2, 50)), g.standard_normal(7), g.standard_normal((2, 6))
    xp = np.concatenate([hist, x], axis=1)
    exp = np.array([[sum(kf[t] * xp[c, n + t] for t in range(7)) for n in range(50)] for c in range(2)])
    assert np.allclose(ref64(x, kf, hist), exp, rtol=1e-13, atol=1e-13)
    assert np.allclose(ref64(x, kf), ref64(x, kf, np.zeros((2, 6))), rtol=0, atol=0)
    assert ref64(x, kf, hist, wide=True).dtype == np.longdouble
    x[1, 10] = np.inf
    kz = kf.copy()
    kz[3] = 0.0
    y = ref64(x, kz)
    assert np.isnan(y[1, 13]) and np.isinf(y[1, 10:17]).sum() == 6 and np.isfinite(y[0]).all() and np.isfinite(y[1, :10]).all()
    assert np.finfo(np.longdouble).nmant >= 63, "float64 kernels are judged against a wider accumulation"


def test_bound_is_the_stated_formula():
    g = np.random.default_rng(1)
    x, kf = g.standard_normal((1, 40)).astype(np.float32), g.standard_normal(5).astype(np.float32)
    s = np.convolve(np.abs(x[0]).astype(np.float64), np.abs(kf[::-1]).astype(np.float64))[:40]
    u = 2.0 ** -24
    assert np.allclose(bound(x, kf)[0], 6 * u / (1 - 6 * u) * s + 5 * 2.0 ** -126, rtol=1e-12, atol=0)
    u = 2.0 ** -53
    assert np.allclose(bound(x.astype(np.float64), kf)[0], 6 * u / (1 - 6 * u) * s + 5 * 2.0 ** -1022, rtol=1e-12, atol=0)
    assert (bound(np.zeros((1, 8), np.float32), kf) == 5 * 2.0 ** -126).all()


def test_reach_mask_and_staircase():
    m = reach_mask(3, 10, 4, [(0, 0), (1, 8), (2, -2)])
    assert m[0].tolist() == [True] * 4 + [False] * 6
    assert m[1].tolist() == [False] * 8 + [True] * 2
    assert m[2].tolist() == [True] * 2 + [False] * 8
    assert not reach_mask(1, 10, 4, [(0, -4)]).any()
    x = staircase(2, 7000, 3, [1000, 2000, 3000, 4000, 5000, 6000], np.float64)
    rms = [np.sqrt(np.mean(x[:, a:a + 1000] ** 2)) for a in range(0, 7000, 1000)]
    exp = [1.0, 2.0 ** -10, 2.0 ** -20, 2.0 ** -30, 2.0 ** -20, 2.0 ** -10, 1.0]
    assert np.allclose(rms, exp, rtol=0.1)
    assert staircase(1, 10, 0, [5]).dtype == np.float32
