"""GPU parity -- the direct FIR at its edges: where a NaN / Inf sample may come out (one-shot, streamed, fused chunk), a
per-sample error bound on signals with quiet stretches, the float64 kernel's tap chunks, the MFMA kernel's tile map,
the shipped dispatch boundary, 4-byte-aligned inputs and exact impulse responses.

References and the derived tolerance: tests/fir_reference.py.  The case builders below are plain numpy and are imported
by tests/test_fir_reference_host.py, which shows on the CPU that the oracle meets every condition asserted here.

Contract ("Non-finite samples in the direct FIR"): a non-finite sample at p reaches exactly the K outputs
p .. p+K-1 of its row on every direct route; zero-valued taps count."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests.fir_reference import bound, reach_mask, ref64, staircase
from tests.gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

KS = [1, 2, 31, 33, 64, 127, 128, 129, 512, 513, 1024, 1025, 2500]
KCS = [None, 128, 512, 1024]
BADS = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
T_REACH = 3 * 4096 + 77
DT = {"f32": np.float32, "f64": np.float64}


# ---------------------------------------------------------------------------------------------- case builders (numpy only)
def positions(K, T=T_REACH):
    raw = [0, 1, 31, 32, K - 2, K - 1, 1023, 1024, 4095, 4096, 4096 + 31, 8191, T - K, T - 2, T - 1]
    out = []
    for p in raw:
        p = min(max(p, 0), T - 1)
        if p not in out:
            out.append(p)
    return out


def make_taps(K, seed, dtype=np.float32, zero_ends=False):
    kf = (np.random.default_rng(seed).standard_normal(K) / np.sqrt(K)).astype(dtype)
    if zero_ends:                       # a Hann-windowed design: first and last two taps exactly 0.0
        kf[:2] = 0.0
        kf[-2:] = 0.0
    return kf


@lru_cache(maxsize=None)
def reach_clean(K, dt, zero_ends=False, T=T_REACH):
    """One row per bad position (the sample there set to 0) plus a last, clean row; taps; the float64 reference and the
    bound of that finite signal."""
    pos = positions(K, T)
    x0 = rnd((len(pos) + 1, T), 31 * K + 7, DT[dt])
    bad = [(r, p) for r, p in enumerate(pos)]
    for r, p in bad:
        x0[r, p] = 0.0
    kf = make_taps(K, 5 * K + 1, DT[dt], zero_ends)
    return dict(x0=x0, kf=kf, bad=bad, ref0=ref64(x0, kf, wide=dt == "f64"), bnd=bound(x0, kf))


@lru_cache(maxsize=None)
def reach_case(K, bad, dt, zero_ends=False):
    c = dict(reach_clean(K, dt, zero_ends))
    x = c["x0"].copy()
    for r, p in c["bad"]:
        x[r, p] = BADS[bad]
    c.update(x=x, ref=ref64(x, c["kf"]), mask=reach_mask(x.shape[0], x.shape[1], K, c["bad"]))
    return c


STREAM_CASES = [(129, (5000, 4096, 60, 50, 7000, 300)), (1024, (4097, 700, 300, 4096, 5000))]


@lru_cache(maxsize=None)
def stream_case(K, chunks, bad):
    """Rows 0..3: the bad sample on the last sample of chunk 0 (it enters the history), the first of chunk 1, inside chunk 2
    and chunk 1's middle -- chunks 2 (and 3, or 1 and 2) are shorter than K-1: the history shifts through; row 4 clean."""
    assert min(chunks[1:3]) < K - 1
    T = sum(chunks)
    o1, o2 = chunks[0], chunks[0] + chunks[1]
    pos = [o1 - 1, o1, o2 + chunks[2] // 2, o1 + chunks[1] // 2]
    x = rnd((len(pos) + 1, T), K + T)
    badl = [(r, p) for r, p in enumerate(pos)]
    for r, p in badl:
        x[r, p] = BADS[bad]
    kf = make_taps(K, 3 * K + 2)
    return dict(x=x, kf=kf, bad=badl, ref=ref64(x, kf), mask=reach_mask(x.shape[0], T, K, badl))


CHUNK_TAPS = [33, 34, 35, 36, 129, 1024]
CHUNK_T = [511, 512, 1000]
CHUNK_EPI = [(None, False), (1.7, True)]


def chunk_positions(T):
    return [0, 1, 2, 3, T - 4, T - 3, T - 2, T - 1, T // 2]


def epilogue64(v, gain, clamp):
    with np.errstate(all="ignore"):
        if gain is not None:
            v = v * np.float64(np.float32(gain))
        return np.clip(v, -1.0, 1.0) if clamp else v          # np.clip keeps NaN and turns +-Inf into +-1


@lru_cache(maxsize=None)
def chunk_case(K, T, bad):
    """Three chunks of T; row r carries one bad sample at chunk position chunk_positions(T)[r] of chunk r % 3; last row clean."""
    q = chunk_positions(T)
    x0 = rnd((len(q) + 1, 3 * T), 17 * K + T)
    badl = [(r, (r % 3) * T + p) for r, p in enumerate(q)]
    x = x0.copy()
    for r, p in badl:
        x0[r, p] = 0.0
        x[r, p] = BADS[bad]
    kf = make_taps(K, 11 * K + 3)
    return dict(x=x, x0=x0, kf=kf, bad=badl, ref=ref64(x, kf), ref0=ref64(x0, kf), bnd=bound(x0, kf),
                mask=reach_mask(x.shape[0], 3 * T, K, badl))


STAIR_K = [5, 129, 513, 1024, 1100, 2500]
STAIR_T = [4095, 4096, 4097, 16385, 40000]


def stair_edges(T, row):
    """A step within one sample of every 1024-sample tile edge (1024 m - 1, 1024 m, 1024 m + 1 in turn, the turn shifted per
    row so that the 4096 m edges see all three), and mid-tile steps in every other tile."""
    e = []
    for m in range(1, T // 1024 + 2):
        e.append(1024 * m + (m + row) % 3 - 1)
        if m % 2:
            e.append(1024 * m - 507)
    return e


@lru_cache(maxsize=None)
def stair_case(K, T, dt):
    x = np.vstack([staircase(1, T, 1000 * K + T + r, stair_edges(T, r), DT[dt]) for r in range(3)])
    kf = make_taps(K, 7 * K + 5, DT[dt])
    return dict(x=x, kf=kf, ref=ref64(x, kf, wide=dt == "f64"), bnd=bound(x, kf))


STAIR_STREAM = [(129, 1000), (129, 5000), (1024, 1000), (1024, 5000)]


@lru_cache(maxsize=None)
def stair_stream_case(K, T, quiet_hist):
    """A history 2^-30 below the chunk it precedes, or the reverse."""
    g = np.random.default_rng(K + T)
    a, b = (2.0 ** -30, 1.0) if quiet_hist else (1.0, 2.0 ** -30)
    hist = (g.standard_normal((2, K - 1)) * a).astype(np.float32)
    x = (g.standard_normal((2, T)) * b).astype(np.float32)
    kf = make_taps(K, 13 * K)
    return dict(x=x, hist=hist, kf=kf, ref=ref64(x, kf, hist), bnd=bound(x, kf, hist))


F64_GRID = [(2, 1023, 513), (3, 1025, 1025), (1, 5000, 2500), (2, 2049, 512), (1, 300, 700)]
TILE_MAP = [(37, 3 * 4096 + 5), (9, 4096), (8, 4097), (1, 9 * 4096), (13, 7 * 4096 - 1)]
DISPATCH = [(2049, 1024), (2048, 1024), (1, 2048 * 1024 + 1), (3, 4095), (600, 4096)]
K_TILE_MAP, K_DISPATCH = 129, 33


@lru_cache(maxsize=None)
def noise_case(C, T, K, dt):
    """Every row its own seed."""
    x = np.vstack([rnd((1, T), 100003 * r + T + K, DT[dt]) for r in range(C)]) if C <= 64 else rnd((C, T), C + T + K, DT[dt])
    kf = make_taps(K, 9 * K + C, DT[dt])
    return dict(x=x, kf=kf, ref=ref64(x, kf, wide=dt == "f64"), bnd=bound(x, kf))


def impulse_case(K, T=T_REACH):
    pos = positions(K, T)
    x = np.zeros((len(pos), T), np.float32)
    for r, p in enumerate(pos):
        x[r, p] = 1.0
    return x, make_taps(K, 5 * K + 1), pos


# ---------------------------------------------------------------------------------------------- assertions
def spans(m):
    """First and last true index per row (what a failure message shows)."""
    return {r: (int(np.flatnonzero(row)[0]), int(np.flatnonzero(row)[-1])) for r, row in enumerate(m) if row.any()}


def check_maps(y, ref, mask, what):
    y = np.asarray(y)
    assert y.shape == ref.shape
    nf = ~np.isfinite(y)
    if mask is not None:
        assert np.array_equal(nf, mask), f"{what}: non-finite outputs per row {spans(nf)}, reach {spans(mask)}"
    assert np.array_equal(np.isnan(y), np.isnan(ref)), f"{what}: NaN outputs per row {spans(np.isnan(y))}, reference {spans(np.isnan(ref))}"
    assert np.array_equal(np.isinf(y), np.isinf(ref)), f"{what}: Inf outputs per row {spans(np.isinf(y))}, reference {spans(np.isinf(ref))}"
    inf = np.isinf(ref)
    assert np.array_equal(y[inf] > 0, ref[inf] > 0), f"{what}: sign of Inf"


def check_bound(y, ref, bnd, what, where=None):
    """|y - ref| <= bnd on every element (of `where`)."""
    err = np.abs(np.asarray(y).astype(ref.dtype) - ref).astype(np.float64)
    ok = err <= bnd
    if where is not None:
        ok = ok | ~where
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, 0.0, err / bnd)), err.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} outputs outside the bound; worst at {i}: err {err[i]:.3e}, bound {bnd[i]:.3e}, ref {float(ref[i]):.3e}")


def set_kc(monkeypatch, kc):
    if kc is not None:
        monkeypatch.setenv("TFX_FIR_KC", str(kc))
        monkeypatch.setenv("TFX_FIR_MFMA_MIN_T", "0")      # short rows and small launches too go through the MFMA kernel here
        monkeypatch.setenv("TFX_FIR_ONE_ROUND_TILES", "0")


def direct(x, kf):
    return ext().fir_direct_forward(dev(x), kf).cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------- 1. reach, one-shot
def reach_one_shot(c, what):
    y = direct(c["x"], c["kf"])
    check_maps(y, c["ref"], c["mask"], what)
    y0 = direct(c["x0"], c["kf"])
    assert np.array_equal(bits(y[-1]), bits(y0[-1])), f"{what}: the clean row depends on its neighbours"
    check_bound(y, c["ref0"], c["bnd"], what, where=~c["mask"])


@pytest.mark.parametrize("bad", list(BADS))
@pytest.mark.parametrize("kc", KCS)
@pytest.mark.parametrize("K", KS)
def test_reach_one_shot_f32(K, kc, bad, monkeypatch):
    """One bad sample per row: NaN and Inf maps equal the float64 direct form's, the non-finite outputs are exactly
    [p, p+K), the clean row keeps its bits, every finite output stays inside the bound."""
    set_kc(monkeypatch, kc)
    reach_one_shot(reach_case(K, bad, "f32"), f"K={K} kc={kc} {bad}")


@pytest.mark.parametrize("bad", list(BADS))
@pytest.mark.parametrize("K", KS)
def test_reach_one_shot_f64(K, bad):
    reach_one_shot(reach_case(K, bad, "f64"), f"f64 K={K} {bad}")


@pytest.mark.parametrize("bad", list(BADS))
@pytest.mark.parametrize("kc", KCS)
def test_reach_counts_zero_valued_taps(kc, bad, monkeypatch):
    """First and last two taps exactly 0.0: the reference multiplies every tap (0 * NaN = 0 * Inf = NaN), so the reach is
    still K -- taps may not be skipped by value."""
    set_kc(monkeypatch, kc)
    reach_one_shot(reach_case(129, bad, "f32", True), f"zero end taps kc={kc} {bad}")


# ---------------------------------------------------------------------------------------------- 2. reach, streaming
@pytest.mark.parametrize("bad", list(BADS))
@pytest.mark.parametrize("K,chunks", STREAM_CASES)
def test_reach_streaming(K, chunks, bad, fir_kernel):
    c = stream_case(K, chunks, bad)
    x, kf = c["x"], c["kf"]
    C = x.shape[0]
    hist, outs, off = None, [], 0
    for n in chunks:
        y, hist = ext().fir_stream_forward(dev(x[:, off:off + n]), kf, hist, True)
        off += n
        seen = np.concatenate([np.zeros((C, K - 1), np.float32), x[:, :off]], axis=1)[:, -(K - 1):]
        assert np.array_equal(bits(hist.cpu().numpy()), bits(seen)), f"history after {off} samples"     # bad sample bit-for-bit
        outs.append(y.cpu().numpy())
    ys = np.concatenate(outs, axis=1)
    what = f"K={K} {bad} {fir_kernel}"
    check_maps(ys, c["ref"], c["mask"], "streamed " + what)
    check_maps(direct(x, kf), c["ref"], c["mask"], "one-shot " + what)


# ---------------------------------------------------------------------------------------------- 3. reach, fused chunk
def chunk_run(x, kf, T, gain, clamp):
    xd, hist, outs = dev(x), None, []
    sos = torch.zeros((0, 6), dtype=torch.float64)
    for i in range(3):
        y, _, _, hist = ext().chunk_forward(xd[:, i * T:(i + 1) * T].contiguous(), sos, None, None, torch.from_numpy(kf), hist, gain, clamp)
        outs.append(y.cpu().numpy())
    return np.concatenate(outs, axis=1), hist.cpu().numpy()


@pytest.mark.parametrize("bad", list(BADS))
@pytest.mark.parametrize("gain,clamp", CHUNK_EPI)
@pytest.mark.parametrize("T", CHUNK_T)
@pytest.mark.parametrize("K", CHUNK_TAPS)
def test_reach_fused_chunk(K, T, gain, clamp, bad):
    """chunk_forward with zero sections (a cascade would poison the rest of the row by design): maps after the same gain and
    clamp on the reference; finite outputs within |gain| * bound plus the one rounding of the gain product."""
    c = chunk_case(K, T, bad)
    y, hist = chunk_run(c["x"], c["kf"], T, gain, clamp)
    what = f"chunk K={K} T={T} gain={gain} clamp={clamp} {bad}"
    exp = epilogue64(c["ref"], gain, clamp)
    check_maps(y, exp, c["mask"] if (bad == "nan" or not clamp) else None, what)
    assert np.array_equal(bits(hist), bits(c["x"][:, -(K - 1):])), what + ": history"
    turned = np.isinf(c["ref"]) & np.isfinite(exp)              # the clamp turned +-Inf into +-1: exactly
    assert np.array_equal(y[turned], exp[turned].astype(np.float32)), what + ": clamped Inf"
    g = 1.0 if gain is None else abs(float(np.float32(gain)))
    exp0 = epilogue64(c["ref0"], gain, clamp)                     # (a clamp only shrinks a difference)
    check_bound(y, exp0, g * c["bnd"] * (1 + 2.0 ** -23) + 2.0 ** -24 * np.abs(g * c["ref0"]), what, where=~c["mask"])


# ---------------------------------------------------------------------------------------------- 4. per-sample bound
def bound_and_close(y, c, tol, what):
    check_bound(y, c["ref"], c["bnd"], what)
    close(y, c["ref"].astype(y.dtype), tol, what)


@pytest.mark.parametrize("T", STAIR_T)
@pytest.mark.parametrize("K", STAIR_K)
def test_staircase_bound_f32(K, T, fir_kernel):
    """Amplitude steps of 2^-10 down to 2^-30 and back at tile edges and mid-tile: every output within the forward error
    bound of a K-term float32 sum -- a wrong or missing term in a quiet stretch is far outside it."""
    c = stair_case(K, T, "f32")
    bound_and_close(direct(c["x"], c["kf"]), c, TOL_CONV_F32, f"staircase K={K} T={T} {fir_kernel}")


@pytest.mark.parametrize("kc", KCS[1:])
@pytest.mark.parametrize("T", STAIR_T)
@pytest.mark.parametrize("K", STAIR_K)
def test_staircase_bound_every_tap_chunk(K, T, kc, monkeypatch):
    set_kc(monkeypatch, kc)
    c = stair_case(K, T, "f32")
    bound_and_close(direct(c["x"], c["kf"]), c, TOL_CONV_F32, f"staircase K={K} T={T} kc={kc}")


@pytest.mark.parametrize("T", STAIR_T)
@pytest.mark.parametrize("K", STAIR_K)
def test_staircase_bound_f64(K, T):
    c = stair_case(K, T, "f64")
    bound_and_close(direct(c["x"], c["kf"]), c, TOL_CONV_F64, f"staircase f64 K={K} T={T}")


@pytest.mark.parametrize("quiet_hist", [True, False])
@pytest.mark.parametrize("K,T", STAIR_STREAM)
def test_staircase_bound_streaming(K, T, quiet_hist, fir_kernel):
    c = stair_stream_case(K, T, quiet_hist)
    y, _ = ext().fir_stream_forward(dev(c["x"]), c["kf"], dev(c["hist"]), True)
    bound_and_close(y.cpu().numpy(), c, TOL_CONV_F32, f"stream K={K} T={T} quiet_hist={quiet_hist} {fir_kernel}")


# ---------------------------------------------------------------------------------------------- 5. float64 kernel grid
@pytest.mark.parametrize("C,T,K", F64_GRID)
def test_f64_direct_grid(C, T, K):
    """The float64 kernel's tap-chunk loop (512 taps per chunk) and rows that cross its 1024-sample tiles with long taps."""
    c = noise_case(C, T, K, "f64")
    bound_and_close(direct(c["x"], c["kf"]), c, TOL_CONV_F64, f"f64 C={C} T={T} K={K}")


# ---------------------------------------------------------------------------------------------- 6. tile map, dispatch
@pytest.mark.parametrize("C,T", TILE_MAP)
def test_mfma_tile_to_workgroup_map(C, T, monkeypatch):
    """The MFMA kernel's tile swizzle over the eight XCDs with tile counts that are and are not multiples of 8."""
    monkeypatch.setenv("TFX_FIR_MFMA_MIN_T", "0")
    monkeypatch.setenv("TFX_FIR_ONE_ROUND_TILES", "0")
    c = noise_case(C, T, K_TILE_MAP, "f32")
    bound_and_close(direct(c["x"], c["kf"]), c, TOL_CONV_F32, f"tile map C={C} T={T}")


@pytest.mark.parametrize("C,T", DISPATCH)
def test_default_dispatch_boundary(C, T):
    """No knob set: both sides of the one-round tile count and of the shortest MFMA row, as shipped."""
    c = noise_case(C, T, K_DISPATCH, "f32")
    bound_and_close(direct(c["x"], c["kf"]), c, TOL_CONV_F32, f"dispatch C={C} T={T}")


# ---------------------------------------------------------------------------------------------- 7. alignment
@pytest.mark.parametrize("o", [1, 2, 3, 5])
def test_four_byte_aligned_rows(o, fir_kernel):
    C, T, K = 3, 2 * 4096 + 5, 129
    kf = make_taps(K, 77)
    flat = dev(rnd((C * T + 8,), o))
    x = flat[o:o + C * T].view(C, T)
    assert x.is_contiguous() and x.data_ptr() % 16 == (4 * o) % 16          # 4-byte aligned, not 16
    assert torch.equal(ext().fir_direct_forward(x, kf), ext().fir_direct_forward(x.clone(), kf))


def test_column_window_input(fir_kernel):
    C, T, K = 3, 2 * 4096 + 5, 129
    kf = make_taps(K, 78)
    big = dev(rnd((C, T + 9), 5))
    x = big[:, 3:3 + T]
    assert torch.equal(ext().fir_direct_forward(x, kf), ext().fir_direct_forward(x.clone(), kf))


# ---------------------------------------------------------------------------------------------- 8. impulses
def check_impulse(y, kf, pos, what):
    K, T = len(kf), y.shape[1]
    for r, p in enumerate(pos):
        n = min(K, T - p)
        assert np.array_equal(bits(y[r, p:p + n]), bits(kf[::-1][:n])), f"{what}: response to the impulse at {p}"
        rest = np.concatenate([y[r, :p], y[r, p + n:]])
        assert np.array_equal(rest, np.zeros_like(rest)), f"{what}: non-zero output outside [{p}, {p + n})"      # +-0.0


@pytest.mark.parametrize("kc", KCS)
@pytest.mark.parametrize("K", KS)
def test_impulse_response_is_the_taps(K, kc, monkeypatch):
    """x = delta[n - p]: every product but one is an exact zero, so the outputs are the unflipped taps bit for bit."""
    set_kc(monkeypatch, kc)
    x, kf, pos = impulse_case(K)
    check_impulse(direct(x, kf), kf, pos, f"K={K} kc={kc}")


@pytest.mark.parametrize("T", CHUNK_T)
@pytest.mark.parametrize("K", CHUNK_TAPS)
def test_impulse_response_fused_chunk(K, T):
    x, kf, pos = impulse_case(K, 3 * T)
    y, _ = chunk_run(x, kf, T, None, False)
    check_impulse(y, kf, pos, f"chunk K={K} T={T}")
