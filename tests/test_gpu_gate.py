"""The gate on the device (csrc/gate.hip through torchfx_ext.gate_forward) against the per-sample loop of tests/gate_reference.py.
Shapes come from the kernel's work unit -- 8 samples a lane, 512 a wave, 2048 a tile, whole tiles a segment -- never from the
workload; at most 8 rows.  The open track and the (open, c) of the state are exact; the gain, the outputs and the state's g stay
within gate_reference.within's bounds (the derived 8 u min(T, 1 / (1 - max(aA, aR))) against the long-double twin).  The same
holds between different `segments` and between chunked and one-shot runs."""
import math

import numpy as np
import pytest
import torch

from tests import gate_reference as R
from tests.gpu_common import DEV, dev, ext

pytestmark = pytest.mark.gpu

FS = 48000
TILE = 2048
T_SEAMS = 3 * TILE + 5
DTYPES = {"f32": np.float32, "f64": np.float64}
_REF: dict = {}
WORST = {"f32": 0.0, "f64": 0.0}


def run(x, K, channels=1, state=None, segments=0):
    """The low-level op on a device copy of ``x [groups * channels, T]`` (or ``[B, C, T]``) -> NumPy ``dict(y, g, open, state)``."""
    st = None if state is None else dev(np.asarray(state, dtype=np.float64))
    y, g, o, s = ext().gate_forward(dev(x), K["p_open"], K["p_close"], K["r"], K["H"], K["aA"], K["aR"], channels, st, True, True,
                                    segments)
    torch.cuda.synchronize()
    return dict(y=y.cpu().numpy(), g=g.cpu().numpy(), open=o.cpu().numpy(), state=s.cpu().numpy())


def reference(name, x, K, channels, state=None):
    """``gate_ref`` on ``x`` in groups of ``channels`` rows, computed once per ``name``."""
    if name not in _REF:
        _REF[name] = R.gate_ref(x.reshape(-1, channels, x.shape[-1]), K, True, state)
    return _REF[name]


def check(what, got, ref, x, K, T_total=None):
    frac = R.within(got, ref, x, K, x.shape[-1] if T_total is None else T_total, what)
    key = "f32" if got["y"].dtype == np.float32 else "f64"
    WORST[key] = max(WORST[key], frac)
    print(f"{what} [{key}]: gain error {frac:.3e} of its bound")


def same_bits(a, b, what=""):
    for k in ("y", "g", "open", "state"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def runs_signal(K, rows, T, seed, dtype, channels=2):
    """Rows of alternating stretches -- loud (above ``p_open``), between the levels, quiet (below ``p_close``) -- whose lengths
    scatter around ``H`` (from 1 to ``2 H + 3``), so that holds end before, at and after ``H`` anywhere in the row; every row
    starts with a few quiet samples.  ``channels`` consecutive rows share the stretches (not the samples), so that a linked
    group sees them too."""
    rng = np.random.default_rng(seed)
    H = K["H"]
    x = np.empty((rows, T))
    mid = 0.5 * (K["p_open"] + K["p_close"])
    for r in range(0, rows, channels):
        c = min(channels, rows - r)
        n, kind = int(rng.integers(0, 4)), 0
        x[r:r + c, :n] = 0.25 * K["p_close"]
        while n < T:
            m = int(rng.integers(1, 2 * H + 4)) if kind == 0 else int(rng.integers(1, 12))
            amp = (rng.uniform(0.0, 0.9, (c, m)) * K["p_close"], np.full((c, m), mid), rng.uniform(1.5, 3.0, (c, m)) * K["p_open"])[kind]
            x[r:r + c, n:n + m] = (amp * rng.choice([-1.0, 1.0], (c, m)))[:, :T - n]
            n += m
            kind = int(rng.choice([0, 0, 1, 2])) if kind else int(rng.choice([1, 2, 2]))
    return x.astype(dtype)


def planted(K, T, starts_lengths, dtype, seed=0):
    """One row per entry of ``starts_lengths`` (a list of ``[(start, length), ..]``): loud everywhere but for the quiet runs."""
    rng = np.random.default_rng(seed)
    return np.concatenate([R.phrases(rng, (1, T), K, sl, dtype) for sl in starts_lengths], 0)


# ---- every size at which the kernel takes another path ------------------------------------------------------------------------

@pytest.mark.parametrize("link", [True, False], ids=["linked", "unlinked"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("T", [1, 7, 8, 9, 2047, 2048, 2049, T_SEAMS])
def test_sizes_against_the_loop(T, dt, link):
    K = R.constants(FS, hold=3 / FS if T < 100 else 40 / FS, attack=0.2e-3, release=2e-3, range_db=30.0)
    assert K["H"] == (3 if T < 100 else 40)
    x = runs_signal(K, 4, T, 100 + T, DTYPES[dt])                      # [B = 2, C = 2, T]
    channels = 2 if link else 1
    ref = reference(("sizes", T, dt, link), x, K, channels)
    if T > 100:
        assert 0.1 < ref["open"].mean() < 0.9
    check(f"T={T} link={link}", run(x, K, channels), ref, x, K)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_segments_agree_with_each_other_and_the_loop(dt):
    K = R.constants(FS, hold=700 / FS, attack=1e-3, release=100e-3)
    x = runs_signal(K, 4, T_SEAMS, 7, DTYPES[dt])
    ref = reference(("segments", dt), x, K, 2)
    assert 0.1 < ref["open"].mean() < 0.9
    got = {}
    for s in (1, 2, 3, 4):
        assert ext().gate_plan_info(T_SEAMS, 2, 2, s)["segments"] == s
        got[s] = run(x, K, 2, segments=s)
        check(f"segments={s}", got[s], ref, x, K)
        assert np.array_equal(got[s]["open"], got[1]["open"]) and np.array_equal(got[s]["state"][:, 1:], got[1]["state"][:, 1:])
    assert ext().gate_plan_info(T_SEAMS, 2, 2)["segments"] == 4
    same_bits(run(x, K, 2), got[4], "the plan's own choice")


# ---- the hold counter across every seam ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("H", [5, 300])
def test_hold_counter_straddles_lane_wave_tile_and_segment_seams(H, dt):
    """Quiet runs of H - 1, H and H + 1 samples (and H + 2) placed so that the sample at which a run of H + 1 closes the gate is
    the last of a lane / wave / tile / segment, the first of the next, and the one after; the shorter runs end there open."""
    K = R.constants(FS, hold=H / FS, attack=0.0, release=1e-3, range_db=40.0)
    assert K["H"] == H
    seams = [b for b in (8, 512, TILE, 2 * TILE) if b - H - 2 >= 1]    # 2 * TILE: between the segments of segments = 2
    rows = [[(b - 1 - H, H + 1) for b in seams], [(b - H, H + 1) for b in seams], [(b + 1 - H, H + 1) for b in seams],
            [(b - H + 1, H) for b in seams], [(b - H + 1, H - 1) for b in seams], [(b - H - 1, H + 2) for b in seams]]
    x = planted(K, T_SEAMS, rows, DTYPES[dt])
    ref = reference(("straddle", H, dt), x, K, 1)
    for k, d in enumerate((-1, 0, 1)):                                 # the reference closes exactly there, for one sample or two
        for b in seams:
            assert ref["open"][k, b + d - 1] == 1 and ref["open"][k, b + d] == 0 and ref["open"][k, b + d + 1] == 1
    assert ref["open"][3:5].all() and not ref["open"][5].all()
    for s in (1, 2, 4):
        check(f"H={H} segments={s}", run(x, K, 1, segments=s), ref, x, K)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_hold_of_zero_samples(dt):
    K = R.constants(FS, hold=0.0, attack=0.1e-3, release=0.5e-3, range_db=12.0)
    assert K["H"] == 0
    x = runs_signal(dict(K, H=3), 4, T_SEAMS, 11, DTYPES[dt])
    ref = reference(("hold0", dt), x, K, 2)
    assert 0.1 < ref["open"].mean() < 0.9
    for s in (1, 4):
        check(f"H=0 segments={s}", run(x, K, 2, segments=s), ref, x, K)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_hold_longer_than_a_whole_segment(dt):
    """H = 2500 > 2048: whole segments are all quiet and only lengthen the count (the summary's all-quiet path).  Triggers in the
    first and in the last sample of a segment; a closed row; a holding sample between the levels at a segment's first sample."""
    H = 2500
    K = R.constants(FS, hold=H / FS, attack=0.0, release=5e-3)
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.5, 0.5, (5, T_SEAMS)) * K["p_close"]
    loud, mid = 2.0 * K["p_open"], 0.5 * (K["p_open"] + K["p_close"])
    x[0, 0], x[0, TILE] = loud, -loud                                  # re-triggered at a segment's first sample: closes at 2048 + 2501
    x[1, 2 * TILE - 1] = loud                                          # opened by a segment's last sample: still open at the end
    x[2, 0] = loud                                                     # closes at 2501, inside the second tile
    x[3, 100], x[3, TILE] = loud, mid                                  # the hold restarts at a segment's first sample
    x = x.astype(DTYPES[dt])                                           # row 4 never opens
    ref = reference(("longhold", dt), x, K, 1)
    assert ref["open"][0].sum() == TILE + H + 1 and ref["open"][2].sum() == H + 1 and ref["open"][3].sum() == TILE - 100 + H + 1
    assert ref["state"][1, 1:].tolist() == [1.0, T_SEAMS - 2 * TILE] and not ref["open"][4].any()
    for s in (1, 2, 3, 4):
        check(f"H={H} segments={s}", run(x, K, 1, segments=s), ref, x, K)


def test_levels_compare_at_exactly_the_host_doubles():
    K = R.constants(FS, hold=0.0, attack=0.0, release=0.0)
    po, pc = K["p_open"], K["p_close"]
    below = lambda v: np.nextafter(v, 0.0)                             # noqa: E731
    x = np.array([[below(po), po, pc, below(pc), pc, below(po), po, below(pc), -po, -pc, -below(pc)]])
    got = run(x, K)
    assert got["open"][0].tolist() == [0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 0]
    check("levels", got, R.gate_ref(x, K), x, K)


# ---- the exact consequences ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("range_db, r", [(math.inf, 0.0), (20.0, 10.0 ** (-20.0 / 20.0))], ids=["r0", "r0.1"])
def test_hard_gate_is_exact(range_db, r, dt):
    K = R.constants(FS, hold=30 / FS, attack=0.0, release=0.0, range_db=range_db)
    assert K["r"] == r and K["aA"] == 0.0 and K["aR"] == 0.0
    dtype = DTYPES[dt]
    x = runs_signal(K, 4, 2 * TILE + 100, 13, dtype)
    for s in (1, 3):
        got = run(x, K, 2, segments=s)
        op = got["open"].astype(bool)                                  # [2, T]
        assert 0.1 < op.mean() < 0.9 and np.array_equal(got["open"], reference(("hard", range_db, dt), x, K, 2)["open"])
        assert np.array_equal(got["g"], np.where(op, 1.0, r).astype(dtype))
        xg, yg = x.reshape(2, 2, -1), got["y"].reshape(2, 2, -1)
        opb = np.broadcast_to(op[:, None, :], xg.shape)
        assert np.array_equal(yg[opb], xg[opb])
        assert np.array_equal(yg[~opb], (r * xg[~opb].astype(np.float64)).astype(dtype))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_always_open_group_comes_back_bit_identical(dt):
    K = R.constants(FS, hold=400 / FS, attack=0.0, release=50e-3)
    rng = np.random.default_rng(17)
    x = R.phrases(rng, (4, T_SEAMS), K, [(300, 400), (TILE - 200, 400), (2 * TILE - 1, 399)], DTYPES[dt])    # H samples do not close
    for s in (1, 3):
        got = run(x, K, 2, segments=s)
        assert got["open"].all() and np.array_equal(got["y"], x) and np.array_equal(got["g"], np.ones((2, T_SEAMS), DTYPES[dt]))
        assert np.array_equal(got["state"], np.array([[1.0, 1.0, 0.0]] * 2))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_groups_bits_do_not_depend_on_the_other_groups(dt):
    K = R.constants(FS, hold=60 / FS, range_db=18.0)
    x = runs_signal(K, 8, T_SEAMS, 19, DTYPES[dt])                     # 4 groups of 2 channels
    for s in (0, 2):
        whole = run(x, K, 2, segments=s)
        alone = run(x[4:6], K, 2, segments=s)
        same_bits({k: v[2:3] if k != "y" else v[4:6] for k, v in whole.items()}, alone, f"alone, segments={s}")
        back = run(x.reshape(4, 2, -1)[::-1].reshape(8, -1), K, 2, segments=s)
        same_bits({k: (v[::-1] if k != "y" else v.reshape(4, 2, -1)[::-1].reshape(8, -1)) for k, v in back.items()}, whole,
                  f"reversed, segments={s}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_non_finite_samples_poison_their_group_from_there_on(dt):
    """NaN and Inf at a tile's last and first sample (2047, 2048; with 4 segments those are a segment's, too)."""
    K = R.constants(FS, hold=60 / FS, attack=0.0, release=0.0, range_db=18.0)       # a = 0: the NaN must carry through 0 * NaN
    x = runs_signal(K, 8, T_SEAMS, 23, DTYPES[dt])                     # 4 groups of 2 channels
    K2 = R.constants(FS, hold=60 / FS, range_db=18.0)
    for KK in (K, K2):
        clean = {s: run(x, KK, 2, segments=s) for s in (1, 4)}
        for bad, at in ((np.nan, TILE - 1), (np.inf, TILE), (-np.inf, TILE - 1), (np.nan, TILE)):
            z = x.copy()
            z[3, at] = bad                                             # group 1, its second channel
            ref = R.gate_ref(z.reshape(4, 2, -1), KK)
            for s in (1, 4):
                got = run(z, KK, 2, segments=s)
                check(f"poison {bad} at {at} segments={s}", got, ref, z, KK)
                for k in ("g", "open", "state"):
                    assert np.array_equal(got[k][[0, 2, 3]], clean[s][k][[0, 2, 3]]), k
                assert np.array_equal(got["y"][[0, 1, 4, 5, 6, 7]], clean[s]["y"][[0, 1, 4, 5, 6, 7]])
                assert np.array_equal(got["y"][2:4, :at], clean[s]["y"][2:4, :at]) and np.array_equal(got["g"][1, :at], clean[s]["g"][1, :at])
                assert np.array_equal(got["open"][1, :at], clean[s]["open"][1, :at]) and not got["open"][1, at:].any()
                assert np.isnan(got["y"][2:4, at:]).all() and np.isnan(got["g"][1, at:]).all() and np.isnan(got["state"][1]).all()
    again = run(x[2:4], K2, 2, state=np.full((1, 3), np.nan))          # a poisoned state stays poisoned
    assert np.isnan(again["y"]).all() and not again["open"].any() and np.isnan(again["state"]).all()


# ---- state in and out ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("chunk", [1, 100, 2048, 2049])
def test_chunks_with_the_state_equal_one_shot(chunk, dt):
    T = {1: 300, 100: 2500}.get(chunk, T_SEAMS)
    K = R.constants(FS, hold=70 / FS, attack=0.5e-3, release=10e-3, range_db=26.0)
    x = runs_signal(K, 4, T, 29, DTYPES[dt])
    ref = reference(("chunks", T, dt), x, K, 2)
    st, parts = None, {"y": [], "g": [], "open": []}
    for n0 in range(0, T, chunk):
        got = run(x[:, n0:n0 + chunk], K, 2, state=st)
        st = got["state"]
        for k in parts:
            parts[k].append(got[k])
    whole = dict({k: np.concatenate(v, -1) for k, v in parts.items()}, state=st)
    check(f"chunks of {chunk}", whole, ref, x, K)
    one = run(x, K, 2)
    assert np.array_equal(whole["open"], one["open"]) and np.array_equal(st[:, 1:], one["state"][:, 1:])


def test_start_state_is_the_closed_gate_at_r():
    K = R.constants(FS, hold=20 / FS, range_db=10.0)
    x = runs_signal(K, 2, 700, 31, np.float64)
    x[:, :10] = 0.1 * K["p_close"]
    same_bits(run(x, K, 2), run(x, K, 2, state=[[K["r"], 0.0, 0.0]]))
    ref = R.gate_ref(x.reshape(1, 2, -1), K, state=[[0.7, 1.0, 15.0]])
    check("from an open state", run(x, K, 2, state=[[0.7, 1.0, 15.0]]), ref, x, K)
    assert ref["open"][0, :5].all() and ref["open"][0, 5] == 0         # 15 + 6 > 20: the carried counter closes it


# ---- the public function on the device -----------------------------------------------------------------------------------------

def test_gate_on_the_device_is_the_op_and_keeps_shape_dtype_and_device():
    from torchfx_amd import gate

    kw = dict(threshold_db=-30.0, hysteresis_db=3.0, range_db=20.0, attack=0.3e-3, hold=1e-3, release=4e-3)
    K = R.constants(FS, **kw)
    for dt, dtype in DTYPES.items():
        x = runs_signal(K, 6, TILE + 9, 37, dtype).reshape(3, 2, -1)
        xd = dev(x)
        y, g, o, st = gate(xd, FS, return_gain=True, return_open=True, return_state=True, **kw)
        assert y.shape == xd.shape and y.dtype == xd.dtype and y.device == xd.device
        assert g.shape == (3, TILE + 9) and g.dtype == xd.dtype and o.dtype == torch.uint8 and st.shape == (3, 3)
        low = run(x, K, 2)
        assert np.array_equal(y.cpu().numpy(), low["y"]) and np.array_equal(o.cpu().numpy(), low["open"])
        assert torch.equal(gate(xd, FS, **kw), y) and gate(xd, FS, link=False, return_open=True, **kw)[1].shape == (6, TILE + 9)
        host = gate(torch.from_numpy(x), FS, return_open=True, **kw)[1]
        assert torch.equal(host, o.cpu())                              # the decision is the same on any device
        e = torch.empty(3, 2, 0, dtype=xd.dtype, device=DEV)
        y0, st0 = gate(e, FS, state=st, return_state=True, **kw)
        assert y0.shape == (3, 2, 0) and torch.equal(st0, st)


def test_empty_work_hands_the_state_on():
    K = R.constants(FS, range_db=20.0)
    got = run(np.zeros((4, 0), np.float32), K, 2)
    assert got["y"].shape == (4, 0) and got["open"].shape == (2, 0) and got["state"].tolist() == [[0.1, 0.0, 0.0]] * 2
    got = run(np.zeros((4, 0), np.float32), K, 2, state=[[0.5, 1.0, 9.0], [0.25, 0.0, 0.0]])
    assert got["state"].tolist() == [[0.5, 1.0, 9.0], [0.25, 0.0, 0.0]]


def test_zz_report_the_largest_fraction_of_the_bound():
    print("largest gain error as a fraction of its bound on the device:", {k: f"{v:.3e}" for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
