"""The cases of the compressor's edge tests (tests/test_gpu_compressor_edges.py, tests/test_compressor_cases_host.py): the
positions at which the scan of csrc/compressor.hip hands a carry on, signals that plant a maximum or a non-finite sample exactly
there, the parameter corners, the census that says which operand of the release stage's `max` wins at each of those positions,
and the bounds.  NumPy and the host-only plan query: nothing here needs a device.

The scan's levels, for sample `a` of a tile of 2048: thread a // 8 and element a % 8 (a lane's 8 samples), lane (a // 8) % 64
(six Kogge-Stone strides: lane 2^j is the first to receive at stride j), wave a // 512 (four totals through LDS), the tile
carry in registers, and the segment summaries that cross the launches.  At T = 3 * 2048 + 17 and segments = 3 the segments are
tiles 0-1, tile 2 and the short tile 3, so tile 1 is the second tile of a segment.  `geometry` compares this with what
compressor_plan_info says.

The bounds are those of tests/test_gpu_compressor.py (float64 detector for both signal dtypes):
  float64   |20 log10 g - 20 log10 g_ref| <= 1e-10 dB   and   |y - y_ref| <= 1e-11 max|y_ref|
  float32   |y - y_ref| <= 2^-23 |y_ref| + 1e-11 max|y_ref|;   |g - g_ref| <= (2^-24 + 2e-11) g_ref
  state     1e-10 (dB);   the same between two segment counts (there a float32 gain is two roundings: 2^-23 + 2e-11)
and for the static curve alone (`curve_row`), where max|y_ref| would make the output's bound vacuous, per sample:
  |y - y_ref| <= (2u + 1.2e-11) |y_ref|     (u the dtype's unit round-off; 1e-10 dB is 1.15e-11 relative)
"""
import functools
import math

import numpy as np

from tests import compressor_reference as R

FS = 48000
TILE, ELEMS, LANES, WAVES = 2048, 8, 64, 4
WAVE = ELEMS * LANES                            # samples of a tile one wave owns
T_SEAMS = 3 * TILE + 17
SEGMENTS = 3                                    # the cut the positions are made for
T_LONG = 10 * TILE + 5
DTYPES = {"f32": np.float32, "f64": np.float64}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
TH, W = -20.0, 6.0                              # compress()'s default threshold and knee
G_MIN = 2.0 ** -100                             # every case keeps g above this: float32 gains stay normal


def _positions():
    in_tile = [0, 7, 8, 15] + [8 * 2 ** j - 1 for j in range(1, 6)] + [8 * 2 ** j for j in range(1, 6)]
    in_tile += [511, 512, 1023, 1024, 1535, 1536, 2047]
    row = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 3 * TILE - 1, 3 * TILE, T_SEAMS - 1]
    return tuple(sorted({TILE + a for a in in_tile} | set(row)))


P = _positions()                                # one group per position in the packed families
BAD = (np.nan, np.inf, -np.inf)

LN2 = math.log(2.0)
CORNERS = {
    "defaults": {},
    "hold": {"release": 1e300, "attack": 0.0},                         # aR rounds to 1: y1 is the running maximum of v, exactly
    "fast": {"attack": 1.0 / (FS * LN2), "release": 1.0 / (FS * LN2)},  # a = 0.5: a^2048 = 0 in pw[8] and seg[]
    "tiny": {"alphas_": (1e-200, 1e-200)},                              # a^8 = 0 in pw[0]; the low-level op only
    "slow": {"attack": 0.5, "release": 2.0},
    "ratio1": {"ratio": 1.0},                                           # s = 0: v = +0 whatever the level
    "ratio1_makeup": {"ratio": 1.0, "makeup_db": 4.5},
}
LIVE_CORNERS = ("defaults", "hold", "slow")     # where a click's carry outlasts the row and a staircase's never reaches 0
NONFINITE_CORNERS = {"defaults": {}, "instant": {"attack": 0.0, "release": 0.0}, "hold": CORNERS["hold"]}


def ext():
    from torchfx_amd import torchfx_ext
    return torchfx_ext


def geometry():
    """What the plan says about the shapes the cases are made for, compared with what they assume."""
    info = ext().compressor_plan_info(T_SEAMS, len(P), 2, SEGMENTS)
    assert (info["tile"], info["tiles"], info["segments"], info["seg_tiles"]) == (TILE, 4, SEGMENTS, 2), info
    assert TILE == ELEMS * LANES * WAVES
    one = ext().compressor_plan_info(T_SEAMS, len(P), 2, 1)
    assert (one["segments"], one["seg_tiles"], one["scratch_bytes"]) == (1, 4, 0), one
    return info


def long_split(segments):
    """(segments, tiles of the longest segment) the plan takes for the long-segment case."""
    info = ext().compressor_plan_info(T_LONG, 2, 2, segments)
    assert info["tile"] == TILE and info["tiles"] == 11, info
    return info["segments"], info["seg_tiles"]


LONG_SPLITS = {0: (11, 1), 1: (1, 11), 2: (2, 6), 4: (4, 3), 11: (11, 1)}      # 2: 6 + 5 tiles; 4: 3 + 3 + 3 + 2


def reduced(kw):
    """compress()'s keywords -> (th, s, w, alpha_a, alpha_r, makeup) of the low-level op (`alphas_` replaces the coefficients)."""
    import torch

    from torchfx_amd.dynamics import CompressorParams

    kw = dict(kw)
    al = kw.pop("alphas_", None)
    Q = CompressorParams(FS, torch.float32, **kw)
    aa, ar = (Q.alpha_a, Q.alpha_r) if al is None else al
    return Q.th, Q.s, Q.w, aa, ar, Q.makeup


# ---- the signals -----------------------------------------------------------------------------------------------------------

def quiet_floor(rng, shape):
    """|x| <= 0.06, under Th - W/2 = -23 dB (0.0708) for the defaults: v = 0 exactly."""
    return np.clip(rng.standard_normal(shape) * 0.03, -0.06, 0.06)


def loud_floor(rng, shape):
    """Random sign, |x| uniform in [0.1, 0.2] (-20 to -14 dB): v > 0 everywhere, so the B terms of every combine carry weight.
    The magnitudes lie on a grid of 1024 steps, so two different levels differ by 5e-4 relative or more: successive records of
    the running maximum stay apart in a float32 gain (`check_hold` counts them)."""
    return (0.1 + rng.integers(0, 1025, shape) / 10240.0) * rng.choice([-1.0, 1.0], shape)


def _clicks(x):
    for k, n in enumerate(P):
        x[k, k % 2, n] = -1.5
    return x


@functools.lru_cache(maxsize=None)
def family(name, dt):
    """The input ``[groups, 2, T]`` of a planted family in the dtype ``dt`` ("f32" / "f64"), never modified."""
    rng = np.random.default_rng({"click_silent": 101, "click_loud": 102, "staircase": 103, "long": 104}[name])
    if name == "click_silent":
        x = _clicks(quiet_floor(rng, (len(P), 2, T_SEAMS)))
    elif name == "click_loud":
        x = _clicks(loud_floor(rng, (len(P), 2, T_SEAMS)))
    elif name == "staircase":
        x = quiet_floor(rng, (1, 2, T_SEAMS))
        for i, (n, mag) in enumerate(zip(P, np.linspace(0.2, 1.9, len(P)))):
            x[0, :, n] = 0.0
            x[0, (i // 2) % 2, n] = mag * (-1.0) ** i
    elif name == "long":
        x = loud_floor(rng, (2, 2, T_LONG))
        x[0, 1, 100], x[1, 0, 1500] = -1.5, -1.5
        for k in (2, 3, 7, 9):                                         # bursts that end 5 samples before a tile seam ...
            x[..., k * TILE - 300:k * TILE - 5] *= 4.0 + 0.5 * k
        x[..., 5 * TILE - 40:5 * TILE + 60] *= 9.0                     # ... one across a seam inside a segment of both cuts ...
        x[..., 6 * TILE - 40:6 * TILE + 60] *= 8.0                     # ... and one across the seam where 6 + 5 and 3 + 3 + 3 + 2 cut
    else:
        raise KeyError(name)
    x = x.astype(DTYPES[dt])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, corner, dt):
    """``compress_ref`` of a family at a corner, computed once: dict of y, g, state, v, y1 (read-only)."""
    trace = {}
    y, g, st = R.compress_ref(family(name, dt), FS, link=True, trace=trace, **CORNERS[corner])
    out = dict(y=y, g=g, state=st, v=trace["v"], y1=trace["y1"])
    for a in out.values():
        a.setflags(write=False)
    return out


def ref_tuple(ref):
    return ref["y"], ref["g"], ref["state"]


FAMILY_CORNERS = [("click_silent", "defaults"), ("long", "defaults")] + [(f, c) for f in ("click_loud", "staircase") for c in CORNERS]


@functools.lru_cache(maxsize=None)
def nonfinite_input(dt, channels=2):
    """(clean, bad, positions) ``[groups, channels, T]``.  channels = 2: one group per position of P, the bad value cycling
    NaN, +Inf, -Inf and the channel alternating, and two clean groups.  Otherwise one group per channel index that holds the bad
    value (at positions of P in turn) and one clean group."""
    bad_groups = len(P) if channels == 2 else channels
    groups = bad_groups + (2 if channels == 2 else 1)
    rng = np.random.default_rng(300 + channels)
    x = R.bursty(rng, (groups, channels, T_SEAMS), quiet=0.02, loud=0.7, burst=350, gap=650, dtype=DTYPES[dt])
    xb = x.copy()
    pos = np.array(P[:bad_groups] if channels == 2 else [P[(7 * k + 5) % len(P)] for k in range(bad_groups)])
    for k, n in enumerate(pos):
        xb[k, k % channels, n] = BAD[k % 3]
    for a in (x, xb, pos):
        a.setflags(write=False)
    return x, xb, pos


def check_nonfinite(clean, got, pos, what=""):
    """Per group with a bad sample at ``pos[k]``: outputs and gain before it bit-equal to the clean run, outputs, gain and end
    state NaN from it on; the groups behind the bad ones bit-equal in everything.  ``clean`` and ``got`` are (y, g, state)."""
    (yc, gc, sc), (y, g, st) = clean, got
    nb, T = len(pos), y.shape[-1]
    after = np.arange(T)[None, :] >= np.asarray(pos)[:, None]
    for k in range(nb):
        n0 = int(pos[k])
        assert np.array_equal(bits(y[k][:, :n0]), bits(yc[k][:, :n0])) and np.array_equal(bits(g[k][:n0]), bits(gc[k][:n0])), (what, k, n0)
    assert np.isnan(y[:nb][np.broadcast_to(after[:, None, :], y[:nb].shape)]).all(), what
    assert np.isnan(g[:nb][after]).all() and np.isnan(st[:nb]).all(), what
    assert not np.isnan(g[:nb][~after]).any() and not np.isnan(y[:nb][np.broadcast_to(~after[:, None, :], y[:nb].shape)]).any(), what
    for a, b in ((y, yc), (g, gc), (st, sc)):
        assert len(a) > nb and np.array_equal(bits(a[nb:]), bits(b[nb:])), what


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- the census: which operand of the release stage's max wins at a boundary ---------------------------------------------

def boundary_classes(T=T_SEAMS):
    """class name -> positions of the row: the first sample of a lane (not lane 0), of lane 2^j (the first lane that receives
    at Kogge-Stone stride j), of a wave (not wave 0), of a tile inside a segment, of a segment (at SEGMENTS = 3)."""
    n = np.arange(1, T)
    a = n % TILE
    lane = (a // ELEMS) % LANES
    first = a % ELEMS == 0
    out = {"lane": n[first & (lane > 0)], "wave": n[first & (lane == 0) & (a > 0)]}
    for j in range(6):
        out["stride%d" % j] = n[first & (lane == 2 ** j)]
    out["tile"] = np.array([TILE])                                     # tile 1 follows tile 0 inside segment 0 (it > 0)
    out["segment"] = np.array([2 * TILE, 3 * TILE])
    return out


def live(v, y1, state=0.0):
    """[T] bool: the carry decides y1[b] (y1[b-1] > v[b]); dead where v[b] >= y1[b-1]."""
    return np.concatenate([[state], y1[:-1]]) > v


def in_tile_1(n):
    return (n >= TILE) & (n < 2 * TILE)


def running_maximum(v):
    """y1 of the hold corner: the running maximum of v from the silent state 0."""
    return np.maximum.accumulate(np.maximum(v, 0.0), axis=-1)


def check_hold(g, v_ref, what=""):
    """On the device's gain alone (hold corner: b = 0 and every power is 1, nothing rounds): g[n] is bit-equal to g[m], m the
    last record position <= n, and there are as many distinct gains as records (the silent stretch in front of the first record
    counts as one where there is one)."""
    top = running_maximum(v_ref)
    for k in range(len(g)):
        starts = np.concatenate([[0], np.flatnonzero(np.diff(top[k]) != 0) + 1])
        run = np.cumsum(np.concatenate([[0], np.diff(top[k]) != 0]))
        assert np.array_equal(bits(g[k]), bits(g[k][starts][run])), (what, k)
        assert len(np.unique(g[k])) == len(starts), (what, k, len(np.unique(g[k])), len(starts))


# ---- the bounds ----------------------------------------------------------------------------------------------------------

WORST: dict = {}


def check(what, got, ref, dtype, key=None):
    """The module's bounds for ``got = (y, g, state)`` against ``ref``; the largest deviations (gain: dB for float64, relative
    for float32, where it is the rounding of g; the output's excess over the float32 rounding as a fraction of max|y_ref|;
    state) go to WORST[key]."""
    (y, g, st), (yr, gr, sr) = got, ref
    yr = yr.reshape(y.shape)
    top = np.abs(yr).max() if yr.size else 0.0
    if dtype == np.float64:
        dy = np.abs(y - yr).max() / max(top, 1e-300)
        dg = np.abs(20 * np.log10(g) - 20 * np.log10(gr)).max()
        ok = dy <= 1e-11 and dg <= 1e-10
    else:
        err = np.abs(y.astype(np.float64) - yr)
        dy = (err - 2.0 ** -23 * np.abs(yr)).max() / max(top, 1e-300)
        dg = (np.abs(g.astype(np.float64) - gr) / gr).max()
        ok = dy <= 1e-11 and dg <= 2.0 ** -24 + 2e-11
    ds = np.abs(st - sr).max()
    w = WORST.setdefault(key or what, [0.0, -np.inf, 0.0])
    w[0], w[1], w[2] = max(w[0], dg), max(w[1], dy), max(w[2], ds)
    print(f"{what} [{np.dtype(dtype).name}]: dy {dy:.3e}  dg {dg:.3e}  dstate {ds:.3e}")
    assert ok and ds <= 1e-10, (what, dy, dg, ds)


def between(what, a, b, dtype):
    """The same bounds between two results (two float32 outputs are two roundings of products 1e-11 apart: one ulp)."""
    (ya, ga, sa), (yb, gb, sb) = a, b
    ya, yb, ga, gb = (v.astype(np.float64) for v in (ya, yb, ga, gb))
    dy = (np.abs(ya - yb) - (2.0 ** -23 * np.abs(yb) if dtype == np.float32 else 0.0)).max() / np.abs(yb).max()
    dg = np.abs(20 * np.log10(ga) - 20 * np.log10(gb)).max() if dtype == np.float64 else (np.abs(ga - gb) / gb).max()
    ds = np.abs(sa - sb).max()
    print(f"{what}: dy {dy:.3e}  dg {dg:.3e}  dstate {ds:.3e}")
    assert dy <= 1e-11 and dg <= (1e-10 if dtype == np.float64 else 2.0 ** -23 + 2e-11) and ds <= 1e-10, (what, dy, dg, ds)


def report():
    """Prints WORST.  The output's figure is what lies beyond the relative part of its bound (float32: beyond the one rounding
    of the product), 0 where nothing does."""
    for key, (dg, dy, ds) in sorted(WORST.items(), key=lambda kv: str(kv[0])):
        print(f"compressor edges worst {key}: gain {dg:.3e} (f64: dB, f32: relative), y excess {max(dy, 0.0):.3e}, state {ds:.3e}")


# ---- the static curve by itself ---------------------------------------------------------------------------------------------

CURVE_KW = {"attack": 0.0, "release": 0.0}     # g[n] = 10^((makeup - v[n]) / 20): no memory


@functools.lru_cache(maxsize=None)
def curve_row(dt):
    """One row ``[1, 1, N]``: +-0, the smallest denormal, log-spaced magnitudes over the dtype's range (and 300 more from -26 to
    -14 dB, across the knee) with random sign, and for
    each of Th - W/2, Th and Th + W/2 (Th is both edges of the hard knee) the linear level rounded to the dtype with its
    neighbours at 1 and 2 ulps and at 2^-30 and 2^-21 relative (a float64 ulp is 1e-15 dB, under what the bound resolves)."""
    dtype = DTYPES[dt]
    rng = np.random.default_rng(500)
    tiny = np.nextafter(dtype(0), dtype(1))
    lo, hi = (-45.0, math.log10(3e38)) if dtype == np.float32 else (-323.0, 300.0)
    mags = (10.0 ** np.concatenate([np.linspace(lo, hi, 2 * TILE + 100), np.linspace(-26.0, -14.0, 300) / 20.0])).astype(dtype)
    edges = []
    for level in (TH - W / 2, TH, TH + W / 2):
        c = dtype(10.0 ** (level / 20.0))
        up1, dn1 = np.nextafter(c, dtype(np.inf)), np.nextafter(c, dtype(0))
        edges += [c, up1, dn1, np.nextafter(up1, dtype(np.inf)), np.nextafter(dn1, dtype(0))]
        edges += [dtype(float(c) * (1.0 + sg * 2.0 ** -k)) for k in (30, 21) for sg in (1.0, -1.0)]
    x = np.concatenate([[dtype(0.0), dtype(-0.0), tiny, -tiny], mags, np.array(edges, dtype), -np.array(edges, dtype)]).astype(dtype)
    sign = rng.choice([-1.0, 1.0], len(mags)).astype(dtype)
    x[4:4 + len(mags)] *= sign
    x = x.reshape(1, 1, -1)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def curve_reference(dt, knee_db):
    y, g, st = R.compress_ref(curve_row(dt), FS, knee_db=knee_db, **CURVE_KW)
    return y, g, st


def check_curve(what, got, dt, knee_db, key=None):
    """The static curve's bounds: gain within 1e-10 dB (float32: the module's bound for the rounded gain), the output per
    sample within (2u + 1.2e-11) |y_ref|, and every sample clearly under the knee bit for bit."""
    dtype = DTYPES[dt]
    x = curve_row(dt)
    (y, g, st), (yr, gr, sr) = got, curve_reference(dt, knee_db)
    floor = G_MIN if dtype == np.float32 else 2.0 ** -1000
    assert gr.min() >= floor and np.all(np.isfinite(yr))
    db = np.abs(20 * np.log10(g.astype(np.float64)) - 20 * np.log10(gr)).max()
    rel = (np.abs(g.astype(np.float64) - gr) / gr).max()
    ex = np.abs(y.astype(np.float64) - yr) - (2 * U[dtype] + 1.2e-11) * np.abs(yr)
    under = np.abs(x.astype(np.float64)) < 10.0 ** ((TH - knee_db / 2) / 20.0) * (1.0 - 1e-12)
    over = ~under.reshape(-1)
    worst = (ex.reshape(-1)[over] / np.abs(yr.reshape(-1)[over])).max()
    w = WORST.setdefault(key or what, [0.0, -np.inf, 0.0])
    w[0], w[1], w[2] = max(w[0], db if dtype == np.float64 else rel), max(w[1], worst), max(w[2], np.abs(st - sr).max())
    print(f"{what} [{dt}]: gain {db:.3e} dB ({rel:.3e} relative)  y excess over the bound / |y_ref| {worst:.3e}")
    assert (db <= 1e-10) if dtype == np.float64 else (rel <= 2.0 ** -24 + 2e-11), (what, db, rel)
    assert ex.max() <= 0.0, (what, ex.max())
    assert under.sum() > TILE and np.array_equal(bits(y[under]), bits(x[under])) and np.all(g[under.reshape(g.shape)] == 1.0), what
    assert np.abs(st - sr).max() <= 1e-10, what


# ---- channels, groups, state ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def channel_case(channels, dt):
    """``[channels groups, channels, T]`` over the loud floor: group k's loudest sample is negative and sits in channel k."""
    x = loud_floor(np.random.default_rng(600 + channels), (channels, channels, T_SEAMS))
    for k in range(channels):
        x[k, k, P[(5 * k + 3) % len(P)]] = -1.5
    x = x.astype(DTYPES[dt])
    x.setflags(write=False)
    return x


MANY_GROUPS, MANY_T = 600, TILE + 1
MANY_PICK = (0, 1, 255, 256, 511, 512, 599)


@functools.lru_cache(maxsize=None)
def many_groups(dt):
    x = R.bursty(np.random.default_rng(700), (MANY_GROUPS, 1, MANY_T), quiet=0.02, loud=0.7, burst=300, gap=450, dtype=DTYPES[dt])
    x.setflags(write=False)
    return x


STATE_CUTS = (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, T_SEAMS - 1)


@functools.lru_cache(maxsize=None)
def state_case(dt):
    x = R.bursty(np.random.default_rng(800), (2, 2, T_SEAMS), quiet=0.02, loud=0.7, burst=350, gap=650, dtype=DTYPES[dt])
    x.setflags(write=False)
    return x, R.compress_ref(x, FS)
