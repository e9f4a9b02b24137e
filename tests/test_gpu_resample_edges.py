"""GPU parity -- the polyphase resampler (csrc/resample.hip) in every class of its tiling and at its tile seams: exact impulse
responses, a per-sample error bound on signals with quiet stretches, where a NaN / Inf sample may come out, and rows that do
not depend on their batch.

References and the derived tolerance: tests/resample_reference.py.  The case table and the builders below are plain numpy
plus the host-only planning queries; tests/test_resample_reference_host.py imports them and shows on the CPU that the
reference meets every condition asserted here and that every entry lands in the class it is listed for.

A class is what `resample_tiling_info` reports for the launch: the kernel (reg / lds / gather), more than one phase (up > 1),
G halved until the window fit in LDS (G < G_initial), the outputs per thread at their clamp (E == 64) or at one (E == 1).  It is
asserted at every length a test runs, never assumed.  Row lengths come from the plan: for each entry the longest row of one
tile ("below": n_out <= tile_out), the longest row whose second tile holds at most `up` outputs ("above"), the shortest row
of three tiles ("three", left out where it would pass MAX_T samples) and 1, 2 and Lp samples.  The seam of tiles 0 and 1 is
centred on input floor(tile_out * down / up).

Contract: y[m] = sum_i x[i] * h[m*down + half - i*up] as one fma chain per output from +0, so an
impulse of power-of-two amplitude comes out as amp * tap exactly; every output within gamma(Lp + 1) * (|h| (*) |x|)[m]; a
non-finite input i reaches exactly the outputs with 0 <= (m + n_pre_remove)*down - i*up < Lp*up."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import resample_reference as R
from tests.gpu_common import TOL_CONV_F32, TOL_CONV_F64, close, dev, rnd

pytestmark = pytest.mark.gpu

MAX_T = 300_000                         # samples per row; no launch here has more than MAX_ROWS rows
MAX_ROWS = 4
DT = {"f32": np.float32, "f64": np.float64}
TDT = {"f32": torch.float32, "f64": torch.float64}
TOL = {"f32": TOL_CONV_F32, "f64": TOL_CONV_F64}
BADS = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
AMPS = (1.0, -0.5, 0.125)

# want: kernel, and where not None: up > 1, G halved (True) or not (False), E
Case = namedtuple("Case", "cls up down window dt kernel up_gt1 halved E")
REG, LDS, GATHER = "resample_reg_kernel", "resample_lds_kernel", "resample_gather_kernel"


def _cases():
    out = []

    def add(cls, ratios, kernel, up_gt1=None, halved=None, E=None):
        for up, down, window, dts in ratios:
            out.extend(Case(cls, up, down, window, dt, kernel, up_gt1, halved, E) for dt in dts.split("+"))
    add("gather, up > 1", [(3, 4000, None, "f32+f64"), (5, 3001, None, "f32"), (3, 2000, None, "f32"), (2, 1001, None, "f64")],
        GATHER, up_gt1=True)
    add("lds, G halved, up > 1", [(3, 200, None, "f32+f64"), (7, 300, None, "f32"), (3, 700, None, "f32")], LDS, up_gt1=True,
        halved=True)
    add("lds, G halved, E == 1", [(3, 200, None, "f32")], LDS, halved=True, E=1)
    add("lds, up > 1, full G", [(7, 64, None, "f32")], LDS, up_gt1=True, halved=False)
    add("reg, G halved", [(2, 75, ("taps", 41, 1), "f32+f64"), (3, 100, ("taps", 31, 2), "f32")], REG, up_gt1=True, halved=True)
    add("reg, up >= 511", [(511, 512, None, "f32"), (512, 3, None, "f32"), (513, 512, None, "f32")], REG, up_gt1=True, halved=False)
    add("reg, E == 64", [(3, 1, None, "f32"), (512, 3, None, "f32+f64")], REG, halved=False, E=64)      # 3/1 in float64: E = 36
    add("reg, baseline", [(160, 147, None, "f32+f64"), (3, 1, None, "f64")], REG, up_gt1=True, halved=False)
    return out


CASES = _cases()
REACH_CASES = [c for c in CASES if (c.up, c.down, c.dt, c.cls) in {(160, 147, "f32", "reg, baseline"), (3, 200, "f32", "lds, G halved, up > 1"),
                                                                  (2, 1001, "f64", "gather, up > 1")}]


def case_id(c):
    w = "" if c.window is None else f"-{c.window[1]}taps"
    return f"{c.up}/{c.down}{w}-{c.dt}-{c.cls.replace(' ', '').replace(',', '_')}"


def unique(cases):
    """One entry per launch geometry (an entry may be listed under two classes)."""
    seen, out = set(), []
    for c in cases:
        if (c.up, c.down, c.window, c.dt) not in seen:
            seen.add((c.up, c.down, c.window, c.dt))
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- case builders (numpy + host queries)
def window_of(c):
    """None: the product's default design.  ("taps", n, seed): n random taps with sum |w| = 1, float32 values held in float64,
    so that float32 and float64 arithmetic scale them by `up` to the same float32 taps."""
    if c.window is None:
        return ("kaiser", 5.0)
    _, n, seed = c.window
    w = np.random.default_rng(seed).uniform(-1, 1, n)
    return (w / np.abs(w).sum()).astype(np.float32).astype(np.float64)


@lru_cache(maxsize=None)
def taps(c):
    """The taps the product runs for this entry, in the signal dtype."""
    from torchfx_amd.resample import design_taps
    return design_taps(c.up, c.down, window_of(c), TDT[c.dt]).numpy().copy()


@lru_cache(maxsize=None)
def plan(c, T):
    """resample_plan_info and resample_tiling_info for rows of T samples, plus `seam`: the input the seam of tiles 0 and 1 is
    centred on."""
    from torchfx_amd import torchfx_ext
    args = (T, c.up, c.down, len(taps(c)), TDT[c.dt])
    p = dict(torchfx_ext.resample_plan_info(*args))
    t = torchfx_ext.resample_tiling_info(*args)
    assert t["kernel"] == p["kernel"] and t["tiles"] == -(-p["n_out"] // t["tile_out"])
    p.update(t, seam=t["tile_out"] * c.down // c.up)
    return p


def check_class(c, T):
    p = plan(c, T)
    what = f"{case_id(c)} T={T}: {p}"
    assert p["kernel"] == c.kernel, what
    if c.up_gt1:
        assert c.up > 1, what
    if c.halved is not None:
        assert (p["G"] < p["G_initial"]) == c.halved and p["G"] >= 1, what
    if c.E is not None:
        assert p["E"] == c.E, what
    return p


@lru_cache(maxsize=None)
def lengths(c):
    """{"below", "above", "three" (None past MAX_T), "short": [1, 2, Lp]} -- see the module docstring.  Lp, and through it E
    and tile_out, moves a little with T (SciPy's post-padding), so every candidate T is asked for its own plan."""
    up, down = c.up, c.down
    T = 1000
    for _ in range(4):                                   # settle near n_out = tile_out
        T = max(3, plan(c, T)["tile_out"] * down // up)
    lo = max(2, T - 2 * down - 2)
    above = None
    for t in range(lo, lo + 6 * down + 8):
        p = plan(c, t)
        if p["tiles"] == 2 and p["tile_out"] < p["n_out"] <= p["tile_out"] + up:
            above = t                                    # the longest of the first run
        elif above is not None:
            break
    assert above is not None, case_id(c)
    below = above
    while plan(c, below)["n_out"] > plan(c, below)["tile_out"]:
        below -= 1
    three = max(above + 1, 2 * plan(c, above)["tile_out"] * down // up)
    while plan(c, three - 1)["tiles"] >= 3:
        three -= 1
    while plan(c, three)["tiles"] < 3:
        three += 1
    return dict(below=below, above=above, three=three if three <= MAX_T else None, short=[1, 2, plan(c, above)["Lp"]])


def seam_lengths(c):
    L = lengths(c)
    return [(k, L[k]) for k in ("below", "above", "three") if L[k] is not None]


def all_lengths(c):
    out = []
    for T in lengths(c)["short"] + [T for _, T in seam_lengths(c)]:
        if T not in out:
            out.append(T)
    return out


def check_seam(c, kind, T):
    """The class, the tile count the length was chosen for, and the seam inside the row where there is one."""
    p = check_class(c, T)
    what = f"{case_id(c)} {kind} T={T}: {p}"
    assert T <= MAX_T, what
    if kind == "below":
        assert p["tiles"] == 1 and p["n_out"] <= p["tile_out"], what
        assert plan(c, T + 1)["n_out"] > plan(c, T + 1)["tile_out"], what + ": not the longest one-tile row"
    elif kind == "above":
        assert p["tiles"] == 2 and p["tile_out"] < p["n_out"] <= p["tile_out"] + c.up and p["seam"] < T, what
    else:
        assert p["tiles"] == 3 and plan(c, T - 1)["tiles"] == 2, what
    return p


def stair_edges(c, T, row):
    """A step on the seam's centre (both rows), steps Lp / 2 to either side of it and one a whole filter before it, and steps
    through the rest of the row; the second row's other steps are shifted."""
    p = plan(c, T)
    s, Lp = p["seam"], p["Lp"]
    e = [s, s - Lp - row, s - Lp // 2 - 1 - row, s + Lp // 2 + 1 + row]
    e += [T * k // 7 + 3 * row for k in range(1, 7)]
    return e


@lru_cache(maxsize=None)
def stair_case(c, T):
    """Two rows that differ, their reference (long double for float64 entries) and bound."""
    x = np.vstack([R.staircase(1, T, 1000 * c.up + c.down + T + r, stair_edges(c, T, r), DT[c.dt]) for r in range(2)])
    h, Lp = taps(c), plan(c, T)["Lp"]
    return dict(x=x, h=h, ref=R.ref(x, h, c.up, c.down, wide=c.dt == "f64"), bnd=R.bound(x, h, c.up, c.down, Lp))


def impulse_inputs(c, T):
    """Inputs 0, 1, T-2, T-1 and seam + {-Lp, -1, 0, +1}; and the ends of the two windows that meet at the seam, each with its
    neighbour outside: the oldest input of tile 1's first output (x[n // up - (Lp - 1)], n = (tile_out + n_pre_remove)*down: the
    first sample of that tile's window) and the newest input of tile 0's last output."""
    p = plan(c, T)
    s, Lp, pre, tile = p["seam"], p["Lp"], p["n_pre_remove"], p["tile_out"]
    oldest = (tile + pre) * c.down // c.up - (Lp - 1)
    newest = (tile - 1 + pre) * c.down // c.up
    return [0, 1, T - 2, T - 1, s - Lp, s - 1, s, s + 1, oldest - 1, oldest, newest, newest + 1]


def impulse_positions(c, T):
    """`impulse_inputs` (those that exist) in ascending order, with the amplitudes 1, -0.5, 0.125 in turn."""
    pos = []
    for q in impulse_inputs(c, T):
        if 0 <= q < T and q not in pos:
            pos.append(q)
    pos.sort()
    return [(q, AMPS[k % 3]) for k, q in enumerate(pos)]


@lru_cache(maxsize=None)
def impulse_case(c, T):
    """Rows of impulses more than Lp + 1 inputs apart (no output sees two), in launches of at most MAX_ROWS rows:
    [(x [rows, T], expected [rows, n_out])]."""
    Lp, h = plan(c, T)["Lp"], taps(c)
    rows = []                                            # [[(position, amplitude)]]
    for q, a in impulse_positions(c, T):
        for r in rows:
            if q - r[-1][0] > Lp + 1:
                r.append((q, a))
                break
        else:
            rows.append([(q, a)])
    xs = [R.impulses(T, *zip(*r), dtype=DT[c.dt]) for r in rows]
    ys = [R.impulse_response(T, h, c.up, c.down, *zip(*r)) for r in rows]
    return [(np.stack(xs[k:k + MAX_ROWS]), np.stack(ys[k:k + MAX_ROWS])) for k in range(0, len(rows), MAX_ROWS)]


def reach_positions(c, T):
    p = plan(c, T)
    return [0, T - 1, p["seam"], p["seam"] - p["Lp"]]


@lru_cache(maxsize=None)
def reach_case(c, T, pos):
    """Four rows that differ; rows 0..2 get NaN, +Inf, -Inf at `pos`, row 3 stays clean.  x0: the bad samples set to 0; its
    reference and bound; the mask of the outputs the bad sample reaches."""
    p = plan(c, T)
    x0 = np.vstack([rnd((1, T), 7919 * r + T + pos + c.up, DT[c.dt]) for r in range(4)])
    x0[:3, pos] = 0.0
    x = x0.copy()
    for r, v in enumerate(BADS.values()):
        x[r, pos] = v
    h = taps(c)
    mask = R.reach_mask(T, p["n_out"], c.up, c.down, p["n_pre_remove"], p["Lp"], [(r, pos) for r in range(3)], rows=4)
    return dict(x=x, x0=x0, h=h, mask=mask, ref0=R.ref(x0, h, c.up, c.down, wide=c.dt == "f64"),
                bnd=R.bound(x0, h, c.up, c.down, p["Lp"]))


@lru_cache(maxsize=None)
def batch_case(c, T):
    return np.vstack([rnd((1, T), 104729 * r + T + c.down, DT[c.dt]) for r in range(3)])


# ---------------------------------------------------------------------------------------------- assertions
def check_bound(y, ref, bnd, what, where=None):
    """|y - ref| <= bnd on every element (of `where`); returns the largest err / bound there."""
    err = np.abs(np.asarray(y).astype(ref.dtype) - ref).astype(np.float64)
    ok = err <= bnd
    if where is not None:
        ok = ok | ~where
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, 0.0, err / bnd)), err.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} outputs outside the bound; worst at {i}: err {err[i]:.3e}, "
                             f"bound {bnd[i]:.3e}, ref {float(ref[i]):.3e}")
    ratio = err / bnd
    return float(ratio.max() if where is None else ratio[where].max()) if ratio.size else 0.0


def check_impulses(y, exp, what):
    """Equality with ==: the sign of a zero is free, nothing else is."""
    y = np.asarray(y)
    assert y.shape == exp.shape and y.dtype == exp.dtype, f"{what}: {y.shape} {y.dtype}"
    bad = np.argwhere(~(y == exp))
    assert bad.size == 0, (f"{what}: {len(bad)} outputs differ, first at (row, m) = {tuple(bad[0])}: got {y[tuple(bad[0])]!r}, "
                           f"expected {exp[tuple(bad[0])]!r}")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def resample(c, x):
    from torchfx_amd import torchfx_ext
    y = torchfx_ext.resample_forward(dev(x), c.up, c.down, torch.from_numpy(taps(c)))
    assert y.dtype == TDT[c.dt] and y.is_cuda
    return y


# ---------------------------------------------------------------------------------------------- 1. impulses
@pytest.mark.parametrize("c", unique(CASES), ids=case_id)
def test_impulse_responses_are_the_taps(c):
    """Every product but one of an output's chain is an exact zero and a power-of-two amplitude scales a normal tap exactly, so
    the outputs are amp * h[m*down + half - i*up] bit for bit (up to the sign of a zero): a dropped or doubled edge tap, a phase
    off by one or a window staged one input short all show."""
    T = lengths(c)["above"]
    check_seam(c, "above", T)
    for k, (x, exp) in enumerate(impulse_case(c, T)):
        assert x.shape[0] <= MAX_ROWS
        check_impulses(resample(c, x).cpu().numpy(), exp, f"{case_id(c)} T={T} launch {k}")


# ---------------------------------------------------------------------------------------------- 2. per-sample bound
@pytest.mark.parametrize("c", unique(CASES), ids=case_id)
def test_staircase_bound(c):
    """Amplitude steps of 2^-10 down to 2^-30 and back, one on the seam's centre: every output within the forward error bound
    of an Lp-term sum in the signal dtype -- an error that scales with the loud part of a window is far outside it in the
    quiet part.  Prints the largest err / bound (a measurement)."""
    kinds = dict((T, k) for k, T in seam_lengths(c))
    worst = 0.0
    for T in all_lengths(c):
        if T in kinds:
            check_seam(c, kinds[T], T)
        s = stair_case(c, T)
        y = resample(c, s["x"]).cpu().numpy()
        what = f"{case_id(c)} T={T}"
        worst = max(worst, check_bound(y, s["ref"], s["bnd"], what))
        close(y, s["ref"].astype(y.dtype), TOL[c.dt], what)
    print(f"\nresample err/bound | {c.cls} | {c.up}/{c.down} {c.dt} | {worst:.4f}")


# ---------------------------------------------------------------------------------------------- 3. non-finite reach
@pytest.mark.parametrize("c", REACH_CASES, ids=case_id)
def test_non_finite_reach(c):
    """NaN, +Inf and -Inf on the first and last input, on the seam's centre and Lp inputs before it: the non-finite outputs are
    exactly the reach, the others stay inside the bound of the signal without the bad sample, and the clean row of the launch
    keeps the bits it has alone."""
    T = lengths(c)["above"]
    check_seam(c, "above", T)
    assert c.up > 1
    for pos in reach_positions(c, T):
        r = reach_case(c, T, pos)
        what = f"{case_id(c)} T={T} bad input {pos}"
        y = resample(c, r["x"]).cpu().numpy()
        nf = ~np.isfinite(y)
        assert not r["mask"][3].any() and r["mask"][:3].any(axis=1).all(), what
        assert np.array_equal(nf, r["mask"]), (f"{what}: non-finite outputs (row, first, last) "
                                                f"{[(i, *np.flatnonzero(m)[[0, -1]]) for i, m in enumerate(nf) if m.any()]}, reach "
                                                f"{[(i, *np.flatnonzero(m)[[0, -1]]) for i, m in enumerate(r['mask']) if m.any()]}")
        check_bound(y, r["ref0"], r["bnd"], what, where=~r["mask"])
        alone = resample(c, r["x"][3:]).cpu().numpy()
        assert np.array_equal(bits(y[3]), bits(alone[0])), f"{what}: the clean row depends on its neighbours"


# ---------------------------------------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize("c", unique(CASES), ids=case_id)
def test_rows_do_not_depend_on_the_batch(c):
    T = lengths(c)["above"]
    check_seam(c, "above", T)
    x = dev(batch_case(c, T))
    from torchfx_amd import torchfx_ext
    h = torch.from_numpy(taps(c))
    together = torchfx_ext.resample_forward(x, c.up, c.down, h)
    for r in range(x.shape[0]):
        assert torch.equal(together[r:r + 1], torchfx_ext.resample_forward(x[r:r + 1].contiguous(), c.up, c.down, h)), f"{case_id(c)} row {r}"
