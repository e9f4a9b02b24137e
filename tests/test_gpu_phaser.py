"""The phaser on the device (csrc/phaser.hip) against tests/phaser_reference.py.  Two checks, kept apart: the coefficient track the
kernel stores against the long-double track within the derived delta_a, and the recursion against the per-sample loop fed the
kernel's own coefficient bits, within 16 E_REF of the loop's long-double twin -- every length class of the tiling, row counts and a
batch, 1 to 12 stages, both LFO shapes, every segment count that cuts the row differently, position 2^40, the weakest-decay corner,
a given state, a cut and rejoin -- and the exact properties with torch.equal: the dry path, equal rows, row independence, causality
and the reach of a planted NaN / Inf.  Signals hold float32-representable values so that one reference serves both dtypes."""
import functools

import numpy as np
import pytest
import torch

from tests import phaser_reference as R
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 48000
DTYPES = {"f32": torch.float32, "f64": torch.float64}
BASE = dict(stages=4, fs=FS, rate=3.0, min_freq=200.0, max_freq=2000.0, phase=0.1, spread=0.25, dry=0.6, wet=0.5, shape="sine")
CORNER = dict(BASE, fs=192000, min_freq=10.0, max_freq=0.45 * 192000, rate=40.0)


@functools.lru_cache(maxsize=None)
def tile():
    return ext().phaser_plan_info(1, 1, 1, 1)["tile"]


def long_T():
    return 3 * tile() + 17


def signal(shape, seed):
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)
    x.setflags(write=False)
    return x


def run(x, dt="f64", segments=0, state=None, position=0, **over):
    """The low-level op on x (array): (y, coef, new state) as arrays."""
    p = dict(BASE, **over)
    t = torch.from_numpy(np.array(x)).to(DEV, DTYPES[dt])
    st = None if state is None else torch.from_numpy(np.array(state, dtype=np.float64)).to(DEV)
    y, coef, new, _ = ext().phaser_forward(t, p["stages"], p["fs"], p["rate"], p["min_freq"], p["max_freq"], p["phase"], p["spread"],
                                           p["dry"], p["wet"], p["shape"], position, None, st, True, segments)
    torch.cuda.synchronize()
    assert y.shape == t.shape and y.dtype == t.dtype and new.shape == (max(1, int(np.prod(t.shape[:-1]))), p["stages"] + 1)
    return y.cpu().numpy(), coef.cpu().numpy(), new.cpu().numpy()


_REFS = {}


def ref_for(key, x, coef, state=None, **over):
    """The case's (long-double result, end state, E_REF), computed once from the first coefficient track seen for `key`; every
    later call must bring the same bits."""
    p = dict(BASE, **over)
    if key not in _REFS:
        rows = x.reshape(-1, x.shape[-1])
        C = x.shape[-2] if x.ndim >= 2 else 1
        _REFS[key] = (coef.copy(),) + R.reference(rows, coef, p["stages"], p["dry"], p["wet"], C, state)
    c0, yld, sld, e_ref = _REFS[key]
    assert np.array_equal(c0, coef), f"{key}: the coefficient track changed"
    return yld.reshape(x.shape), sld, e_ref


def both_checks(key, x, dt, segments=0, state=None, position=0, **over):
    p = dict(BASE, **over)
    y, coef, st = run(x, dt, segments, state, position, **over)
    C = x.shape[-2] if x.ndim >= 2 else 1
    assert coef.shape == ((C if p["spread"] != 0.0 and C > 1 else 1), x.shape[-1])
    R.check_coef(coef, p["fs"], p["min_freq"], p["max_freq"], p["rate"], p["phase"], p["spread"], p["shape"], position, f"{key} {dt}")
    yld, sld, e_ref = ref_for(key, x, coef, state, **over)
    R.check(y, yld, e_ref, f"{key} {dt} segments={segments}")
    assert np.array_equal(st[:, 0], x.reshape(-1, x.shape[-1])[:, -1].astype(np.float64))      # x_0[T-1] is the input's last sample
    return y, coef, st, yld, e_ref


def at_work(yld, x, dry, e_ref, what):
    """The result differs from dry x by more than 100 times the tolerance in every row."""
    rows = yld.reshape(-1, yld.shape[-1]).astype(np.float64)
    gap = np.abs(rows - dry * x.reshape(rows.shape).astype(np.float64)).max(-1)
    tol = 16.0 * e_ref + 2.0 ** -24 * np.abs(rows).max(-1)
    assert np.all(gap > 100.0 * tol), f"{what}: the wet part is not at work"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("which", ["1", "2", "7", "8", "9", "tile-1", "tile", "tile+1", "3tile+17"])
def test_lengths(which, dt):
    T = {"tile-1": tile() - 1, "tile": tile(), "tile+1": tile() + 1, "3tile+17": long_T()}.get(which) or int(which)
    x = signal((3, T), 10 + T % 97)
    *_, yld, e_ref = both_checks(f"len{T}", x, dt)
    if T > 8:
        at_work(yld, x, BASE["dry"], e_ref, f"T={T}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("lead", [(), (2,), (3,), (5, 2)])
def test_shapes(lead, dt):
    x = signal(lead + (tile() + 1,), 21 + len(lead))
    *_, yld, e_ref = both_checks(f"shape{lead}", x, dt, stages=2)
    at_work(yld, x, BASE["dry"], e_ref, f"shape {lead}")


@pytest.mark.parametrize("lfo", ["sine", "triangle"])
@pytest.mark.parametrize("N", [1, 2, 4, 12])
def test_stages_and_lfo_shapes(N, lfo):
    x = signal((2, tile() + 1), 30 + N)
    for dt in DTYPES:
        *_, yld, e_ref = both_checks(f"N{N}{lfo}", x, dt, stages=N, shape=lfo)
    at_work(yld, x, BASE["dry"], e_ref, f"N={N} {lfo}")


def test_spread_makes_the_channels_differ_and_its_absence_shares_the_track():
    x = signal((2, 2, tile() + 1), 40)
    _, coef, *_ = both_checks("spread", x, "f64")
    assert coef.shape[0] == 2 and not np.array_equal(coef[0], coef[1])
    _, shared, *_ = both_checks("nospread", x, "f64", spread=0.0)
    assert shared.shape[0] == 1
    # batch items of equal channel index share the track bit for bit: one row of coef serves both
    solo, c1, _ = run(x[1], "f64")
    assert np.array_equal(c1, coef)


@pytest.mark.parametrize("rows", [1, 3])
def test_segments(rows):
    x = signal((rows, long_T()), 50 + rows)
    info = ext().phaser_plan_info(long_T(), rows, rows, 4, 9)
    assert info["tiles"] == 4 and info["segments"] == 4 and info["scratch_bytes"] == rows * 4 * 2 * 4 * 8
    for dt in DTYPES:
        base = None
        for segments in (1, 0, 2, 3, 9):
            y, coef, st, yld, e_ref = both_checks(f"seg{rows}", x, dt, segments)
            base = coef if base is None else base
            assert np.array_equal(coef, base)
            # the dry path returns a finite input bit for bit at every segment count
            t = torch.from_numpy(np.array(x)).to(DEV, DTYPES[dt])
            d, *_ = ext().phaser_forward(t, 4, FS, 3.0, 200.0, 2000.0, 0.1, 0.25, 1.0, 0.0, "sine", 0, None, None, False, segments)
            assert torch.equal(d, t)
    at_work(yld, x, BASE["dry"], e_ref, f"segments, {rows} row(s)")


def test_position_2_to_the_40():
    x = signal((2, tile() + 1), 60)
    for dt in DTYPES:
        _, far, *_ = both_checks("pos", x, dt, position=1 << 40)
    _, near, _ = run(x, "f64")
    assert not np.array_equal(far, near)


@pytest.mark.parametrize("segments", [1, 3])
def test_weakest_decay_corner(segments):
    """fs = 192 kHz with min_freq = 10 Hz puts a down to -0.9997, max_freq = 0.45 fs sweeps it up to +0.73 (1.3 LFO cycles here)."""
    x = signal((2, long_T()), 70)
    for dt in DTYPES:
        _, coef, _, yld, e_ref = both_checks("corner", x, dt, segments, **CORNER)
    assert coef.min() < -0.999 and coef.max() > 0.7
    at_work(yld, x, BASE["dry"], e_ref, "corner")


def test_given_state_and_cut_and_rejoin():
    T, cut = long_T(), tile() + 5
    x = signal((3, T), 80)
    state = np.random.default_rng(81).uniform(-1.0, 1.0, (3, 5))
    for dt in DTYPES:
        for segments in (1, 3):
            both_checks("state", x, dt, segments, state=state)
        # cut at tile + 5, rejoined through the returned state and the position
        ya, ca, sa = run(x[:, :cut], dt, state=state)
        yb, cb, sb = run(x[:, cut:], dt, state=sa, position=cut)
        whole, coef, *_ = run(x, dt, state=state)
        assert np.array_equal(np.concatenate([ca, cb], -1), coef)
        yld, sld, e_ref = ref_for("state", x, coef, state)
        R.check(np.concatenate([ya, yb], -1), yld, e_ref, f"cut and rejoin {dt}")


def test_equal_rows_and_row_independence():
    T = long_T()
    x = np.array(signal((2, 2, T), 90))
    x[1] = x[0]                                                # batch items with equal rows
    for dt in DTYPES:
        for segments in (1, 3):
            y, *_ = run(x, dt, segments)
            assert np.array_equal(y[0], y[1])
            other = x.copy()
            other[0, 1] = signal((T,), 91)                     # another row's values change; this row's bits do not
            z, *_ = run(other, dt, segments)
            assert np.array_equal(z[0, 0], y[0, 0]) and np.array_equal(z[1], y[1]) and not np.array_equal(z[0, 1], y[0, 1])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("where", ["mid-lane", "tile seam", "segment seam"])
def test_a_planted_non_finite_sample(where, bad):
    T = long_T()
    m = {"mid-lane": 37, "tile seam": tile(), "segment seam": 2 * tile()}[where]      # 4 tiles in 3 segments: 2 + 1 + 1
    x = np.array(signal((3, T), 95))
    zeros = x.copy()
    zeros[1, m:] = 0.0
    planted = x.copy()
    planted[1, m] = bad
    for dt in DTYPES:
        for segments in (1, 3):
            clean, *_ = run(zeros, dt, segments)
            y, _, st = run(planted, dt, segments)
            assert np.array_equal(y[1, :m], clean[1, :m]), "outputs before the planted sample changed"
            assert not np.isfinite(y[1, m:]).any(), "a finite output after the planted sample"
            assert np.array_equal(y[0], clean[0]) and np.array_equal(y[2], clean[2]), "another row changed"
            assert not np.isfinite(st[1, 1:]).any() and np.isfinite(st[[0, 2]]).all()


def test_cpu_tensors_are_refused_by_the_op_and_served_by_the_function():
    from torchfx_amd import phase_shift

    x = torch.from_numpy(np.array(signal((2, 300), 99)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext().phaser_forward(x, 4, FS, 3.0, 200.0, 2000.0)
    host = phase_shift(x, FS, rate=3.0)
    dev = phase_shift(x.to(DEV), FS, rate=3.0)
    assert host.shape == x.shape and not host.is_cuda and dev.is_cuda
    assert torch.allclose(dev.cpu(), host, rtol=0, atol=2e-7)


def test_route_and_explain_name_the_plan():
    import torchfx_amd as f

    x = torch.from_numpy(np.array(signal((2, long_T()), 98))).to(DEV)
    ph = f.Phaser(rate=3.0, stages=6, shape="triangle")
    w = f.Wave(x, FS, device=DEV) | ph
    want = f"native (phaser_kernel, 6 stage(s), triangle LFO, 4 tile(s) of {tile()} per row in 4 segment(s); two launches)"
    assert ph.route(x) == want and w.explain() == ["Phaser: " + want]
    assert ph.route(x, 100).endswith("1 tile(s) of 2048 per row in 1 segment(s); one launch)")
    assert torch.equal(w.ys, f.phase_shift(x, FS, 6, rate=3.0, shape="triangle"))


def test_zz_report():
    """Closing report: the largest deviation seen, in units of the bound 16 E_REF (+ 2^-24 |ref| for float32), per dtype."""
    for name, ratio in sorted(R.RATIOS.items()):
        units = f", i.e. {16.0 * ratio:.2f} E_REF" if name == "float64" else " (the final rounding to float32 alone reaches 1)"
        print(f"phaser on the device, {name}: largest deviation / bound {ratio:.3f}{units}")
    assert all(r <= 1.0 for r in R.RATIOS.values())
