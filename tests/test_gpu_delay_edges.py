"""GPU parity -- the one-launch Delay (csrc/delay.hip) in every regime its plan can choose and at the seams inside a launch:
exact echoes of integer signals, a per-sample error bound and bit identity with the torch composition on noise, where a
NaN / Inf sample may come out, and the epilogue's statistics when a row is reduced from several workgroups.

Reference and the derived tolerance: tests/delay_reference.py.  The case table and the builders below are plain numpy plus the
host-only `delay_tiling_info`; tests/test_delay_reference_host.py imports them and shows on the CPU that every entry lands in
the class it is listed for and that the torch composition meets what is asserted here.

A class is the regime `delay_tiling_info` reports for the launch (span / lattice / gather) and, where an entry names them, its
residue blocks, steps per chunk and chunks.  It is asserted before anything runs.  The selection edges of `delay_regime`
that the table pins: S = taps*D = 4096 (the last span before lattice) and 4104; taps = 8 / 9 past four tiles (600 x 9 here, 600 x 8
in the host test); D = 255 with 17 taps (below D = 256 the lattice needs S > 4096, that is more than 8 taps, so that edge never
decides alone); and the 64 KiB LDS fit, which moves with the dtype and with ping-pong (the largest D that fits with 16 taps,
and D + 1, per variant; 512 x 8, 600 x 9, 255 x 17 and 768 x 5 leave span for float64 pairs only).

Every (D, taps, T) runs as float32 and float64, mono on two rows and ping-pong on four, unless the entry says otherwise."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import delay_reference as R
from tests.gpu_common import dev
from tests.test_gpu_delay import composition

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}
TDT = {"f32": torch.float32, "f64": torch.float64}
VARIANTS = [("f32", False), ("f32", True), ("f64", False), ("f64", True)]
MIXES = (0.0, 0.25, 0.5, 0.75, 1.0)
BADS = (np.nan, np.inf, -np.inf, np.nan)
SPAN, LATTICE, GATHER = "span", "lattice", "gather"
TILE = 1024                              # outputs per span / gather workgroup
# the largest D whose 16 taps still fit 64 KiB of LDS: rows * (16 D + 1024) * element size <= 65536
LDS_EDGE = {("f32", False): 960, ("f32", True): 448, ("f64", False): 448, ("f64", True): 192}

# want: ((key, value), ...) of delay_tiling_info that the entry expects besides the regime
Case = namedtuple("Case", "cls D taps T dt pp want")


def _cases():
    out = []

    def add(D, taps, T, cls, other=None, only=None, **want):
        for dt, pp in VARIANTS:
            if only is None or (dt, pp) in only:
                k = (other or {}).get((dt, pp), cls)
                out.append(Case(k, D, taps, T, dt, pp, tuple(sorted(want.items())) if k == cls else ()))
    T0 = 2 * TILE + 5
    f64pp = ("f64", True)
    # span
    add(0, 3, T0, SPAN)
    add(1, 5, T0, SPAN)
    add(37, 4, T0, SPAN)
    add(512, 8, T0, SPAN, {f64pp: LATTICE})                 # S = 4096: the last span before lattice (float64 pairs: no LDS fit)
    add(600, 9, T0, SPAN, {f64pp: GATHER})                  # halo over five tiles, one tap more than the ring
    add(255, 17, T0, SPAN, {f64pp: GATHER})                 # D one short of the lattice
    add(20, 70, T0, SPAN)                                   # amplitudes from the device table
    add(768, 5, 26 * 768 + 300, SPAN, {f64pp: LATTICE})     # S = 3840 < 4096: span wherever it fits
    for v, D in LDS_EDGE.items():
        add(D, 16, T0, SPAN, only=[v], lds_bytes=65536)
        add(D + 1, 16, T0, GATHER, only=[v], lds_bytes=0)
    # lattice
    add(513, 8, 40 * 513, LATTICE, tiles=3, kc=16, nchunks=3)               # S = 4104; the last residue block has one live lane
    add(768, 6, 26 * 768, LATTICE, tiles=3, kc=16, nchunks=2)               # 32 steps: a full last chunk
    add(768, 6, 26 * 768 + 300, LATTICE, tiles=3, kc=16, nchunks=3)         # 33 steps: a one-step last chunk
    add(768, 6, 32 * 768 + 77, LATTICE, tiles=3, kc=16, nchunks=3)          # 39 steps: a ragged last chunk
    add(4097, 1, 20 * 4097, LATTICE, tiles=17, kc=16, nchunks=2)
    add(12000, 8, 120_007, LATTICE, tiles=47, kc=16, nchunks=2)
    add(4097, 2, 300, LATTICE, tiles=17, kc=16, nchunks=1)                   # T < D
    # gather
    add(3, 5000, 3000, GATHER, {("f32", False): SPAN})
    add(100, 200, T0, GATHER)
    return out


CASES = _cases()
EPILOGUE_CASES = [c for c in CASES if (c.D, c.taps, c.T, c.dt) in {(513, 8, 40 * 513, "f32"), (37, 4, 2 * TILE + 5, "f32"),
                                                                   (100, 200, 2 * TILE + 5, "f64")}]


def case_id(c):
    return f"{c.D}x{c.taps}-T{c.T}-{c.dt}-{'pp' if c.pp else 'mono'}-{c.cls}"


def rows_of(c):
    return 4 if c.pp else 2


def feedback_of(c):
    """The exact inputs' feedback: 0.5 up to 8 taps (amplitudes down to 2^-7), 1.0 above, where 0.5 would need more than 24 bits."""
    return 0.5 if c.taps <= 8 else 1.0


def noise_feedback(c):
    """The noise signals' feedback.  The bound's model (gamma) has no term for underflow, so no a_i * x may leave the normal range
    of float32: 0.7 up to 100 taps (0.7^99 = 5e-16), 0.999 above (0.999^4999 = 7e-3; 0.7^300 is already a float32 subnormal)."""
    return 0.7 if c.taps <= 100 else 0.999


# ---------------------------------------------------------------------------------------------- builders (numpy + host queries)
@lru_cache(maxsize=None)
def plan(c, T=None):
    from torchfx_amd import torchfx_ext
    return torchfx_ext.delay_tiling_info(rows_of(c), c.T if T is None else T, c.D, c.taps, TDT[c.dt], c.pp)


def check_class(c, T=None):
    """The regime (and what else the entry names) from the launch's own plan, and the plan's arithmetic."""
    p = plan(c, T)
    T = c.T if T is None else T
    what = f"{case_id(c)} T={T}: {p}"
    assert p["regime"] == c.cls, what
    L = T + c.taps * c.D
    units = rows_of(c) if c.cls == GATHER else rows_of(c) // (2 if c.pp else 1)
    assert p["units"] == units and p["nwg"] == p["units"] * p["groups"], what
    if c.cls == LATTICE:
        steps = -(-L // c.D)
        assert p["tiles"] == -(-c.D // 256) and p["nchunks"] == -(-steps // p["kc"]) and p["groups"] == p["tiles"] * p["nchunks"], what
    else:
        assert p["tiles"] == -(-L // TILE) == p["groups"] and p["kc"] == p["nchunks"] == 0, what
    if T == c.T:
        for k, v in c.want:
            assert p[k] == v, f"{what}: {k} != {v}"
    return p


def int_signal(c, seed, T=None):
    """Integers in [-1000, 1000]: with feedback_of(c) and the five mixes every product, sum and lerp is exactly representable."""
    T = c.T if T is None else T
    g = np.random.default_rng(1000 * seed + 7 * c.D + c.taps + T)
    return g.integers(-1000, 1001, (rows_of(c), T)).astype(DT[c.dt])


@lru_cache(maxsize=None)
def noise_case(c):
    """Uniform noise in [-1, 1) in the signal dtype with noise_feedback(c), and its wet / dry / S."""
    g = np.random.default_rng(31 * c.D + c.taps + c.T)
    x = g.uniform(-1, 1, (rows_of(c), c.T)).astype(DT[c.dt])
    dry, wet, S = R.wet_dry(x, c.D, c.taps, noise_feedback(c), c.pp)
    return dict(x=x, dry=dry, wet=wet, S=S)


def reach_positions(c):
    """First and last sample; the last input of lattice chunk 0 (step kc - 1, lane D - 1) and the first of chunk 1 (lane 0, and
    the first lane of the last residue block); either side of the seam of tiles 0 and 1 (span, gather)."""
    p = plan(c)
    pos = [0, c.T - 1]
    if c.cls == LATTICE:
        if p["nchunks"] > 1:
            pos += [p["kc"] * c.D - 1, p["kc"] * c.D, p["kc"] * c.D + (p["tiles"] - 1) * 256]
    else:
        pos += [TILE - 1, TILE]
    out = []
    for q in pos:
        if 0 <= q < c.T and q not in out:
            out.append(q)
    return out


def bad_samples(c, pos):
    """[(row, position)]: one per row, shifted by the row number so that the rows of a pair differ."""
    return [(r, pos + r if pos + r < c.T else pos - r) for r in range(rows_of(c))]


@lru_cache(maxsize=None)
def reach_case(c, pos):
    g = np.random.default_rng(17 * c.D + c.taps + pos)
    x0 = g.uniform(-1, 1, (rows_of(c), c.T)).astype(DT[c.dt])
    bad = bad_samples(c, pos)
    x = x0.copy()
    for r, q in bad:
        assert 0 <= q < c.T
        x0[r, q] = 0.0
        x[r, q] = BADS[r]
    return dict(x=x, x0=x0, mask=R.reach_mask(bad, rows_of(c), c.T, c.D, c.taps, c.pp))


# ---------------------------------------------------------------------------------------------- assertions
def check_exact(y, ref, what):
    """Equality with ==: the sign of a zero is free, nothing else is."""
    y = np.asarray(y)
    assert y.shape == ref.shape, f"{what}: shape {y.shape} != {ref.shape}"
    bad = np.argwhere(~(y.astype(np.float64) == ref))
    assert bad.size == 0, (f"{what}: {len(bad)} outputs differ, first at (row, n) = {tuple(bad[0])}: got {y[tuple(bad[0])]!r}, "
                           f"expected {ref[tuple(bad[0])]!r}")


def check_bound(y, ref, bnd, what, where=None):
    """|y - ref| <= bnd on every element (of `where`), which asks for an exact 0 where S = 0; returns the largest err / bound."""
    err = np.abs(np.asarray(y).astype(np.float64) - ref)
    ok = err <= bnd
    if where is not None:
        ok = ok | ~where
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, 0.0, err)), err.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} outputs outside the bound; worst at {i}: err {err[i]:.3e}, "
                             f"bound {bnd[i]:.3e}, ref {ref[i]:.3e}")
    ratio = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)
    if where is not None:
        ratio = ratio[where]
    return float(ratio.max()) if ratio.size else 0.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def shaped(c, x):
    """[rows, T] as the tensor the op takes: ping-pong pairs are the last-but-one axis."""
    t = dev(x)
    return t.view(t.shape[0] // 2, 2, t.shape[-1]) if c.pp else t


def delay(c, x, feedback, mix, epilogue=None):
    from torchfx_amd import torchfx_ext
    y = torchfx_ext.delay_forward(shaped(c, x), c.D, c.taps, feedback, mix, c.pp, epilogue=epilogue)
    assert y.dtype == TDT[c.dt] and y.is_cuda and y.shape[-1] == x.shape[-1] + c.taps * c.D
    return y.reshape(x.shape[0], x.shape[-1] + c.taps * c.D)


WORST = {}


def report(c, ratio, kind):
    WORST[c.cls, kind] = max(WORST.get((c.cls, kind), 0.0), ratio)
    print(f"\ndelay err/bound ({kind}) | {case_id(c)} | {ratio:.4f} | worst of {c.cls} so far {WORST[c.cls, kind]:.4f}")


# ---------------------------------------------------------------------------------------------- 1. exact echoes
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_exact_echoes(c):
    """Integer signals at the five mixes equal the float64 definition exactly: a sample taken from the wrong place, a tap dropped
    at a seam or a row of the wrong parity cannot hide under a tolerance.  Two signals of one shape, the first result freed
    before the second launch, so that an output the kernel never writes shows the first signal's values."""
    check_class(c)
    fb = feedback_of(c)
    for mix in MIXES:
        for seed in (1, 2):
            x = int_signal(c, seed)
            dry, wet, _ = R.wet_dry(x, c.D, c.taps, fb, c.pp)
            y = delay(c, x, fb, mix)
            got = y.cpu().numpy()
            del y
            check_exact(got, R.mix_of(dry, wet, mix), f"{case_id(c)} mix={mix} signal {seed}")


# ---------------------------------------------------------------------------------------------- 2. noise: bound, bit identity
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_noise_within_the_bound(c):
    """Every output within gamma(taps + 6) * S of the float64 definition, on both branches of the lerp; exactly 0 where S = 0.
    Prints the largest err / bound (a measurement)."""
    check_class(c)
    n = noise_case(c)
    bnd = R.bound(n["S"], c.taps, DT[c.dt])
    worst = 0.0
    for mix in (0.3, 0.65):
        y = delay(c, n["x"], noise_feedback(c), mix).cpu().numpy()
        worst = max(worst, check_bound(y, R.mix_of(n["dry"], n["wet"], mix), bnd, f"{case_id(c)} mix={mix}"))
    report(c, worst, "noise")


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_noise_bit_identical_to_the_composition(c):
    """torch.equal with the reference's composition run by torch on the device: only this sees the tap order, the separately
    rounded product and sum, and ATen's lerp."""
    check_class(c)
    x = shaped(c, noise_case(c)["x"])
    for mix in (0.3, 0.65):
        from torchfx_amd import torchfx_ext
        y = torchfx_ext.delay_forward(x, c.D, c.taps, noise_feedback(c), mix, c.pp)
        ref = composition(x, c.D, c.taps, noise_feedback(c), mix, c.pp)
        assert y.shape == ref.shape and y.dtype == ref.dtype
        if not torch.equal(y, ref):
            d = (y != ref).nonzero()
            raise AssertionError(f"{case_id(c)} mix={mix}: {len(d)} outputs differ from the composition, first at {d[0].tolist()}: "
                                 f"{y[tuple(d[0])].item()!r} != {ref[tuple(d[0])].item()!r}")


# ---------------------------------------------------------------------------------------------- 3. non-finite reach
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_non_finite_reach(c):
    """One NaN / +Inf / -Inf per row (feedback 0.5, mix 0.3): the non-finite outputs are exactly the reach, every other output
    keeps the bits it has with the bad samples set to 0."""
    check_class(c)
    for pos in reach_positions(c):
        r = reach_case(c, pos)
        what = f"{case_id(c)} bad samples {bad_samples(c, pos)}"
        y = delay(c, r["x"], 0.5, 0.3).cpu().numpy()
        clean = delay(c, r["x0"], 0.5, 0.3).cpu().numpy()
        assert np.isfinite(clean).all(), what
        nf = ~np.isfinite(y)
        if not np.array_equal(nf, r["mask"]):
            extra, missing = np.argwhere(nf & ~r["mask"]), np.argwhere(~nf & r["mask"])
            raise AssertionError(f"{what}: {len(extra)} non-finite outputs outside the reach (first {extra[:3].tolist()}), "
                                 f"{len(missing)} finite inside it (first {missing[:3].tolist()})")
        keep = ~r["mask"]
        assert np.array_equal(bits(y)[keep], bits(clean)[keep]), f"{what}: outputs outside the reach changed"


# ---------------------------------------------------------------------------------------------- 4. T = 0 and T = 1
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_empty_and_one_sample_rows(c):
    """T = 0: taps*D zeros.  T = 1: the sample and its echoes, exactly, and bit-identical to the composition."""
    from torchfx_amd import torchfx_ext
    check_class(c, 0)
    y0 = delay(c, np.zeros((rows_of(c), 0), DT[c.dt]), 0.7, 0.3)
    assert y0.shape == (rows_of(c), c.taps * c.D) and not y0.any(), case_id(c)
    check_class(c, 1)
    fb = feedback_of(c)
    x = int_signal(c, 3, T=1)
    for mix in MIXES:
        check_exact(delay(c, x, fb, mix).cpu().numpy(), R.delay_ref(x, c.D, c.taps, fb, mix, c.pp)[0], f"{case_id(c)} T=1 mix={mix}")
    xn = shaped(c, np.random.default_rng(c.D + c.taps).uniform(-1, 1, (rows_of(c), 1)).astype(DT[c.dt]))
    assert torch.equal(torchfx_ext.delay_forward(xn, c.D, c.taps, 0.7, 0.3, c.pp), composition(xn, c.D, c.taps, 0.7, 0.3, c.pp))


# ---------------------------------------------------------------------------------------------- 5. epilogue statistics
@pytest.mark.parametrize("c", EPILOGUE_CASES, ids=case_id)
def test_epilogue_statistics_at_the_seams(c):
    """A row reduced from several workgroups (three lattice chunks of three residue blocks; span and gather tiles): abs-max is
    max|y| of the returned y exactly; the RMS from the sum of squares is within n * 2^-53 (relative) of numpy's float64 RMS of
    the returned y, n the samples reduced -- the forward error of an n-term float64 sum of non-negative terms in any order; gain
    and clamp give the bits of applying them to the plain result."""
    from torchfx_amd import torchfx_ext
    p = check_class(c)
    assert p["groups"] >= 3 and (c.cls != LATTICE or p["nchunks"] == 3), p
    n = noise_case(c)
    fb = noise_feedback(c)
    plain = delay(c, n["x"], fb, 0.3)
    for gain, clamp in ((1.0, False), (0.7, False), (2.5, True)):
        want = plain * gain if gain != 1.0 else plain
        want = want.clamp(-1.0, 1.0) if clamp else want
        for stat in ("absmax", "sumsq"):
            for per_row in (False, True):
                what = f"{case_id(c)} gain={gain} clamp={clamp} {stat} per_row={per_row}"
                ep = torchfx_ext.Epilogue(gain=gain, clamp=clamp, stat=stat, per_row=per_row)
                y = delay(c, n["x"], fb, 0.3, epilogue=ep)
                assert torch.equal(y, want), what
                got = ep.stat_value.cpu().numpy()
                yd = y.cpu().numpy().astype(np.float64)
                yd = yd if per_row else yd.reshape(1, -1)
                assert got.shape == (yd.shape[0],) and got.dtype == np.float64, what
                if stat == "absmax":
                    assert np.array_equal(got, np.abs(yd).max(axis=1)), what
                else:
                    count = yd.shape[1]
                    rms, ref = np.sqrt(got / count), np.sqrt(np.mean(yd * yd, axis=1))
                    assert (np.abs(rms - ref) <= count * 2.0 ** -53 * ref).all(), f"{what}: {rms} vs {ref}"
