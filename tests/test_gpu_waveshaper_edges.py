"""The waveshaper's kernels (csrc/waveshaper.hip) at every geometry of tests/waveshaper_cases.py, through the low-level ops with
explicit host taps, so that stages of equal and of unequal length share the helpers:

A  every register bucket (its smallest and its largest tap count) and every unequal pair, one-shot, against the wide reference
   within the per-sample bound of tests/waveshaper_reference.py: the hard clipper at 9 dB (no transfer-function allowance, the
   tightest bound), then tanh, cubic or a 5-point curve under a bias and a partial mix.  Equal stages also go through the public
   waveshape(..., window=h), which must be torch.equal.
B  the stream form at the same geometries: chunks of 1, D - 1, D, D + 1, Hs, 0, 512, 513, tile - 1, tile + 1 and the rest, then
   the tail, have the bits of the one-shot call that A ties to the reference.  512 | 513 is the two-chains-per-thread
   decimator's limit, tile +- 1 the whole-waves cut of the positions.
C  exact tap probes: one stage a single tap, the other an asymmetric low-pass, impulses of power-of-two amplitudes at 0, a mid
   position, tile - 1, tile and T - 1.  Every output is one exact product, so the outputs are the probed taps in order and
   np.array_equal holds (tests/test_waveshaper_cases_host.py shows that a reversed, shifted or swapped array fails it).
D  NaN, +Inf and -Inf at 0, T - 1, tile - 1 and tile poison exactly [i - reach_before, i + reach_after] at the extreme
   geometries (two taps per phase, buckets 48 and 72, I0 = -32 and +32), and an up-sampled value that overflows from finite input
   poisons exactly the decimator's reach of that one sample.
E  the transfer functions' edges at L = 1 (waveshaper_plain_kernel) and at L = 2 with one-tap stages: +-0, the smallest
   denormal, +-1 and its neighbours, v = +-Inf from a finite u, curve knots hit exactly, non-finite inputs.

Instantiations of waveshaper_kernel<T, LP, STREAM> and the cases that launch them (tests/waveshaper_cases.py): one-shot float32
LP = b: the two EQUAL cases of bucket b at L = 2, 4, 8 (A) plus the unequal pairs (LP 8: (1, 64 L), (3 L + 1, 40 L); 48:
(40 L, 3 L + 2); 64: (64 L - 1, 2); 72: (64 L, 1)); one-shot float64 LP = b: the two EQUAL cases of bucket b at one L (A) and the
same unequal pairs; stream, either dtype, LP = b: the smallest tap count of bucket b (B, one L per dtype) and the unequal pairs
at L = 4.  Geometry comes from the plan queries; the largest fraction of the bound is printed per (bucket, dtype)."""
import numpy as np
import pytest
import torch

from tests import resample_reference as RR
from tests import waveshaper_cases as C
from tests import waveshaper_reference as R
from tests.gpu_common import DEV, ext
from tests.test_gpu_stream_waveshaper import same_bits
from torchfx_amd import waveshape

pytestmark = pytest.mark.gpu

IDS = C.DT_ID.get
WORST = {}
THREE_TILES = {torch.float32: C.Case(8, 512, 512), torch.float64: C.Case(2, 128, 128)}


def host(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def params(dtype, kw):
    return R.params(C.NP[dtype], **kw)


def forward(x, L, shape, curve, par, hu, hd):
    """The low-level one-shot op: x a device tensor, the curve and the taps numpy arrays."""
    cv = None if curve is None else host(np.asarray(curve)).to(x.dtype)
    return ext().waveshaper_forward(x, L, shape, cv, *par, host(hu), host(hd))


def forward_np(shape, par, curve=None):
    """numpy in, numpy out: what tests/waveshaper_cases.run_probe calls."""
    return lambda x, L, hu, hd: forward(host(x).to(DEV), L, shape, curve, par, hu, hd).cpu().numpy()


def a_cases():
    return [(dt, c) for dt in C.DTYPES for c in C.equal_cases(dt) + C.UNEQUAL]


@pytest.mark.parametrize("dtype, c", a_cases(), ids=lambda v: IDS(v) or C.case_id(v))
def test_every_bucket_and_unequal_pair_stays_within_the_bound(dtype, c):
    g = C.geometry(*c, dtype)
    equal = c.nh_up == c.nh_dn
    hu, hd = C.stage_taps(c, dtype)
    lengths = [C.two_tile_length(g)] + ([C.two_tile_length(g, 3)] if THREE_TILES[dtype] == c else [])
    for T in lengths:
        xh = C.signal(3, T, 7, dtype)
        x = host(xh).to(DEV)
        assert ext().waveshaper_plan_info(T, c.L, c.nh_up, c.nh_dn, 0, dtype)["tiles"] == (3 if T > lengths[0] else 2)
        for name, kw in (("hard", C.KW_HARD), (C.soft_shape(c), C.KW_SOFT)):
            shape, curve = C.shape_args(name)
            y = forward(x, c.L, shape, curve, params(dtype, kw), hu, hd)
            frac = R.check(y.cpu().numpy(), xh, c.L, hu, hd, g["Lp_up"], g["Lp_dn"], shape,
                           what=f"{C.case_id(c)} {IDS(dtype)} LP={g['bucket']} I0={g['I0']} {name} T={T}", curve=curve, **kw)
            key = ("equal" if equal else "unequal", g["bucket"], IDS(dtype))
            WORST[key] = max(WORST.get(key, 0.0), frac)
            if equal:
                pub = waveshape(x, None if curve is not None else shape, oversample=c.L, curve=curve, window=C.window_of(c, dtype), **kw)
                assert torch.equal(pub, y), (c, name, T)
    print("largest fraction of the bound so far:", {k: round(v, 3) for k, v in sorted(WORST.items())})


def stream_run(x, L, shape, curve, par, hu, hd, sizes, D):
    """A chunk loop over the low-level stream op as its docstring has it: the history and the stream position go from call to
    call, and the tail is a chunk with T = D, n_in = 0.  Returns the stream's outputs [rows, T]."""
    E = ext()
    cv = None if curve is None else host(np.asarray(curve)).to(x.dtype)
    tu, td = host(hu), host(hd)
    hist, consumed, outs, n = None, 0, [], x.shape[-1]
    for k in list(sizes) + [n]:
        k = min(k, n - consumed)
        y, hist = E.waveshaper_stream_forward(x[..., consumed:consumed + k].contiguous(), hist, consumed, L, shape, cv, *par, tu, td)
        assert y.shape[-1] == k
        outs.append(y)
        consumed += k
    assert consumed == n
    y, _ = E.waveshaper_stream_forward(torch.zeros(*x.shape[:-1], D, dtype=x.dtype, device=x.device), hist, consumed, L, shape, cv,
                                       *par, tu, td, n_in=0)
    out = torch.cat(outs + [y], dim=-1)
    assert out.shape[-1] == n + D and not out[..., :D].any()             # the outputs before the stream's start are zeros
    return out[..., D:]


def b_cases():
    return [(dt, c) for dt in C.DTYPES for c in C.smallest_cases(dt) + [u for u in C.UNEQUAL if u.L == 4]]


@pytest.mark.parametrize("dtype, c", b_cases(), ids=lambda v: IDS(v) or C.case_id(v))
def test_stream_chunks_have_the_bits_of_the_one_shot_call(dtype, c):
    g = C.geometry(*c, dtype)
    D, Hs, N = g["latency"], g["history"], g["tile"]
    T = 3 * N + 100
    x = host(C.signal(2, T, 11, dtype)).to(DEV)
    hu, hd = C.stage_taps(c, dtype)
    shape, curve = C.shape_args(C.soft_shape(c))
    par = params(dtype, C.KW_SOFT)                                       # dry = 0.7: the stream's dry sample comes from the window
    ref = forward(x, c.L, shape, curve, par, hu, hd)
    sizes = [1, D - 1, D, D + 1, Hs, 0, 512, 513, N - 1, N + 1]
    runs, left = [[]], T                                                 # as many streams as it takes to run every size in full
    for k in sizes:
        if k > left:
            runs.append([])
            left = T
        runs[-1].append(k)
        left -= k
    assert sum(len(r) for r in runs) == len(sizes) and len(runs) <= 2
    for r in runs:
        got = stream_run(x, c.L, shape, curve, par, hu, hd, r, D)
        assert got.shape == ref.shape and same_bits(got, ref), (c, r, int((got != ref).sum()))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=IDS)
@pytest.mark.parametrize("p", C.PROBES, ids=C.probe_id)
def test_exact_tap_probes(p, dtype):
    seen, clipped = C.run_probe(p, dtype, forward_np("hard", params(dtype, {})))
    assert seen == set(range(p.nh)) and (clipped or p.stage == "dn")


D_CASES = [C.Case(2, 1, 1), C.Case(4, 128, 128), C.Case(8, 512, 512), C.Case(4, 1, 256), C.Case(8, 512, 1)]
D_KW = dict(drive_db=6.0, bias=0.1, mix=0.7)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=IDS)
@pytest.mark.parametrize("c", D_CASES, ids=C.case_id)
def test_non_finite_samples_poison_exactly_their_reach(c, dtype):
    """The assertions of test_gpu_waveshaper.test_a_nan_poisons_exactly_its_window; the plantings are rows of one launch."""
    g = C.geometry(*c, dtype)
    N, rb, ra = g["tile"], g["reach_before"], g["reach_after"]
    T = C.two_tile_length(g)
    base = C.signal(1, T, 9, dtype)[0]
    sites = (0, T - 1, N - 1, N)
    plant = [(i, bad) for i in sites for bad in (np.nan, np.inf, -np.inf)]
    x = np.stack([base] * (len(plant) + len(sites)))
    for r, (i, bad) in enumerate(plant):
        x[r, i] = bad
    for k, i in enumerate(sites):
        x[len(plant) + k, i] = 0.0
    hu, hd = C.stage_taps(c, dtype)
    y = forward(host(x).to(DEV), c.L, "tanh", None, params(dtype, D_KW), hu, hd).cpu().numpy()
    assert not np.isnan(y[len(plant):]).any()
    for r, (i, bad) in enumerate(plant):
        y0 = y[len(plant) + sites.index(i)]
        want = np.zeros(T, bool)
        want[max(0, i - rb):min(T, i + ra + 1)] = True
        assert np.array_equal(np.isnan(y[r]), want), (i, bad, np.flatnonzero(np.isnan(y[r]) != want)[:8])
        assert np.array_equal(y[r][~want], y0[~want]), (i, bad)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=IDS)
@pytest.mark.parametrize("c", D_CASES, ids=C.case_id)
def test_an_overflow_from_finite_input_poisons_the_decimators_reach_of_one_sample(c, dtype):
    """h_up = a single tap of 2 at the centre: u[p L] = 2 * (the largest finite value) = Inf and every other up-sampled value is
    finite, so the NaNs are the outputs whose decimator window holds up-sampled index p L, zero-padded taps counted."""
    L, ndt = c.L, C.NP[dtype]
    nh_up = 2 * L + 1
    g = C.geometry(L, nh_up, c.nh_dn, dtype)
    N, T = g["tile"], C.two_tile_length(g)
    base = C.signal(1, T, 13, dtype)[0]
    sites = (0, N - 1, N, T - 1)
    x = np.stack([base] * (2 * len(sites)))
    for r, p in enumerate(sites):
        x[r, p], x[len(sites) + r, p] = np.finfo(ndt).max, 0.0
    hu, hd = C.delta(nh_up, L, 2.0, dtype), C.taps(c.nh_dn, dtype)
    y = forward(host(x).to(DEV), L, "tanh", None, params(dtype, D_KW), hu, hd).cpu().numpy()
    q = ext().resample_plan_info(T * L, 1, L, c.nh_dn, dtype)
    want = RR.reach_mask(T * L, T, 1, L, q["n_pre_remove"], q["Lp"], [(r, p * L) for r, p in enumerate(sites)], rows=len(sites))
    assert want.any(axis=1).all() and not np.isnan(y[len(sites):]).any()
    for r, p in enumerate(sites):
        assert np.array_equal(np.isnan(y[r]), want[r]), (p, np.flatnonzero(np.isnan(y[r]) != want[r])[:8])
        assert np.array_equal(y[r][~want[r]], y[len(sites) + r][~want[r]]), p


def edge_inputs(ndt):
    one, big, f = ndt(1), np.finfo(ndt).max, np.finfo(ndt)
    vals = [0.0, -0.0, f.smallest_subnormal, -f.smallest_subnormal, one, -one, np.nextafter(one, ndt(2)), np.nextafter(one, ndt(0)),
            np.nextafter(-one, ndt(-2)), np.nextafter(-one, ndt(0)), big, -big, 0.5, -0.25]
    return np.array(vals, ndt)


def edge_stages(L, dtype):
    """(h_up, h_dn, Lp_up, Lp_dn): nothing for L = 1, one tap of 1 per stage for L = 2."""
    if L == 1:
        return None, None, 0, 0
    g = C.geometry(L, 1, 1, dtype)
    return C.delta(1, 0, 1.0, dtype), C.delta(1, 0, 1.0, dtype), g["Lp_up"], g["Lp_dn"]


@pytest.mark.parametrize("dtype", C.DTYPES, ids=IDS)
@pytest.mark.parametrize("L", [1, 2])
def test_transfer_function_edges(L, dtype):
    ndt = C.NP[dtype]
    hu, hd, Lp_up, Lp_dn = edge_stages(L, dtype)
    x = np.stack([edge_inputs(ndt), -edge_inputs(ndt)[::-1]])
    for drive_db in (0.0, 20.0 * np.log10(2.0)):                         # drive = 2: v = +-Inf from the largest finite u
        par = params(dtype, dict(drive_db=drive_db))
        assert par == (2.0 if drive_db > 0 else 1.0, 0.0, 0.0, 1.0)
        y = forward(host(x).to(DEV), L, "hard", None, par, hu, hd).cpu().numpy()
        with np.errstate(over="ignore"):                                  # the float64 reference of a float64 signal: v = Inf too
            want = R.ref(x, L, hu, hd, "hard", drive_db=drive_db, wide=dtype == torch.float64).astype(ndt)
        assert np.array_equal(y, want), (drive_db, y, want)
        huge = np.abs(x) == np.finfo(ndt).max
        assert huge.sum() == 4 and np.array_equal(y[huge], np.sign(x[huge]))
        for shape in ("cubic", "tanh"):
            y = forward(host(x).to(DEV), L, shape, None, par, hu, hd).cpu().numpy()
            with np.errstate(over="ignore"):
                R.check(y, x, L, hu, hd, Lp_up, Lp_dn, shape, what=f"edges {shape} L={L} {IDS(dtype)} drive={par[0]}", drive_db=drive_db)
            # the bound is relative to |v| and says nothing at the largest values: f(+-huge) = +-1, within E_SHAPE u for tanh
            slack = R.e_shape(shape, ndt) * np.finfo(ndt).eps / 2 if shape == "tanh" else 0.0
            assert (np.abs(y[huge] - np.sign(x[huge])) <= slack).all(), (shape, drive_db, y[huge])
    bad = np.zeros((1, 16), ndt)
    bad[0, [0, 5, 10, 15]] = np.nan, np.inf, -np.inf, 0.5
    rb, ra = (0, 0) if L == 1 else (C.geometry(L, 1, 1, dtype)[k] for k in ("reach_before", "reach_after"))
    want = np.zeros(16, bool)
    for i in (0, 5, 10):
        want[max(0, i - rb):i + ra + 1] = True
    assert not want[15]
    for shape, curve in (("hard", None), ("cubic", None), ("tanh", None), ("curve", C.CURVE5)):
        y = forward(host(bad).to(DEV), L, shape, curve, params(dtype, {}), hu, hd).cpu().numpy()
        assert np.array_equal(np.isnan(y[0]), want) and y[0, 15] != 0, (shape, y)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=IDS)
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("n", [2, 3, 5, 4095, 4096])
def test_curve_knots_and_ends_are_read_exactly(n, L, dtype):
    ndt = C.NP[dtype]
    hu, hd, _, _ = edge_stages(L, dtype)
    curve = C.dyadic_curve(n)
    assert np.array_equal(curve.astype(np.float32), curve) and curve[0] != curve[1] and curve[-1] != curve[-2]
    big = np.finfo(ndt).max
    v = [-1.0, 1.0, -1.5, 1.5, -big, big, np.nextafter(ndt(-1), ndt(-2)), np.nextafter(ndt(1), ndt(2))]
    want = [curve[0], curve[-1]] * 4
    if ((n - 1) & (n - 2)) == 0:                                           # n - 1 a power of two: every knot is a dyadic v
        v += [-1.0 + 2.0 * k / (n - 1) for k in range(n)]
        want += list(curve)
    x = np.array([v], ndt)
    c0 = R.c0_of(ndt, "curve", 0.0, curve)
    y = forward(host(x).to(DEV), L, "curve", curve, params(dtype, {}), hu, hd).cpu().numpy()
    assert np.array_equal(y[0] + ndt(c0), np.array(want, ndt)), (n, y[0] + ndt(c0), want)
    assert np.array_equal(y, R.ref(x, L, hu, hd, "curve", curve=curve, wide=dtype == torch.float64).astype(ndt))
