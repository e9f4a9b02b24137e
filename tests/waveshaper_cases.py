"""The cases of the waveshaper's edge tests (tests/test_gpu_waveshaper_edges.py, tests/test_waveshaper_cases_host.py): tap counts
(nh_up, nh_dn) that reach every register-tap bucket of waveshaper_kernel<T, LP, STREAM> with stages of equal length, stages of
unequal length (the only way to a tile origin I0 != 0), deliberately asymmetric taps, the signals, and the exact tap probes.
NumPy and the host-only plan queries of the C ABI: nothing here needs a device.

Geometry is looked up (`geometry`) and compared with the tables by tests/test_waveshaper_cases_host.py, never assumed.  With
Lp_up = ceil((nh_up + 1 + post_pad) / L) a bucket b holds nh in [first, b L - 1]; bucket 72 holds Lp_up = 65 alone, which only
nh = 64 L gives.

The probes.  With the hard clipper, drive = 1, bias = 0, dry = 0, wet = 1 and one stage a single tap `delta(2 L + 1, L + s)`,
an impulse a at input i gives, in tests/resample_reference.py's indexing (half = (nh - 1) // 2),

    up-stage probe    h_dn = delta:  z[m] = clip(a h_up[(m - i) L - s + half_up])        where m L - s lies in [0, T L)
    down-stage probe  h_up = delta:  z[m] = clip(a) h_dn[(m - i) L - s + half_dn]        where i L + s lies in [0, T L)

and 0 where the tap does not exist: one exact product per output (a is a power of two), so the outputs are the probed stage's
taps themselves, in order, and a reversed, shifted or swapped tap array cannot pass `np.array_equal`.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import resample_reference as RR
from tests import waveshaper_reference as R

NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = [torch.float32, torch.float64]
DT_ID = {torch.float32: "f32", torch.float64: "f64"}
BUCKETS = (8, 16, 24, 32, 48, 64, 72)
LS = (2, 4, 8)
CURVE5 = np.array([-0.9, -0.2, 0.05, 0.4, 0.8])
KW_HARD = dict(drive_db=9.0)
KW_SOFT = dict(drive_db=9.0, bias=0.15, mix=0.3, output_db=-6.0)
SOFT = ("tanh", "cubic", "curve5")


def ext():
    from torchfx_amd import torchfx_ext
    return torchfx_ext


def bucket_of(Lp):
    return next(b for b in BUCKETS if Lp <= b)


def nh_range(L, bucket):
    """The nh (both stages alike) that land in `bucket`: (smallest, largest)."""
    k = BUCKETS.index(bucket)
    if bucket == 72:
        return 64 * L, 64 * L
    return (BUCKETS[k - 1] * L if k else 1), bucket * L - 1


@functools.lru_cache(maxsize=None)
def geometry(L, nh_up, nh_dn, dtype=torch.float32, T=1000):
    """What the two plan queries say about stages of nh_up and nh_dn taps: Lp_up, the kernel's register bucket, Lp_dn, the tile,
    the reach, the tile's origin I0 = Lp_up - 1 - reach_after (counted from the tile's first output), the stream's latency and
    history.  What the two plans must agree on is asserted."""
    E = ext()
    q = E.waveshaper_plan_info(T, L, nh_up, nh_dn, 0, dtype)
    s = E.waveshaper_stream_plan_info(T, L, nh_up, nh_dn, 0, dtype)
    assert s["tile"] == q["tile"] and s["latency"] == q["reach_before"], (q, s)
    assert s["history"] == q["reach_before"] + q["reach_after"] and s["lds_bytes"] == q["lds_bytes"], (q, s)
    return dict(Lp_up=q["taps_up"], bucket=bucket_of(q["taps_up"]), Lp_dn=q["taps_dn"], tile=q["tile"],
                reach_before=q["reach_before"], reach_after=q["reach_after"], I0=q["taps_up"] - 1 - q["reach_after"],
                latency=s["latency"], history=s["history"])


Case = namedtuple("Case", "L nh_up nh_dn")
# (L, bucket, nh): the smallest nh of the bucket (the most zero-padded register taps) and the largest (Lp_up == bucket)
EQUAL = [(L, b, nh) for L in LS for b in BUCKETS for nh in sorted(set(nh_range(L, b)))]
UNEQUAL = [Case(L, a, b) for L in LS for a, b in ((1, 64 * L), (64 * L, 1), (64 * L - 1, 2), (3 * L + 1, 40 * L), (40 * L, 3 * L + 2))]


def equal_cases(dtype):
    """float32: every EQUAL case; float64: every bucket's two cases at one L, rotating L over the buckets."""
    if dtype == torch.float32:
        return [Case(L, nh, nh) for L, b, nh in EQUAL]
    return [Case(L, nh, nh) for L, b, nh in EQUAL if L == LS[BUCKETS.index(b) % 3]]


def smallest_cases(dtype):
    """Every bucket's smallest nh; float32 rotates L one way over the buckets, float64 the other."""
    off = 0 if dtype == torch.float32 else 1
    return [Case(L, nh_range(L, b)[0], nh_range(L, b)[0]) for k, b in enumerate(BUCKETS) for L in [LS[(k + off) % 3]]]


def case_id(c):
    return "L%d-up%d-dn%d" % tuple(c)


def soft_shape(c):
    """The second shape of a case in section A: tanh, cubic or curve5, rotating."""
    return SOFT[(c.L + c.nh_up + c.nh_dn) % 3]


def taps(n, dtype, seed=0):
    """A deliberately asymmetric low-pass of n taps in `dtype`, sum 1: a Hann shape times the ramp 1 + 0.5 linspace(-1, 1, n),
    times 1 + 0.02 uniform(-1, 1) drawn from `seed`.  The decimator runs it as it is, the up-sampler runs L times it (exact: L
    is a power of two).  n = 1 gives [1]."""
    if n == 1:
        return np.ones(1, NP[dtype])
    h = np.hanning(n + 2)[1:-1] * (1.0 + 0.5 * np.linspace(-1.0, 1.0, n))
    h = h * (1.0 + 0.02 * np.random.default_rng(1000 * seed + n).uniform(-1.0, 1.0, n))
    return (h / h.sum()).astype(NP[dtype])


def stage_taps(c, dtype):
    """(h_up, h_dn) of a case as the kernel takes them, numpy in the signal's dtype."""
    return NP[dtype](c.L) * taps(c.nh_up, dtype), taps(c.nh_dn, dtype)


def window_of(c, dtype):
    """The float64 tap array that the public waveshape(..., window=) turns into `stage_taps` of a case with equal stages: the
    library casts it to the dtype for the decimator and L times it for the up-sampler."""
    assert c.nh_up == c.nh_dn
    return taps(c.nh_up, dtype).astype(np.float64)


def delta(n, at, value=1.0, dtype=torch.float32):
    h = np.zeros(n, NP[dtype])
    h[at] = value
    return h


def two_tile_length(g, tiles=2):
    """tile + reach_before + 9 made odd: two tiles, the second short; `tiles` = 3: 2 tile + reach_before + 3."""
    T = g["tile"] + g["reach_before"] + 9 if tiles == 2 else 2 * g["tile"] + g["reach_before"] + 3
    return T | 1


def signal(rows, T, seed, dtype):
    """Per row a sine of amplitude 0.8 slow enough to pass the longest filter (periods 311, 173 and 97 samples, random phase)
    plus uniform(-0.1, 0.1): at 9 dB of drive the clipper is at work whatever the filters leave of the noise."""
    g = np.random.default_rng(seed)
    t = np.arange(T)
    per = np.array([311.0, 173.0, 97.0, 251.0, 131.0])[np.arange(rows) % 5]
    x = 0.8 * np.sin(2 * np.pi * (t[None, :] / per[:, None] + g.uniform(0, 1, (rows, 1)))) + g.uniform(-0.1, 0.1, (rows, T))
    return x.astype(NP[dtype])


def shape_args(shape):
    """(the kernel's shape name, the curve or None) of "hard", "tanh", "cubic", "curve5"."""
    return ("curve", CURVE5) if shape == "curve5" else (shape, None)


# ---- the exact tap probes ---------------------------------------------------------------------------------------------------
PROBE_AMPS = (256.0, -0.5, 2.0, -256.0, 1.0)            # powers of two; 256 |h| > 1 at the taps' middle for every nh <= 512
Probe = namedtuple("Probe", "stage L nh")                # stage "up": h_up = L taps(nh); "dn": h_dn = taps(nh)
UP_PROBES = [Probe("up", LS[k % 3], nh_range(LS[k % 3], b)[1]) for k, b in enumerate(BUCKETS)]
DN_PROBES = [Probe("dn", 2, 5), Probe("dn", 4, 160), Probe("dn", 8, 512)]          # 2 L + 1, 40 L, 64 L
PROBES = UP_PROBES + DN_PROBES


def probe_id(p):
    return "%s-L%d-nh%d" % tuple(p)


def probe_case(p):
    return Case(p.L, p.nh, 2 * p.L + 1) if p.stage == "up" else Case(p.L, 2 * p.L + 1, p.nh)


def probe_taps(p, s, dtype):
    """(h_up, h_dn) of probe p at offset s in [-(L - 1), L - 1]."""
    d = delta(2 * p.L + 1, p.L + s, 1.0, dtype)
    if p.stage == "up":
        return NP[dtype](p.L) * taps(p.nh, dtype, 3), d
    return d, taps(p.nh, dtype, 3)


def probe_sites(g, T):
    return (0, (g["tile"] // 2) | 1, g["tile"] - 1, g["tile"], T - 1)


def probe_input(p, dtype):
    """One row per impulse site (0, a mid position, tile - 1, tile, T - 1), so that no output sees two impulses."""
    g = geometry(*probe_case(p), dtype)
    T = two_tile_length(g)
    sites = probe_sites(g, T)
    return np.stack([RR.impulses(T, [i], [a], NP[dtype]) for i, a in zip(sites, PROBE_AMPS)]), sites


def probe_closed_form(p, s, dtype, T, sites):
    """The expected rows from the closed form of the module docstring, and the set of probed-tap indices they read."""
    L = p.L
    hu, hd = probe_taps(p, s, dtype)
    h = hu if p.stage == "up" else hd
    half = (len(h) - 1) // 2
    m = np.arange(T, dtype=np.int64)
    out, seen = np.zeros((len(sites), T), NP[dtype]), set()
    for r, (i, a) in enumerate(zip(sites, PROBE_AMPS)):
        k = (m - i) * L - s + half
        ok = (k >= 0) & (k < len(h))
        ok &= ((m * L - s >= 0) & (m * L - s < T * L)) if p.stage == "up" else (0 <= i * L + s < T * L)
        a = NP[dtype](a)
        out[r, ok] = np.clip(a * h[k[ok]], -1, 1) if p.stage == "up" else np.clip(a, -1, 1) * h[k[ok]]
        seen |= set(k[ok].tolist())
    return out, seen


def run_probe(p, dtype, forward, wrong=None):
    """The probe's assertion: for every s, forward(x, L, h_up, h_dn) (numpy in, numpy out) must be np.array_equal to the
    reference of the right taps cast to the dtype.  `wrong` maps (h_up, h_dn) to what `forward` is given instead (the host's
    discrimination test).  Returns (the tap indices seen, whether some expected output clipped to exactly +-1)."""
    x, sites = probe_input(p, dtype)
    wide = dtype == torch.float64
    seen, clipped = set(), False
    for s in range(-(p.L - 1), p.L):
        hu, hd = probe_taps(p, s, dtype)
        r = R.ref(x, p.L, hu, hd, "hard", wide=wide)
        want = r.astype(NP[dtype])
        assert np.array_equal(want.astype(r.dtype), r), (p, s, "an expected output is not representable")
        closed, k = probe_closed_form(p, s, dtype, x.shape[-1], sites)
        assert np.array_equal(closed, want), (p, s, "the closed form is not the reference")
        seen |= k
        clipped |= bool((np.abs(want) == 1).any())
        got = forward(x, p.L, *(wrong(hu, hd) if wrong else (hu, hd)))
        assert got.dtype == want.dtype and np.array_equal(got, want), (
            p, s, np.argwhere(got != want)[:4].tolist(), got[got != want][:4], want[got != want][:4])
    return seen, clipped


# ---- section E: dyadic curves -----------------------------------------------------------------------------------------------
def dyadic_curve(n):
    """n table values that are multiples of 2^-16 in (-1, 1), neither odd nor monotone and steep enough at both ends that
    neighbours differ at n = 4096: differences and sums of two of them, and of one and f(0), are exact in float32."""
    t = np.linspace(-1.0, 1.0, n)
    return np.round((0.5 * t + 0.25 * t * t + 0.2 * np.sin(3.0 * t)) * 65536.0) / 65536.0
