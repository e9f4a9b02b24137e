"""The modulated delay line with feedback as a per-sample float64 loop (include/torchfx_hip.h,
tfx_modulated_delay_feedback_forward), the cases the host and device tests share, and the bound they hold the product to.
The bound is derived, not tuned: one pass through the voices is the feed-forward effect applied to the line w, whose error is
tests/modulation_reference.py's tol with E = max|w_ref| of the row; it enters w scaled by |feedback| and comes back through an
interpolant of norm L sum|g_v| (L = 1 linear, 1.25 cubic): a geometric series in rho = |feedback| L sum|g_v| < 1, so
|y - ref| <= tol / (1 - rho), plus 2^-24 |ref| for float32 results.

The cases are chosen from the plan (csrc/modulation.hip, mod_fb_plan), and PLANS holds what the plan must report for each, so
that a change of the geometry fails the case's first assertion instead of silently testing something else."""
import functools
import math

import numpy as np

from tests import modulation_reference as R

FS = 8000
T = 1500
DRY, SPREAD, POSITION = 0.7, 0.25, 12345
# name: ((delay, depth, rate, phase, gain) rows for linear interpolation -- cubic adds its one sample to every delay --, feedback,
# the block B = floor(min(delay - depth)) the plan must report)
TABLES = {
    "B1": ([(3.5, 2.25, 23.0, 0.0, 0.6)], 0.9, 1),                      # fully serial, 64 rows per wave
    "B5": ([(8.75, 3.5, 17.0, 0.1, -0.7)], 0.8, 5),                     # 12 rows per wave; 5 batch items leave a remainder
    "B47": ([(70.5, 23.25, 11.0, 0.4, 0.6)], -0.9, 47),                 # one row per wave, 17 idle lanes
    "B150": ([(170.3, 20.1, 29.0, 0.7, 0.5)], 0.95, 150),               # sub-blocks of 64, the last one short
    "two": ([(12.5, 4.25, 19.0, 0.0, 0.5), (40.0, 9.5, 7.0, 0.3, -0.4)], -0.8, 8),
    "B16": ([(20.5, 4.25, 13.0, 0.2, 0.6)], 0.9, 16),                   # a second packed wave (4 rows), the last wave with 1 row
    "B32": ([(40.5, 8.25, 11.0, 0.4, -0.6)], 0.9, 32),                  # the last packed size: waves of 2, 2, 1
    "B33": ([(41.5, 8.25, 11.0, 0.4, 0.6)], -0.9, 33),                  # the first unpacked size, 31 idle lanes
    "B64": ([(70.5, 6.25, 19.0, 0.1, 0.6)], 0.9, 64),                   # exactly one full sub-block
    "B128": ([(140.5, 12.25, 17.0, 0.6, 0.5)], 0.95, 128),              # two full sub-blocks
    "B129": ([(141.5, 12.25, 17.0, 0.6, -0.5)], 0.95, 129),             # a third sub-block of one lane
    # packing cut by LDS: 12 rows would fit the lanes, 7 rings of 1024 + 5 fit 64 KiB: waves of 7 and 2, lanes 35..63 idle
    "B5long": ([(8.75, 3.5, 17.0, 0.1, -0.5), (1000.0, 10.5, 7.0, 0.3, 0.3)], 0.8, 5),
    # MD_MAXV voices in registers
    "V8": ([(12.5 + 9.0 * v, 4.25, r, v / 8.0, 0.1 if v % 2 == 0 else -0.1)
            for v, r in enumerate((19.0, 7.0, 13.0, 29.0, 5.0, 23.0, 11.0, 17.0))], 0.9, 8),
    # three voices in the unpacked single-sub-block regime
    "V3": ([(50.5, 6.25, 13.0, 0.0, 0.3), (70.0, 9.5, 7.0, 0.3, -0.3), (90.25, 12.5, 5.0, 0.6, 0.25)], 0.9, 44),
}
# The one case whose per-sample loop is long: it runs one interpolation / LFO pair (LONG_PAIR) and stays out of the full grid.
# rows_per_wave falls back to 1 with B <= 32 (one active lane), the ring is the longest and the launch takes all 64 KiB of LDS.
LONG_TABLES = {"B1long": ([(3.5, 2.25, 23.0, 0.0, 0.5), (5000.0, 10.5, 7.0, 0.3, 0.3)], 0.8, 1)}
LONG_PAIR = ("cubic", "sine")
# name: (batch, length) where they are not (5, T); B1long is long enough for the long voice to be heard and the 8192 ring to wrap
SHAPES = {"B64": (3, T), "B128": (3, T), "B129": (3, T), "B5long": (9, T), "B1long": (2, 8192 + 300)}
# name: what modulated_delay_feedback_plan_info must say for the case's [batch, 2, length], computed by hand from mod_fb_plan;
# the same for both interpolations
PLANS = {
    "B16": dict(block=16, rows_per_wave=4, ring=64, lds_bytes=4 * 80 * 8, workgroups=2 * 2),
    "B32": dict(block=32, rows_per_wave=2, ring=128, workgroups=2 * 3),
    "B33": dict(block=33, rows_per_wave=1),
    "B64": dict(block=64, rows_per_wave=1),
    "B128": dict(block=128),
    "B129": dict(block=129),
    "B5long": dict(block=5, ring=1024, rows_per_wave=7, lds_bytes=7 * 1029 * 8, workgroups=2 * 2),
    "B1long": dict(block=1, ring=8192, rows_per_wave=1, lds_bytes=65536),
    "V8": dict(block=8, rows_per_wave=8),
    "V3": dict(block=44, rows_per_wave=1, workgroups=2 * 5),
}


def table(name):
    """(voices for linear interpolation, feedback, block) of a case of either table."""
    return TABLES[name] if name in TABLES else LONG_TABLES[name]


def shape_of(name):
    """(batch, length) of a case."""
    return SHAPES.get(name, (5, T))


def voices(name, interpolation):
    pad = 1.0 if interpolation == "cubic" else 0.0
    return [(b + pad, d, r, p, g) for b, d, r, p, g in table(name)[0]]


def plan(name, interpolation, batch=None, length=None):
    """The plan's answer (host-only) for the case's shape, or for another batch / length."""
    from torchfx_amd import torchfx_ext as E

    b, n = shape_of(name)
    rows = [(d, w, r / FS, p, g) for d, w, r, p, g in voices(name, interpolation)]
    return E.modulated_delay_feedback_plan_info(n if length is None else length, rows, table(name)[1], batch=b if batch is None else batch,
                                                channels=2, interpolation=interpolation)


def assert_plan(name, interpolation):
    """The case reaches what it was chosen for: the block of the table and, for the cases of PLANS, the geometry."""
    q = plan(name, interpolation)
    want = dict(PLANS.get(name, {}), block=table(name)[2])
    got = {k: q[k] for k in want}
    assert got == want, f"{name} {interpolation}: the plan says {got}, the case was built for {want}"
    return q


def rho_of(voice_rows, feedback, interpolation):
    return abs(feedback) * sum(abs(v[4]) for v in voice_rows) * (1.25 if interpolation == "cubic" else 1.0)


def feedback_ref(x, fs, table, feedback, dry=1.0, spread=0.0, shape="sine", interpolation="linear", position=0):
    """x [B, C, T] -> (y, w), both unrounded float64 [B, C, T]."""
    xr = np.asarray(x, dtype=np.float64)
    batch, C, n_samples = xr.shape
    rows = R.voice_rows(table, fs)
    y, w = np.empty_like(xr), np.zeros_like(xr)
    zero = np.zeros(batch)
    for c in range(C):
        offs = [(p + float(c) * spread) - math.floor(p + float(c) * spread) for _, _, _, p, _ in rows]
        for j in range(n_samples):
            r = 0.0
            for (base, depth, inc, _, gain), off in zip(rows, offs):
                i, f = R.delay_at(position + j, base, depth, inc, off, shape)
                at = lambda m: w[:, c, m] if m >= 0 else zero                       # noqa: E731
                m = j - i
                if interpolation == "linear":
                    wd = at(m) + f * (at(m - 1) - at(m))
                else:
                    wd = ((-f * (f - 1.0) * (f - 2.0) / 6.0) * at(m + 1) + ((f + 1.0) * (f - 1.0) * (f - 2.0) / 2.0) * at(m)
                          + (-(f + 1.0) * f * (f - 2.0) / 2.0) * at(m - 1) + ((f + 1.0) * f * (f - 1.0) / 6.0) * at(m - 2))
                r = r + gain * wd
            w[:, c, j] = xr[:, c, j] + feedback * r
            y[:, c, j] = dry * xr[:, c, j] + r
    return y, w


@functools.lru_cache(maxsize=None)
def case(name, interpolation, lfo):
    """(x float32 [batch, 2, length] with float32-representable values, so one reference serves both dtypes; y_ref; w_ref),
    read-only.  The loop's result is finite and the case's rho < 1, or the bound would mean nothing."""
    batch, n = shape_of(name)
    x = np.random.default_rng(len(name)).uniform(-1.0, 1.0, (batch, 2, n)).astype(np.float32)
    assert rho_of(voices(name, interpolation), table(name)[1], interpolation) < 1.0, f"{name} {interpolation}: rho >= 1"
    y, w = feedback_ref(x, FS, voices(name, interpolation), table(name)[1], DRY, SPREAD, lfo, interpolation, POSITION)
    assert np.isfinite(y).all() and np.isfinite(w).all(), f"{name} {interpolation} {lfo}: the reference is not finite"
    for a in (x, y, w):
        a.setflags(write=False)
    return x, y, w


SHARES = {}                                                    # dtype name -> largest share of the bound seen by check_bound


def check_bound(got, ref, w, fs, voice_rows, dry, feedback, interpolation, what):
    """got within tol / (1 - rho) (+ 2^-24 |ref| for float32) of ref, w the reference's line of the same rows."""
    got = np.asarray(got)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    tol = R.tolerance(w, fs, voice_rows, dry) / (1.0 - rho_of(voice_rows, feedback, interpolation))
    bound = tol + (2.0 ** -24 * np.abs(ref) if got.dtype == np.float32 else 0.0)
    dev = np.abs(got.astype(np.float64) - ref)
    share = float((dev / bound).max()) if dev.size else 0.0
    print(f"{what}: largest deviation {float(dev.max()) if dev.size else 0.0:.3e}, largest share of the bound {share:.3f}")
    if np.isfinite(share):
        SHARES[got.dtype.name] = max(SHARES.get(got.dtype.name, 0.0), share)
    assert np.isfinite(share) and share <= 1.0, f"{what}: the deviation is {share:.3f} of the bound"


def check(got, name, interpolation, lfo, what, rows=slice(None), length=None, ref=None):
    """got (rows `rows`, first `length` samples of the case) within the bound of the loop's result (or of `ref`)."""
    _, y, w = case(name, interpolation, lfo)
    length = y.shape[-1] if length is None else length
    ref = y[rows, :, :length] if ref is None else ref
    check_bound(got, ref, w[rows], FS, voices(name, interpolation), DRY, table(name)[1], interpolation, what)
