"""The cases of the detector tests (tests/test_gpu_detector.py, tests/test_gpu_detector_truepeak.py,
tests/test_detector_cases_host.py): interpolators, chosen by their length nh, that reach every register-tap bucket of the `up`x
chain (true_peak_kernel, limiter_kernel) and every split of a position's phases between sample i - 1 and sample i
(rem = n_pre_remove mod up); their random taps; the signals; and the float64 statements the tests compare against.  NumPy and
the host-only plan functions of the C ABI: nothing here needs a device.

Geometry is looked up (`geometry`) and compared with the table, never assumed.  Bucket 72 holds Lp = 65 alone, which only
nh = 64 * up gives, and that length has rem = 0: there is no bucket-72 case with rem > 0 (`test_bucket_72_has_no_lo_phases`).
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import resample_reference as RR

NP = {torch.float32: np.float32, torch.float64: np.float64}
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
DTYPES = [torch.float32, torch.float64]
BUCKETS = (8, 16, 24, 32, 48, 64, 72)
TP_R = 16                                      # consecutive positions per thread of the chain
FS = 48000

# scale: the constant the uniform(-1, 1) taps are multiplied by for the limiter's tests, found once on the host (bisection to
# two digits) so that in the limiter's signal the interpolator's outputs own the maximum p[i] at about 95 % of the positions --
# 90 % or more is what the tests ask -- while |x[i]| and each of the 2 up outputs still own it at some position of every residue
# i mod 16.  seed: which draw of the taps; 0 unless that draw leaves an output that never owns p[i], or a (slot, phase) cell that
# owns no true-peak row's maximum (an 8-tap phase is easily shadowed by its neighbours).  tests/test_detector_cases_host.py
# asserts all of it; DESIGN.md section 4.11c lists the shares.
Case = namedtuple("Case", "up nh Lp bucket i_lo rem scale seed", defaults=(0,))
CASES = [
    Case(2, 15, 8, 8, 4, 0, 1.0), Case(2, 31, 16, 16, 8, 0, 0.52), Case(2, 41, 21, 24, 10, 1, 0.67),
    Case(2, 63, 32, 32, 16, 0, 0.33), Case(2, 95, 48, 48, 24, 0, 0.43), Case(2, 127, 64, 64, 32, 0, 0.37),
    Case(2, 128, 65, 72, 32, 0, 0.23), Case(2, 2, 2, 8, 0, 1, 1.0),
    Case(4, 28, 8, 8, 3, 2, 0.61, 2), Case(4, 61, 16, 16, 7, 3, 0.45), Case(4, 81, 21, 24, 10, 1, 0.43),
    Case(4, 83, 21, 24, 10, 2, 0.29), Case(4, 94, 24, 24, 11, 3, 0.36), Case(4, 127, 32, 32, 16, 0, 0.26),
    Case(4, 189, 48, 48, 23, 3, 0.26), Case(4, 191, 48, 48, 24, 0, 0.27), Case(4, 253, 64, 64, 31, 3, 0.19),
    Case(4, 255, 64, 64, 32, 0, 0.21), Case(4, 256, 65, 72, 32, 0, 0.18), Case(4, 3, 2, 8, 0, 2, 1.0),
    Case(8, 57, 8, 8, 3, 5, 0.46, 9), Case(8, 121, 16, 16, 7, 5, 0.3), Case(8, 161, 21, 24, 10, 1, 0.3),
    Case(8, 187, 24, 24, 11, 6, 0.25), Case(8, 255, 32, 32, 16, 0, 0.24), Case(8, 381, 48, 48, 23, 7, 0.19),
    Case(8, 511, 64, 64, 32, 0, 0.14), Case(8, 512, 65, 72, 32, 0, 0.17),
]
# One tap per phase (Lp = 2 counts SciPy's leading zero): every output is one product h[k] * x[i], so the phase with the largest
# tap owns every maximum and no choice of signal gives the others a turn.  These two run for bit equality and the bound only.
SINGLE_TAP = [k for k, c in enumerate(CASES) if c.Lp == 2]
FULL = [k for k, c in enumerate(CASES) if c.Lp > 2]


def case_id(c):
    return "up%d-nh%d-b%d-rem%d" % (c.up, c.nh, c.bucket, c.rem)


def find(up, nh):
    (c,) = [c for c in CASES if (c.up, c.nh) == (up, nh)]
    return c


def bucket_of(Lp):
    return next(b for b in BUCKETS if Lp <= b)


def ext():
    from torchfx_amd import torchfx_ext
    return torchfx_ext


def geometry(up, nh, dtype=torch.float32, A=1, H=1):
    """What the plan functions say about an `up`x interpolator of nh taps in a limiter of look-ahead A and hold H: Lp, the
    limiter's register bucket (from halo_left = A + H - 1 + LP - 1 - i_lo), the true-peak kernel's (the same table, from its
    own Lp), i_lo, rem, the tiles and the stream's latency and history.  Every redundancy between the four plans is asserted."""
    E = ext()
    tp = E.true_peak_plan_info(1, 1000, up, nh, dtype)
    lm = E.limiter_plan_info(1000, A, H, up, nh, dtype)
    st = E.limiter_stream_plan_info(512, A, H, up, nh, dtype)
    rs = E.resample_plan_info(1000, up, 1, nh, dtype)
    i_lo = lm["halo_right"] - A
    bucket = lm["halo_left"] - (A + H - 1) + 1 + i_lo
    rem = rs["n_pre_remove"] % up
    assert rs["n_pre_remove"] // up == i_lo and tp["Lp"] == lm["Lp"] == rs["Lp"], (tp, lm, rs)
    assert bucket == bucket_of(lm["Lp"]) and 0 <= i_lo <= bucket - 1, (bucket, lm)
    assert lm["tile"] == st["tile"] == 8193 - 2 * A - H
    return dict(Lp=lm["Lp"], bucket=bucket, tp_bucket=bucket_of(tp["Lp"]), i_lo=i_lo, rem=rem, tile=lm["tile"],
                tile_in=tp["tile_in"], halo_left=lm["halo_left"], halo_right=lm["halo_right"], latency=st["latency"],
                history=st["history"])


def check(c, dtype=torch.float32, A=1, H=1):
    """`geometry` of a case, asserted against the table."""
    g = geometry(c.up, c.nh, dtype, A, H)
    assert (g["Lp"], g["bucket"], g["tp_bucket"], g["i_lo"], g["rem"]) == (c.Lp, c.bucket, c.bucket, c.i_lo, c.rem), (c, g)
    assert g["latency"] == A - 1 + c.i_lo + (c.rem >= 2), (c, g)
    return g


@functools.lru_cache(maxsize=None)
def _uniform_taps(up, nh, seed=0):
    return np.random.default_rng(90000 + 1000 * up + nh + 100000 * seed).uniform(-1.0, 1.0, nh)


def taps(c, dtype, scaled=True):
    """uniform(-1, 1) from the case's seed in the signal's dtype, times the case's scale (`scaled`; the true-peak tests take
    them as they are): a host tensor, as the library holds an interpolator (already scaled by up)."""
    h = _uniform_taps(c.up, c.nh, c.seed).astype(NP[dtype])
    if scaled:
        h = h * NP[dtype](c.scale)
    return torch.from_numpy(np.ascontiguousarray(h))


def phase_table(h, up, LP):
    """hp[ph][j] = h_padded[ph + j * up], h_padded = [0, h..., 0 ...] (SciPy's n_pre_pad = 1 for down = 1): [up, LP] float64."""
    hp = np.zeros(up * LP)
    hp[1:1 + len(h)] = np.asarray(h, dtype=np.float64)
    return hp.reshape(LP, up).T.copy()


# ---- the limiter's signal and what the float64 definition says about it ---------------------------------------------------
LIMITER_T = 2 * 8190 + 3                       # 2 * tile + 3 at A = H = 1 (the tests assert the tile)


def limiter_shape(k):
    from tests.test_gpu_limiter import SHAPES
    return SHAPES[k % len(SHAPES)]


def over_signal(shape, seed, dtype):
    """|x| uniform in [1, 2] with random signs: p >= |x| > c at every position, so the gain shows p everywhere."""
    g = np.random.default_rng(seed)
    x = g.uniform(1.0, 2.0, shape) * g.choice([-1.0, 1.0], shape)
    x = x.astype(NP[dtype])
    assert float(np.abs(x).min()) >= 1.0 and float(np.abs(x).max()) <= 2.0
    return x


def limiter_signal(k, dtype):
    """Case k's signal [*lead, T] and whether its channels are linked (the rotation of tests/test_gpu_limiter.SHAPES)."""
    lead, link = limiter_shape(k)
    return over_signal(lead + (LIMITER_T,), 7000 + k, dtype), link


def grouped(x, link):
    """[groups, channels, T] of a signal [*lead, T]."""
    channels = x.shape[-2] if (link and x.ndim >= 2) else 1
    return x.reshape(-1, channels, x.shape[-1])


def candidates(xg, h, up):
    """For one group xg [C, T] (float64 statement): cand[ch, i, :] = (|x[i]|, the up outputs |v[i*up + ph]| of position i, the
    up outputs of position i - 1 (0 at i = 0)) -- the 2 up + 1 values p[i] is the maximum of, per channel."""
    xg = np.atleast_2d(np.asarray(xg, dtype=np.float64))
    C, T = xg.shape
    q = np.abs(RR.ref(xg, np.asarray(h, dtype=np.float64), up, 1)).reshape(C, T, up)
    qs = np.concatenate([np.zeros((C, 1, up)), q[:, :-1]], 1)
    return np.concatenate([np.abs(xg)[:, :, None], q, qs], -1)


def owner(cand):
    """Which of the 2 up + 1 candidates owns p[i] (over the channels): [T] ints; 0 is the sample itself."""
    return cand.max(0).argmax(-1)


def share_and_coverage(cand, up):
    """(share of positions whose maximum is an interpolator output, the (residue i mod 16, candidate) pairs that never own one)."""
    own = owner(cand)
    missing = [(res, k) for res in range(TP_R) for k in range(2 * up + 1) if not (own[res::TP_R] == k).any()]
    return float((own != 0).mean()), missing


def beta(xg, h, up, Lp):
    """beta[i] for one group xg [C, T] in the signal's dtype: the largest resample_reference.bound over the outputs of
    positions i - 1 and i, over the channels.  |p - p_ref| <= beta: |x| is exact and p is a maximum of such outputs."""
    xg = np.atleast_2d(xg)
    C, T = xg.shape
    b = np.stack([RR.bound(xg[ch], np.asarray(h), up, 1, Lp) for ch in range(C)]).reshape(C, T, up).max(-1).max(0)
    return np.maximum(b, np.concatenate([[0.0], b[:-1]]))


def gain_tolerance(c_lin, p_ref, b, extra):
    """|g - g_ref| <= c beta / (p_ref (p_ref - beta)) + extra: r = fl(c / p) with |p - p_ref| <= beta, and `extra` for the
    roundings of the division and of 1 - fl(1 - r) (2u on the device; (2A + 4)u on the CPU path)."""
    assert (p_ref > 2 * b).all()
    return c_lin * b / (p_ref * (p_ref - b)) + extra


# ---- true-peak rows: every (slot, phase) cell of the chain owns some row's maximum ----------------------------------------
TP_SHORT = 600                                 # the cell sweep, the first and the last thread
TP_NOISE = 0.01


def _matched_rows(c, T, targets, seed):
    """Two rows per target (P, ph): noise at 0.01 plus a burst of amplitude 1 on the Lp inputs x[i_lo + P - j] that output
    (P, ph) = sum_j hp[ph][j] x[i_lo + P - j] reads -- in the first row the least-squares burst whose outputs, over every
    position and phase it reaches, come closest to 1 at (P, ph) and 0 elsewhere, in the second the phase's own taps reversed in
    time (the burst a filter answers loudest, by Cauchy-Schwarz).  Where the maximum really falls is read from the reference
    (`truepeak_reference`), not taken from here."""
    hp = phase_table(_uniform_taps(c.up, c.nh, c.seed), c.up, c.Lp)
    L = c.Lp
    x = np.random.default_rng(seed).uniform(-TP_NOISE, TP_NOISE, (2 * len(targets), T))
    bursts = {}
    for k, (P, ph) in enumerate(targets):
        if ph not in bursts:
            # output (P + d, ph') = sum_j' hp[ph'][d + j'] b[j'],  b[j'] = x[i_lo + P - j'],  |d| < Lp
            M = np.zeros((2 * L - 1, c.up, L))
            for d in range(-(L - 1), L):
                for jj in range(L):
                    if 0 <= d + jj < L:
                        M[d + L - 1, :, jj] = hp[:, d + jj]
            e = np.zeros((2 * L - 1, c.up))
            e[L - 1, ph] = 1.0
            b = np.linalg.lstsq(M.reshape(-1, L), e.reshape(-1), rcond=None)[0]
            top = np.abs(hp[ph]).max()                         # 0: a phase of SciPy's padding alone, nothing to aim at
            bursts[ph] = (b / np.abs(b).max(), hp[ph] / top) if top > 0 else (np.zeros(L), np.zeros(L))
        for j in range(L):
            i = c.i_lo + P - j
            if 0 <= i < T:
                x[2 * k, i] += bursts[ph][0][j]
                x[2 * k + 1, i] += bursts[ph][1][j]
    return x


def last_position(c, T):
    """The last position (from i_lo) with an output: with rem > 0 only its phases below rem are outputs."""
    return (T * c.up - 1 + c.rem) // c.up


@functools.lru_cache(maxsize=None)
def truepeak_rows(k, dtype, tile_in=4096):
    """The two row sets of case k in the signal's dtype, never modified: "short" [rows, 600] -- every cell (slot, ph) behind
    positions 64 .. 79, then the first thread's 16 positions and the last 16 positions -- and "long" [rows, tile_in + 100]:
    every phase at positions 1023 | 1024 (lane 63 of wave 0 | lane 0 of wave 1) and tile_in - 1 | tile_in (the first seam)."""
    c = CASES[k]
    cells = [(64 + s, ph) for s in range(TP_R) for ph in range(c.up)]
    first = [(s, (s + 1) % c.up) for s in range(TP_R)]
    PL = last_position(c, TP_SHORT)
    last = [(PL - s, (c.rem - 1 - s) % c.up) for s in range(TP_R)]
    short = _matched_rows(c, TP_SHORT, cells + first + last, 31000 + k)
    marks = [(P, ph) for P in (1023, 1024, tile_in - 1, tile_in) for ph in range(c.up)]
    long = _matched_rows(c, tile_in + 100, marks, 32000 + k)
    out = {"short": short.astype(NP[dtype]), "long": long.astype(NP[dtype])}
    for v in out.values():
        v.setflags(write=False)
    return out


def truepeak_reference(c, x, h, wide):
    """(peak_ref [rows] float64, the argmax's position P counted from i_lo [rows], its table phase [rows], the tolerance
    max_n bound[n] [rows]) of rows x in the signal's dtype with taps h, from resample_reference.ref (`wide` for float64 signals)."""
    v = np.abs(RR.ref(x, np.asarray(h), c.up, 1, wide=wide))
    m = v.argmax(-1)
    peak = v[np.arange(len(x)), m].astype(np.float64)
    tol = np.array([RR.bound(row, np.asarray(h), c.up, 1, c.Lp).max() for row in x])
    return peak, (m + c.rem) // c.up, (m + c.rem) % c.up, tol


def cell_coverage(c, P, ph, T, tile_in=4096):
    """What a set of rows' argmax positions cover: the (slot, phase) cells, and whether the first thread, the thread that owns
    the last position, lane 63 of wave 0, lane 0 of wave 1 and either side of the first tile seam own one."""
    thread = P // TP_R
    return dict(cells={(int(a % TP_R), int(b)) for a, b in zip(P, ph)}, first=bool((thread == 0).any()),
                last=bool((thread == last_position(c, T) // TP_R).any()), lane63=bool((thread == 63).any()),
                lane64=bool((thread == 64).any()), seam_lo=bool((P == tile_in - 1).any()), seam_hi=bool((P == tile_in).any()))


def assert_truepeak_coverage(c, cov):
    """The coverage the true-peak test needs of `cell_coverage` of the "short" and the "long" rows."""
    short, long = cov["short"], cov["long"]
    assert not ALL_CELLS[c.up] - short["cells"], sorted(ALL_CELLS[c.up] - short["cells"])
    assert short["first"] and short["last"], short          # with rem > 0 the first thread takes the loop with the bounds test
    assert long["lane63"] and long["lane64"] and long["seam_lo"] and long["seam_hi"], long


ALL_CELLS = {up: {(s, ph) for s in range(TP_R) for ph in range(up)} for up in (2, 4, 8)}


# ---- the limiter at A = H = 1 against the float64 definition, position by position ----------------------------------------
def limiter_kwargs(c, dtype, A=1, H=1):
    """limit()'s arguments for a case: A = max(1, round(lookahead * fs)) and H likewise, the case's scaled taps."""
    return dict(lookahead=(A if A > 1 else 0.0) / FS, hold=H / FS, detector="true_peak", oversample=c.up, taps=taps(c, dtype))


@functools.lru_cache(maxsize=None)
def limiter_statement(k, dtype):
    """Case k at A = H = 1 (window [1]): the signal, its grouping, the call's parameters and per group the float64 reference
    (tests/limiter_reference.limit_reference on float64(x) with the rounded c, w and h): y_ref, g_ref, p_ref and beta."""
    from tests import limiter_reference as R
    from tests.test_limiter_host import params, reference
    c = CASES[k]
    x, link = limiter_signal(k, dtype)
    x.setflags(write=False)
    P = params(dtype, **limiter_kwargs(c, dtype))
    assert (P.A, P.H, P.up, P.taps.numel()) == (1, 1, c.up, c.nh) and P.w.tolist() == [1.0]
    h = P.taps.numpy()
    groups = []
    for xg in grouped(x, link):
        y_ref, g_ref, _ = reference(xg, P)
        p_ref = R.detector(xg, c.up, h.astype(np.float64))
        groups.append(dict(x=xg, y_ref=y_ref, g_ref=g_ref, p_ref=p_ref, beta=beta(xg, h, c.up, c.Lp)))
    return dict(x=x, link=link, P=P, groups=groups)


def limiter_errors(st, g, y, dtype, extra):
    """Largest err / tol of a gain curve g [groups, T] and a result y (the signal's shape) against `limiter_statement`'s
    reference: |g - g_ref| <= c beta / (p_ref (p_ref - beta)) + extra and |y - y_ref| <= that |x| + u |y_ref|."""
    u = U[dtype]
    y = np.asarray(y).reshape(len(st["groups"]), -1, st["x"].shape[-1])
    worst_g = worst_y = 0.0
    for G, gg, yy in zip(st["groups"], np.asarray(g), y):
        tol = gain_tolerance(st["P"].c, G["p_ref"], G["beta"], extra)
        worst_g = max(worst_g, float((np.abs(gg.astype(np.float64) - G["g_ref"]) / tol).max()))
        tol_y = tol * np.abs(G["x"].astype(np.float64)) + u * np.abs(G["y_ref"])
        worst_y = max(worst_y, float((np.abs(yy.astype(np.float64) - G["y_ref"]) / tol_y).max()))
    return worst_g, worst_y
