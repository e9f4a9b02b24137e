"""Freeverb's definition (include/torchfx_hip.h, tfx_freeverb_forward) as plain per-sample loops straight from the difference
equations, independent of the product's block-wise host path, in any NumPy float type; the cases the reverb tests share; and
the error bound they hold the product to.

    u[n]   = input_gain (2 / C) sum_c x_c[n]
    comb k:      o[n] = w[n - D];  f[n] = d2 o[n] + d1 f[n-1];  w[n] = u[n] + fb f[n];  d2 = 1 - d1
    s_0[n] = ((o_0[n] + o_1[n]) + o_2[n]) + ...
    all-pass j:  b[n] = v[n - D];  s_{j+1}[n] = b[n] - s_j[n];  v[n] = s_j[n] + g b[n]
    y_c[n] = dry x_c[n] + wet1 r_c[n] + wet2 r_{1-c}[n],  r = s_NA          (one channel: dry x[n] + (wet1 + wet2) r_0[n])

The bound is measured, not invented.  E_REF is the largest max|ref_float64 - ref_longdouble| / max(1, max|ref|) over every case
below (outputs and states), measured on an x86 host whose np.longdouble is the 80-bit format, with

    python -m tests.reverb_reference

which printed `E_REF = 3.7e-16 (worst case: bank eight-four-d0.4-fb0.98-T4097-C2)`: 3.6989e-16, the constant below rounded up to two digits.
tests/test_reverb_host.py measures it again wherever np.longdouble is wider than float64.  With scale = max(1, max|ref|):

    float64 outputs and states:  |got - ref_float64| <= 16 E_REF scale
    float32 outputs, per sample: |got - ref_float64| <= 2^-23 |ref_float64| + 16 E_REF scale

16 covers the parallel scan (a NumPy emulation of the 64-lane scan stayed within 3.5 times the serial float64 error) and fma
contraction on the device; a real defect -- a lost carry, a delay off by one -- shows at 1e-3 or more.  Signals hold
float32-representable values in [-1, 1], so one reference serves both dtypes."""
import functools
import sys

import numpy as np

E_REF = 3.7e-16
TOL = 16.0 * E_REF

COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_TUNING = (556, 441, 341, 225)


def tunings(fs, channels):
    """Freeverb's delays at fs: max(1, floor(t fs / 44100 + 0.5)) with t including the second channel's 23 samples."""
    def at(t):
        return max(1, int(np.floor(t * fs / 44100.0 + 0.5)))
    return ([[at(t + 23 * c) for t in COMB_TUNING] for c in range(channels)],
            [[at(t + 23 * c) for t in ALLPASS_TUNING] for c in range(channels)])


def freeverb_constants(room_size=0.5, damping=0.5, wet=1.0 / 3.0, dry=0.5, width=1.0):
    """(fb, d1, g, input_gain, dry_gain, wet1, wet2) of Freeverb's user parameters."""
    return (0.7 + 0.28 * room_size, 0.4 * damping, 0.5, 0.015, 2.0 * dry, 3.0 * wet * (width / 2.0 + 0.5),
            3.0 * wet * ((1.0 - width) / 2.0))


def state_len(comb, allpass):
    return max(sum(cd) + len(cd) + sum(ad) for cd, ad in zip(comb, allpass))


def _bank(u, comb, allpass, fb, d1, g, st, dt):
    """One bank over the feed u (a list of dt scalars): the wet signal r (a list) and the end state (a list, time order)."""
    d2 = dt(1) - d1
    lines, fs_, pos, off = [], [], [], 0
    for D in comb:
        lines.append(list(st[off:off + D]))
        fs_.append(st[off + D])
        pos.append(0)
        off += D + 1
    aps, apos = [], []
    for D in allpass:
        aps.append(list(st[off:off + D]))
        apos.append(0)
        off += D
    r = []
    nc = len(comb)
    for un in u:
        s = None
        for k in range(nc):
            ln, p = lines[k], pos[k]
            o = ln[p]
            f = d2 * o + d1 * fs_[k]
            fs_[k] = f
            ln[p] = un + fb * f
            p += 1
            pos[k] = 0 if p == comb[k] else p
            s = o if s is None else s + o
        for j, D in enumerate(allpass):
            ln, p = aps[j], apos[j]
            b = ln[p]
            ln[p] = s + g * b
            s = b - s
            p += 1
            apos[j] = 0 if p == D else p
        r.append(s)
    out = []
    for k in range(nc):
        out += lines[k][pos[k]:] + lines[k][:pos[k]] + [fs_[k]]
    for j in range(len(allpass)):
        out += aps[j][apos[j]:] + aps[j][:apos[j]]
    return r, out


def freeverb_ref(x, comb, allpass, fb, d1, g=0.5, input_gain=0.015, dry=1.0, wet1=1.0, wet2=0.0, tail=0, state=None,
                 dtype=np.float64):
    """x [T], [C, T] or [B, C, T] (C 1 or 2; any float array); comb / allpass [C][NC] / [C][NA] -> (y [..., T + tail] unrounded
    in `dtype`, state [B * C, state_len] in `dtype`).  `state` likewise, or None (silence)."""
    x = np.asarray(x)
    T = x.shape[-1]
    C = x.shape[-2] if x.ndim >= 2 else 1
    xr = x.reshape(-1, C, T)
    B, Tn = xr.shape[0], T + tail
    S = state_len(comb, allpass)
    dt = float if np.dtype(dtype) == np.float64 else np.dtype(dtype).type
    fb, d1, g, dry, wet1, wet2 = (dt(v) for v in (fb, d1, g, dry, wet1, wet2))
    gin = dt(input_gain) * (dt(2) / dt(C))
    y = np.zeros((B, C, Tn), dtype)
    st_out = np.zeros((B * C, S), dtype)
    zero = dt(0)
    for i in range(B):
        xs = [[dt(v) for v in xr[i, c]] + [zero] * tail for c in range(C)]
        u = [gin * (xs[0][n] if C == 1 else xs[0][n] + xs[1][n]) for n in range(Tn)]
        rs = []
        for c in range(C):
            st = [zero] * S if state is None else [dt(v) for v in np.asarray(state)[i * C + c]]
            r, so = _bank(u, list(comb[c]), list(allpass[c]), fb, d1, g, st, dt)
            rs.append(r)
            st_out[i * C + c, :len(so)] = so
        for c in range(C):
            if C == 1:
                y[i, c] = [dry * xs[0][n] + (wet1 + wet2) * rs[0][n] for n in range(Tn)]
            else:
                y[i, c] = [dry * xs[c][n] + wet1 * rs[c][n] + wet2 * rs[1 - c][n] for n in range(Tn)]
    return y.reshape(*x.shape[:-1], Tn), st_out


# ---- the cases the host and the device tests share ---------------------------------------------------------------------------
def signal(shape, seed):
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)
    x.setflags(write=False)
    return x


COMBS = {"one": (1,), "two": (2, 3), "wave": (63, 64, 65), "eight": (70, 83, 97, 111, 64, 129, 1, 200), "long": (7000,)}
ALLPASS = {"none": (), "one": (1,), "four": (5, 37, 64, 90)}
BANK_INPUT_GAIN = 0.1


def _bank_grid():
    """A covering subset of comb sets x all-pass sets x damp x fb x T: every comb set at T in {1, min D - 1, min D, min D + 1,
    4097} (the never-wrapping 7000 at 1 and 6000), the other three cycling so that every value of each occurs with several
    comb sets, one and two channels (the second channel's delays 2 samples longer, and a cross-feed wet2 = 0.25) alternating."""
    damps, fbs, aps = (0.0, 0.2, 0.4, 0.9), (0.98, 0.0, 0.5, 0.84), ("four", "none", "one")
    grid, i = [], 0
    for name, cd in COMBS.items():
        m = min(cd)
        for T in ([1, 6000] if name == "long" else sorted({1, m - 1, m, m + 1, 4097} - {0})):
            grid.append((name, aps[i % 3], damps[i % 4], fbs[(i // 2) % 4], T, 1 + i % 2))
            i += 1
    grid.append(("wave", "four", 0.9, 0.98, 4097, 2))
    grid.append(("eight", "four", 0.4, 0.98, 4097, 2))
    return grid


BANK_GRID = _bank_grid()
# Freeverb() itself: (shape, fs); T = 5000 wraps the lines three to four times
FREEVERB_CASES = [((5000,), 44100), ((1, 5000), 44100), ((2, 5000), 44100), ((3, 2, 5000), 44100), ((2, 5000), 48000)]


def bank_id(case):
    name, ap, damp, fb, T, C = case
    return f"{name}-{ap}-d{damp}-fb{fb}-T{T}-C{C}"


def bank_args(case):
    """(x float32 array, comb [C][NC], allpass [C][NA], keyword arguments) of a BANK_GRID case."""
    name, ap, damp, fb, T, C = case
    comb = [[d + 2 * c for d in COMBS[name]] for c in range(C)]
    allpass = [[d + 2 * c for d in ALLPASS[ap]] for c in range(C)]
    x = signal((T,) if C == 1 else (C, T), 1000 + BANK_GRID.index(case))
    kw = dict(feedback=fb, damp=damp, allpass_gain=0.5, input_gain=BANK_INPUT_GAIN, dry_gain=0.75, wet1=0.5, wet2=0.25 if C == 2 else 0.0)
    return x, comb, allpass, kw


def _ref_kw(kw):
    return dict(fb=kw["feedback"], d1=kw["damp"], g=kw["allpass_gain"], input_gain=kw["input_gain"], dry=kw["dry_gain"],
                wet1=kw["wet1"], wet2=kw["wet2"])


@functools.lru_cache(maxsize=None)
def bank_case(case, dtype=np.float64):
    """(x, comb, allpass, kw, unrounded reference y, reference state), computed once per case and shared; read-only."""
    x, comb, allpass, kw = bank_args(case)
    y, st = freeverb_ref(x, comb, allpass, dtype=dtype, **_ref_kw(kw))
    y.setflags(write=False)
    st.setflags(write=False)
    return x, comb, allpass, kw, y, st


@functools.lru_cache(maxsize=None)
def freeverb_case(shape, fs, dtype=np.float64, width=1.0, tail=0):
    """(x, unrounded reference of Freeverb(width=width) at fs with `tail` samples of ring-out, reference state)."""
    x = signal(shape, 2000 + len(shape) * 10 + shape[0] % 7 + fs % 5)
    C = shape[-2] if len(shape) >= 2 else 1
    comb, allpass = tunings(fs, C)
    fb, d1, g, gin, dry, wet1, wet2 = freeverb_constants(width=width)
    y, st = freeverb_ref(x, comb, allpass, fb, d1, g, gin, dry, wet1, wet2, tail=tail, dtype=dtype)
    y.setflags(write=False)
    st.setflags(write=False)
    return x, y, st


def check(got, ref, what, out_dtype=np.float64):
    """The bound above; returns the largest error over the float64 tolerance (float32: the largest excess over 2^-23 |ref|,
    over the same tolerance)."""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if ref.size == 0:
        return 0.0
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got.astype(np.float64) - ref)
    if np.dtype(out_dtype) == np.float32:
        err = err - 2.0 ** -23 * np.abs(ref)
    worst = float(err.max())
    print(f"{what}: worst {worst:.3e} of {TOL * scale:.3e}")
    assert np.isfinite(err).all() and worst <= TOL * scale, f"{what}: {worst:.3e} > {TOL * scale:.3e} (scale {scale:.3g})"
    return worst / (TOL * scale)


def measure_e_ref(verbose=False):
    """max over every case of max|ref_float64 - ref_longdouble| / max(1, max|ref|), outputs and states; and the worst case."""
    worst, where = 0.0, ""
    todo = [("bank " + bank_id(c), lambda d, c=c: bank_case(c, d)[4:]) for c in BANK_GRID]
    todo += [(f"freeverb {s} {fs}", lambda d, s=s, fs=fs: freeverb_case(s, fs, d)[1:]) for s, fs in FREEVERB_CASES]
    todo.append(("freeverb (2, 5000) 44100 width 0.3", lambda d: freeverb_case((2, 5000), 44100, d, 0.3)[1:]))
    for name, fn in todo:
        for a, b in zip(fn(np.float64), fn(np.longdouble)):
            e = float(np.abs(a.astype(np.longdouble) - b).max() / max(1.0, float(np.abs(a).max()))) if a.size else 0.0
            if verbose:
                print(f"{name}: {e:.2e}")
            if e > worst:
                worst, where = e, name
    return worst, where


if __name__ == "__main__":
    if np.finfo(np.longdouble).eps >= 2e-19:
        sys.exit("np.longdouble is not wider than float64 here: nothing to measure against")
    e, where = measure_e_ref(verbose=True)
    print(f"E_REF = {e:.1e} (worst case: {where})")
