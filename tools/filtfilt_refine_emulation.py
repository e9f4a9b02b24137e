"""Float64 emulation of the cascade kernel's blocked arithmetic (LC = 16 / 32 / 64 samples per lane, 64 lanes per tile) with and
without the refinement step (csrc/sos.hip, FFR: the zero-phase passes of a float64 result, and the forward cascade and the
measuring pass for the cascades the library's rule picks), against a long-double sequential recursion.  Host
only; prints, per filter, rate and LC, the largest error of the blocked form, of the refined form and of a sequential float64
recursion.  The lane scan is summed lane by lane here (the kernel's tree order differs; the magnitudes do not); the library's
own decision replays the kernel's tree in C++ (tfx_sos_refine_info) and lands on the same figures.

    python tools/filtfilt_refine_emulation.py                       # the 48 kHz table of DESIGN.md 4.8, LC = 32
    python tools/filtfilt_refine_emulation.py --fs 96000 192000 --lc 16 64
"""
from __future__ import annotations

import numpy as np
import scipy.signal as ss

import argparse

LC, NL = 32, 64
TILE = LC * NL


def lane_scan(pm, z):
    """S_j = sum_{i <= j} P^(j - i) z_i."""
    out = np.zeros_like(z)
    for j in range(NL):
        acc = np.zeros(2)
        for i in range(j + 1):
            acc = acc + pm[j - i] @ z[i]
        out[j] = acc
    return out


def section_blocked(b, a, x, refine):
    b0, b1, b2 = b
    na1, na2 = -a[1], -a[2]
    cm = np.array([[na1, na2], [1.0, 0.0]], dtype=np.longdouble)
    base = np.eye(2, dtype=np.longdouble)
    for _ in range(LC):
        base = cm @ base
    pm = [np.eye(2, dtype=np.longdouble)]
    for _ in range(NL):
        pm.append(base @ pm[-1])
    pm = [p.astype(np.float64) for p in pm]                 # the host tables: long double, rounded once

    def recur(s1, s2, f, keep=None):
        for n in range(LC):
            v = na1 * s1 + (na2 * s2 + f[:, n])
            s2, s1 = s1, v
            if keep is not None:
                keep[:, n] = v
        return s1, s2

    y = np.empty_like(x)
    cv, cy = (0.0, 0.0), np.zeros(2)
    for ts in range(0, x.size, TILE):
        d = x[ts:ts + TILE].reshape(NL, LC)
        pv1 = np.concatenate([[cv[0]], d[:-1, -1]])
        pv2 = np.concatenate([[cv[1]], d[:-1, -2]])
        cv = (d[-1, -1], d[-1, -2])
        f = np.empty_like(d)
        for n in range(LC):
            x1 = d[:, n - 1] if n >= 1 else pv1
            x2 = d[:, n - 2] if n >= 2 else (pv1 if n == 1 else pv2)
            f[:, n] = b2 * x2 + (b1 * x1 + b0 * d[:, n])
        u1, u2 = np.zeros(NL), np.zeros(NL)
        u1[0], u2[0] = cy
        u1, u2 = recur(u1, u2, f)
        h = np.vstack([cy, lane_scan(pm, np.stack([u1, u2], 1))[:-1]])
        if refine:                                          # where chunk j - 1 ends minus where chunk j was told to start
            w1, w2 = recur(h[:, 0].copy(), h[:, 1].copy(), f)
            r = np.zeros((NL, 2))
            r[1:, 0], r[1:, 1] = w1[:-1] - h[1:, 0], w2[:-1] - h[1:, 1]
            h = h + lane_scan(pm, r)
        out = np.empty_like(d)
        recur(h[:, 0].copy(), h[:, 1].copy(), f, out)
        cy = np.array([out[-1, -1], out[-1, -2]])
        y[ts:ts + TILE] = out.reshape(-1)
    return y


def section_long_double(b, a, x):
    x = x.astype(np.longdouble)
    y = np.zeros_like(x)
    b = [np.longdouble(v) for v in b]
    a = [np.longdouble(v) for v in a]
    x1 = x2 = y1 = y2 = np.longdouble(0)
    for n in range(x.size):
        v = b[0] * x[n] + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2
        x2, x1, y2, y1 = x1, x[n], y1, v
        y[n] = v
    return y


def run(fs: int, lc: int) -> None:
    global LC, TILE
    LC, TILE = lc, lc * NL
    x = np.random.default_rng(0).uniform(-1, 1, max(TILE * 16, 65536))
    filters = {f"HiButterworth(20, order=5) @ {fs} Hz, LC {lc}": ss.butter(5, 20, "highpass", fs=fs, output="sos"),
               f"HiButterworth(20, order=4) @ {fs} Hz, LC {lc}": ss.butter(4, 20, "highpass", fs=fs, output="sos"),
               f"Notch(60, q=30) @ {fs} Hz, LC {lc}": ss.tf2sos(*ss.iirnotch(60, 30, fs=fs)),
               f"LoButterworth(40, order=8) @ {fs} Hz, LC {lc}": ss.butter(8, 40, fs=fs, output="sos"),
               f"LoButterworth(2000, order=4) @ {fs} Hz, LC {lc}": ss.butter(4, 2000, fs=fs, output="sos")}
    for name, sos in filters.items():
        blocked, refined, seq, ref = x.copy(), x.copy(), x.copy(), x.astype(np.longdouble)
        for s in sos:
            ref = section_long_double(s[:3], s[3:], ref)
            blocked = section_blocked(s[:3], s[3:], blocked, False)
            refined = section_blocked(s[:3], s[3:], refined, True)
            seq = ss.lfilter(s[:3], s[3:], seq)
        scale = max(1.0, float(np.abs(ref).max()))
        print(f"{name}: blocked {float(np.abs(blocked - ref).max()) / scale:.2e}   refined {float(np.abs(refined - ref).max()) / scale:.2e}   "
              f"sequential float64 {float(np.abs(seq - ref).max()) / scale:.2e}   (of max(1, max|y|) = {scale:.2f})")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, nargs="+", default=[48000])
    ap.add_argument("--lc", type=int, nargs="+", default=[32], choices=[16, 32, 64])
    args = ap.parse_args()
    for fs in args.fs:
        for lc in args.lc:
            run(fs, lc)


if __name__ == "__main__":
    main()
