"""Zero-phase filtering on one MI355X at cfg-2 size: 64 rows x 2 880 000 float32 samples (60 s at 48 kHz).

For cfg 2's cascade (LoButterworth-6 | ParametricEQ, 4 sections) and one long-memory filter of the iir_hard set
(HiButterworth(20, order=5)) it times, in the same run and alternating,
  (a) ``sosfiltfilt`` -- two cascade launches around one float64 intermediate, 24 B per sample;
  (b) the float64 composition a caller had to write from the library's existing ops: ``x.double()``, odd-extension ``cat``,
      ``sos_forward`` from hand-computed steady-state start states, ``flip``, ``sos_forward``, ``flip``, slice, ``.float()``;
  (c) one plain forward ``sos_forward`` float32 -> float32,
  (d) ``sosfiltfilt`` of the same signal in float64 (32 B per sample; its passes refine the scan's start states),
and checks (a) against (b) within the float32 IIR tolerance (1.5e-7 of max(1, max|y|)).  Times are device events around one
call, min / median of --repeats.  The gate: (a) at least 2x faster than (b); the ratio to (c) is recorded only.

    python tools/filtfilt_bench.py --out profiles/filtfilt_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 48000
ROWS, T = 64, 2_880_000
WARM = 3
TOL = 1.5e-7


def cascades():
    from torchfx_amd import filter as F

    f1 = F.LoButterworth(2000, order=6, fs=FS)
    f2 = F.ParametricEQ(frequency=1000, q=2.0, gain=3.0, fs=FS)
    hard = F.HiButterworth(20, order=5, fs=FS)
    for f in (f1, f2, hard):
        f.compute_coefficients()
    return {"cfg2 (LoButterworth-6 | ParametricEQ, 4 sections)": torch.cat([f1._sos, f2._sos]).contiguous().double(),
            "iir_hard HiButterworth(20, order=5), 3 sections": hard._sos.contiguous().double()}


def composition(x, sos, pad, gains):
    """sosfiltfilt(padtype="odd") from sos_forward and torch ops, in float64 on the device."""
    from torchfx_amd import torchfx_ext as E

    def start(v):                 # DF1 steady state for the constant v [C]: [K, C, 2] past inputs and past outputs
        gx = gains[:-1].to(v.device)[:, None, None] * v[None, :, None]
        gy = gains[1:].to(v.device)[:, None, None] * v[None, :, None]
        return gx.expand(-1, -1, 2).contiguous(), gy.expand(-1, -1, 2).contiguous()

    xd = x.double()
    ext = torch.cat([2 * xd[:, :1] - xd[:, 1:pad + 1].flip(-1), xd, 2 * xd[:, -1:] - xd[:, -pad - 1:-1].flip(-1)], dim=-1)
    sx, sy = start(ext[:, 0])
    y = E.sos_forward(ext, None, sos, sx, sy)[0]
    y = y.flip(-1)
    sx, sy = start(y[:, 0])
    y = E.sos_forward(y, None, sos, sx, sy)[0]
    return y.flip(-1)[:, pad:pad + x.shape[-1]].float()


def time_alternating(fns, repeats):
    for fn in fns:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(min(t), statistics.median(t)) for t in ts]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--length", type=int, default=T)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filtfilt_bench needs a ROCm device")
    from torchfx_amd import sosfiltfilt, torchfx_ext as E
    from torchfx_amd.filtfilt import default_padlen, steady_state_gains

    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(args.rows, args.length, generator=g, device="cuda", dtype=torch.float32) * 2 - 1
    lines = [f"{args.rows} rows x {args.length} float32 samples on {torch.cuda.get_device_name(0)}; device events around one call, "
             f"min / median of {args.repeats} alternating repeats, ms"]
    ok = True
    for name, sos in cascades().items():
        a = sos.numpy()
        pad = default_padlen(a)
        gains = torch.from_numpy(steady_state_gains(a))
        info = E.sos_filtfilt_plan_info(a, args.rows, args.length)
        ya = sosfiltfilt(x, sos)
        yb = composition(x, sos, pad, gains)
        scale = max(1.0, float(yb.abs().max()))
        diff = float((ya.double() - yb.double()).abs().max())
        del ya, yb
        xd = x.double()
        (a_min, a_med), (b_min, b_med), (c_min, c_med), (d_min, d_med) = time_alternating(
            [lambda: sosfiltfilt(x, sos), lambda: composition(x, sos, pad, gains), lambda: E.sos_forward(x, None, sos, None, None)[0],
             lambda: sosfiltfilt(xd, sos)], args.repeats)
        del xd
        n = args.rows * args.length
        row = dict(cascade=name, padlen=pad, nseg_forward=info["nseg_forward"], nseg_reverse=info["nseg_reverse"],
                   filtfilt_ms=(a_min, a_med), composition_ms=(b_min, b_med), forward_ms=(c_min, c_med),
                   filtfilt_f64_ms=(d_min, d_med),
                   composition_over_filtfilt=b_min / a_min, filtfilt_over_forward=a_min / c_min,
                   filtfilt_GBs_at_24B=24.0 * n / a_min * 1e-6, max_diff=diff, tol=TOL * scale)
        lines.append(json.dumps(row))
        lines.append(f"{name}: (a) sosfiltfilt {a_min:.3f} / {a_med:.3f}   (b) float64 composition {b_min:.3f} / {b_med:.3f}   "
                     f"(c) one forward pass {c_min:.3f} / {c_med:.3f}   b/a {b_min / a_min:.2f}x (gate >= 2)   a/c {a_min / c_min:.2f}x   "
                     f"(d) sosfiltfilt of the float64 signal, refined start states, 32 B/sample {d_min:.3f} / {d_med:.3f}   "
                     f"(a) moves 24 B/sample at {24.0 * n / a_min * 1e-9:.2f} TB/s   max |a - b| {diff:.2e} (bar {TOL * scale:.2e})")
        ok = ok and diff <= TOL * scale and b_min / a_min >= 2.0
        torch.cuda.empty_cache()
    lines.append("gate: " + ("PASS" if ok else "FAIL") + " (sosfiltfilt within the bar of the composition and at least 2x faster, every cascade)")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
