"""True peak (BS.1770-4 Annex 2, 4x oversampled) on one MI355X: 64 rows x 2 880 000 float32 samples (60 s at 48 kHz) and
2 rows x 28 800 000 (a ten-minute stereo file).

It times, in the same run and alternating,
  (a) ``true_peak_linear`` -- the measuring kernel and its fold: reads 4 B per sample, writes one value per 4096 samples;
  (b) the composition a caller had to write: ``resample_poly(x, 4, 1).abs().amax(-1)`` -- the resampler writes 16 B per
      sample, ``abs`` reads and writes them, ``amax`` reads them again;
  (c) the per-row absolute maximum ``stat_forward`` -- the read-once floor of any per-row reading,
and checks (a) against (b) bit for bit.  Times are device events around one call; min / median / max of --repeats are all
recorded, max - min being the run-to-run spread of this run.  The gate: every repeat of (a) is faster than every repeat of
(b) at both shapes.  The ratio (a) / (c) is recorded only.

    python tools/truepeak_bench.py --out profiles/truepeak_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 48000
UP = 4
SHAPES = [(64, 2_880_000), (2, 28_800_000)]
WARM = 3


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
    return [(min(t), statistics.median(t), max(t)) for t in ts]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("truepeak_bench needs a ROCm device")
    from torchfx_amd import resample_poly, true_peak_linear, torchfx_ext as E

    lines = [f"true peak at {FS} Hz, {UP}x oversampled ({20 * UP + 1} taps), float32 signals on {torch.cuda.get_device_name(0)}; device "
             f"events around one call, min / median / max of {args.repeats} alternating repeats, ms"]
    ok = True
    for rows, length in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(rows, length, generator=g, device="cuda", dtype=torch.float32) * 2 - 1
        info = E.true_peak_plan_info(rows, length, UP, 20 * UP + 1)
        same = bool(torch.equal(true_peak_linear(x, FS), resample_poly(x, UP, 1).abs().amax(-1)))
        a, b, c = time_alternating([lambda: true_peak_linear(x, FS), lambda: resample_poly(x, UP, 1).abs().amax(-1),
                                    lambda: E.stat_forward(x, E.STAT_ABSMAX, per_row=True)], args.repeats)
        n = rows * length
        fma = n * UP * info["Lp"]                                       # useful fmas: Lp per output, zero taps of the bucket not counted
        row = dict(rows=rows, length=length, Lp=info["Lp"], tile_in=info["tile_in"], tiles=info["tiles"], true_peak_ms=a,
                   composition_ms=b, absmax_ms=c, composition_over_true_peak=b[0] / a[0], true_peak_over_absmax=a[0] / c[0],
                   true_peak_GBs_at_4B=4.0 * n / a[0] * 1e-6, true_peak_Gfma_per_s=fma / a[0] * 1e-6, bit_equal=same)
        lines.append(json.dumps(row))
        fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"      # noqa: E731
        lines.append(f"{rows} x {length}, {info['tiles']} tiles per row: (a) true_peak_linear {fmt(a)}   (b) resample_poly + abs + amax "
                     f"{fmt(b)}   (c) per-row absmax {fmt(c)}   b/a {b[0] / a[0]:.2f}x   a/c {a[0] / c[0]:.2f}x   spread of (a) "
                     f"{a[2] - a[0]:.3f}, of (b) {b[2] - b[0]:.3f}, of (c) {c[2] - c[0]:.3f}   (a) reads 4 B/sample at "
                     f"{4.0 * n / a[0] * 1e-9:.2f} TB/s and runs {fma / a[0] * 1e-9:.1f} T fma/s   (a) == (b) bit for bit: {same}")
        ok = ok and same and a[2] < b[0]
        del x
        torch.cuda.empty_cache()
    lines.append("gate: " + ("PASS" if ok else "FAIL") + " (true_peak_linear equal to the composition bit for bit, and its slowest repeat "
                 "faster than the composition's fastest, both shapes)")
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
