"""Phaser (defaults but for `stages`: rate 0.5 Hz, 200-2000 Hz, mix 0.5, sine) on one MI355X at float32 and 48 kHz:
[32, 2, 2 880 000] (64 rows: 32 minutes of stereo in one-minute items) and [1, 2, 28 800 000] (2 rows: a ten-minute stereo file).

It times, in the same run and alternating,
  (a) ``Phaser(stages=4)`` and (b) ``Phaser(stages=12)`` -- two launches with the plan's segments (512 workgroups in the second);
  (c) ``Freeverb()`` on the same rows -- the other scan-built effect, one workgroup per row;
  (d) ``gain_forward`` over the same samples -- the read-once / write-once floor of anything that scales a signal,
and, once, (e) the NumPy host path on a CPU copy of one row.  Times are device events around one call; min / median / max of
--repeats are all recorded.  No time is gated: nobody had measured this kernel before.  The figures to read are (a) / (d), the
cost of a stage ((b) - (a)) / 8 and what is left of (a) without its stages, a[n] and the products of the scan.

    python tools/phaser_bench.py --out profiles/phaser_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 48000
SHAPES = [(32, 2, 2_880_000), (1, 2, 28_800_000)]
WARM = 1


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


def signal(B, C, T):
    g = torch.Generator(device="cuda").manual_seed(1)
    return torch.randn(B, C, T, generator=g, device="cuda", dtype=torch.float32) * 0.25


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("phaser_bench needs a ROCm device")
    from torchfx_amd import Freeverb, Phaser, torchfx_ext as E

    lines = [f"Phaser at {FS} Hz, rate 0.5 Hz, 200-2000 Hz, sine, float32 on {torch.cuda.get_device_name(0)}; device events around one "
             f"call, min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    p4, p12, room = Phaser(stages=4, fs=FS), Phaser(stages=12, fs=FS), Freeverb(fs=FS)
    for B, C, T in SHAPES:
        x = signal(B, C, T)
        info = E.phaser_plan_info(T, B * C, C, 4)
        a, b, c, d = time_alternating([lambda: p4(x), lambda: p12(x), lambda: room(x), lambda: E.gain_forward(x, 0.5)], args.repeats)
        n = B * C * T
        stage = (b[0] - a[0]) / 8.0
        row = dict(batch=B, channels=C, length=T, tile=info["tile"], tiles=info["tiles"], segments=info["segments"],
                   seg_tiles=info["seg_tiles"], phaser4_ms=a, phaser12_ms=b, freeverb_ms=c, gain_ms=d, phaser4_over_gain=a[0] / d[0],
                   phaser12_over_gain=b[0] / d[0], phaser4_over_freeverb=a[0] / c[0], ms_per_stage=stage, ms_without_stages=a[0] - 4.0 * stage,
                   phaser4_samples_per_us=n / a[0] * 1e-3, gain_TBs=8.0 * n / d[0] * 1e-9)
        lines.append(json.dumps(row))
        lines.append(f"{B} x {C} x {T} ({B * C} rows, {info['tiles']} tiles of {info['tile']} per row in {info['segments']} segments of up to "
                     f"{info['seg_tiles']}): (a) Phaser(stages=4) {fmt(a)}   (b) Phaser(stages=12) {fmt(b)}   (c) Freeverb() {fmt(c)}   "
                     f"(d) gain_forward {fmt(d)}   a/d {a[0] / d[0]:.1f}x   b/d {b[0] / d[0]:.1f}x   a/c {a[0] / c[0]:.2f}x   a stage costs "
                     f"{stage:.3f} ms, the rest of (a) {a[0] - 4.0 * stage:.3f} ms; (a) runs {n / a[0] * 1e-3:.0f} samples/us; (d) moves "
                     f"8 B/sample at {8.0 * n / d[0] * 1e-9:.2f} TB/s")
        del x
        torch.cuda.empty_cache()
    T = SHAPES[0][2]
    xh = signal(1, 1, T).reshape(T).cpu()
    t0 = time.perf_counter()
    p4(xh)
    lines.append(f"(e) host path (NumPy, a blocked scan per stage, one call, wall clock) on one row of {T}, stages=4: "
                 f"{(time.perf_counter() - t0) * 1e3:.0f} ms")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
