"""Freeverb (defaults: room_size 0.5, damping 0.5, wet 1/3, dry 0.5, width 1) on one MI355X at float32 and 48 kHz:
[32, 2, 2 880 000] (64 rows: 32 minutes of stereo in one-minute items) and [1, 2, 28 800 000] (2 rows: a ten-minute stereo file).

It times, in the same run and alternating,
  (a) ``Freeverb()`` -- one launch, one workgroup per row; a row is a chain of T / 1024 dependent blocks, whatever the row count;
  (b) ``Freeverb(width=0.5)`` -- the channels cross-feed: the banks write the wet signal to a float64 workspace and a second,
      elementwise launch mixes;
  (c) ``gain_forward`` over the same samples -- the read-once / write-once floor of anything that scales a signal,
and, once, (d) the NumPy / SciPy host path on a CPU copy of one row.  Times are device events around one call; min / median /
max of --repeats are all recorded.  No time is gated: nobody had measured this kernel before.  The figures to read are the time
per block of a row (a row's blocks are sequential) and (a) / (c).

    python tools/reverb_bench.py --out profiles/reverb_bench.txt
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
        raise SystemExit("reverb_bench needs a ROCm device")
    from torchfx_amd import Freeverb, torchfx_ext as E
    from torchfx_amd.reverb import tunings

    lines = [f"Freeverb at {FS} Hz, defaults, stereo, float32 on {torch.cuda.get_device_name(0)}; device events around one call, "
             f"min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    comb, allpass = tunings(FS, 2)
    wide, narrow = Freeverb(fs=FS), Freeverb(width=0.5, fs=FS)
    for B, C, T in SHAPES:
        x = signal(B, C, T)
        info = E.freeverb_plan_info(T, comb, allpass, B, C)
        info2 = E.freeverb_plan_info(T, comb, allpass, B, C, wet2=narrow.params().wet2)
        a, b, c = time_alternating([lambda: wide(x), lambda: narrow(x), lambda: E.gain_forward(x, 0.5)], args.repeats)
        n, blocks = B * C * T, -(-T // info["block"])
        row = dict(batch=B, channels=C, length=T, block=info["block"], placement=info["placement"], blocks_per_row=blocks,
                   launches=info["launches"], launches_cross_feed=info2["launches"], workspace_bytes_cross_feed=info2["workspace_bytes"],
                   freeverb_ms=a, freeverb_cross_feed_ms=b, gain_ms=c, freeverb_over_gain=a[0] / c[0], cross_feed_over_one_launch=b[0] / a[0],
                   us_per_block=a[0] * 1e3 / blocks, row_samples_per_us=T / a[0] * 1e-3, all_samples_per_us=n / a[0] * 1e-3,
                   gain_TBs=8.0 * n / c[0] * 1e-9)
        lines.append(json.dumps(row))
        lines.append(f"{B} x {C} x {T} ({B * C} rows, {blocks} blocks of {info['block']} per row, lines in {info['placement']}): "
                     f"(a) Freeverb() {fmt(a)}   (b) Freeverb(width=0.5), two launches {fmt(b)}   (c) gain_forward {fmt(c)}   "
                     f"a/c {a[0] / c[0]:.1f}x   b/a {b[0] / a[0]:.2f}x   (a) takes {a[0] * 1e3 / blocks:.2f} us per block of a row, "
                     f"{T / a[0] * 1e-3:.0f} samples/us per row, {n / a[0] * 1e-3:.0f} over all rows; (c) moves 8 B/sample at "
                     f"{8.0 * n / c[0] * 1e-9:.2f} TB/s")
        del x
        torch.cuda.empty_cache()
    T = SHAPES[0][2]
    xh = signal(1, 1, T).reshape(T).cpu()
    t0 = time.perf_counter()
    wide(xh)
    lines.append(f"(d) host path (NumPy blocks, scipy.signal.lfilter for the damping filter, one call, wall clock) on one row of {T}: "
                 f"{(time.perf_counter() - t0) * 1e3:.0f} ms")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
