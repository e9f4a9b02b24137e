"""Noise gate (defaults: -40 dB threshold, 6 dB hysteresis, infinite range, 1 ms attack, 50 ms hold, 100 ms release, linked
stereo) on one MI355X at float32 and 48 kHz: [32, 2, 2 880 000] (64 rows of one minute) and [1, 2, 28 800 000] (a ten-minute
stereo file), where the plan cuts a row into segments and runs three launches, and [1024, 2, 96 000], where the groups alone
fill the chip and the plan takes one launch.

It times, in the same run and alternating, on the same tensors,
  (a) ``gate`` -- three launches: reads 12 B per sample-channel and writes 4; one launch: reads 4 and writes 4;
  (b) ``gain_forward`` -- the read-once / write-once floor of anything that scales a signal;
  (c) ``compress`` -- the stage that follows the gate in a chain; it moves the same bytes with the same work unit,
and, once, (d) the NumPy host path on a CPU copy of the smallest shape.  Times are device events around one call; min / median /
max of --repeats are all recorded and the minimum is the figure.  No time is gated.  The expectation under test: the gate needs no
log10 / exp10, so (a) should not be slower than (c).  The signal is phrases of noise at -12 dBFS with pauses at -66 dBFS (0.4 s
on, 0.35 s off), so the gate opens and closes all along every row (the share of open samples is recorded per shape).

    python tools/gate_bench.py --out profiles/gate_bench.txt
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
SHAPES = [(32, 2, 2_880_000), (1, 2, 28_800_000), (1024, 2, 96_000)]
WARM = 2


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
    x = torch.randn(B, C, T, generator=g, device="cuda", dtype=torch.float32) * 0.25
    n = torch.arange(T, device="cuda", dtype=torch.int64)
    phrase = ((n % int(0.75 * FS)) < int(0.4 * FS)).to(torch.float32)
    return x.mul_(phrase * (1.0 - 0.002) + 0.002)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gate_bench needs a ROCm device")
    from torchfx_amd import compress, gate, torchfx_ext as E

    lines = [f"gate at {FS} Hz, defaults, linked stereo, float32 on {torch.cuda.get_device_name(0)}; device events around one "
             f"call, min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    for B, C, T in SHAPES:
        x = signal(B, C, T)
        info = E.gate_plan_info(T, B, C)
        cinfo = E.compressor_plan_info(T, B, C)
        open_share = float(gate(x[:1], FS, return_open=True)[1].float().mean())
        a, b, c = time_alternating([lambda: gate(x, FS), lambda: E.gain_forward(x, 0.5), lambda: compress(x, FS)], args.repeats)
        n = B * C * T
        bytes_per = 16.0 if info["segments"] > 1 else 8.0
        row = dict(batch=B, channels=C, length=T, tile=info["tile"], tiles=info["tiles"], segments=info["segments"],
                   seg_tiles=info["seg_tiles"], scratch_bytes=info["scratch_bytes"], compressor_segments=cinfo["segments"],
                   open_share=open_share, gate_ms=a, gain_ms=b, compress_ms=c, gate_over_gain=a[0] / b[0],
                   gate_over_compress=a[0] / c[0], bytes_per_sample_channel=bytes_per, gate_TBs=bytes_per * n / a[0] * 1e-9,
                   gain_TBs=8.0 * n / b[0] * 1e-9, group_samples_per_us=B * T / a[0] * 1e-3)
        lines.append(json.dumps(row))
        lines.append(f"{B} x {C} x {T}, {info['tiles']} tiles in {info['segments']} segment(s) per group, gate open for {open_share:.0%} of "
                     f"the samples: (a) gate {fmt(a)}   (b) gain_forward {fmt(b)}   (c) compress {fmt(c)}   a/b {a[0] / b[0]:.2f}x "
                     f"(by bytes: {bytes_per / 8:.0f})   a/c {a[0] / c[0]:.2f}x   spread of (a) {a[2] - a[0]:.3f}, of (b) {b[2] - b[0]:.3f}   "
                     f"(a) moves {bytes_per:.0f} B/sample-channel at {bytes_per * n / a[0] * 1e-9:.2f} TB/s, (b) 8 at "
                     f"{8.0 * n / b[0] * 1e-9:.2f} TB/s")
        del x
        torch.cuda.empty_cache()
    B, C, T = min(SHAPES, key=lambda s: s[0] * s[1] * s[2])
    xh = signal(B, C, T).cpu()
    t0 = time.perf_counter()
    gate(xh, FS)
    lines.append(f"(d) host path (NumPy scans, one call, wall clock) on {B} x {C} x {T}: {(time.perf_counter() - t0) * 1e3:.0f} ms")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
