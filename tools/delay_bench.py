"""Delay on one MI355X: the one-launch kernel (torchfx_ext.delay_forward) against the reference's composition run by torch
on the same device (strategy.apply_delay, zero pad, torch.lerp).  Prints one line per configuration: ms per call (device
events, after warm-up, >= 0.5 s of calls), the floor bytes e*(T + T + taps*D) per row divided by that time as a fraction
of the 6.29 TB/s device-copy rate, the composition's ms per call, and the max |difference| of the two outputs.

    python tools/delay_bench.py [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29
T60 = 60 * 48000
CONFIGS = [  # name, shape, dtype, D, taps, pingpong
    ("mono f32 64x60s D=12000 taps=3", (64, T60), torch.float32, 12000, 3, False),
    ("mono f32 64x60s D=12000 taps=8", (64, T60), torch.float32, 12000, 8, False),
    ("pingpong f32 32x2x60s D=12000 taps=3", (32, 2, T60), torch.float32, 12000, 3, True),
    ("pingpong f32 32x2x60s D=12000 taps=8", (32, 2, T60), torch.float32, 12000, 8, True),
    ("mono f32 64x60s D=37 taps=4", (64, T60), torch.float32, 37, 4, False),
    ("mono f64 8x60s D=12000 taps=8", (8, T60), torch.float64, 12000, 8, False),
]


def time_ms(fn, min_s=0.5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    one = max(a.elapsed_time(b), 1e-3)
    n = max(3, int(min_s * 1000 / one) + 1)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from torchfx_amd import torchfx_ext as E
    from torchfx_amd.effect import MonoDelayStrategy, PingPongDelayStrategy

    def composition(x, D, taps, fb, mix, pp):
        delayed = (PingPongDelayStrategy() if pp else MonoDelayStrategy()).apply_delay(x, D, taps, fb)
        pad = torch.zeros(*x.shape[:-1], delayed.size(-1), dtype=x.dtype, device=x.device)
        pad[..., :x.size(-1)] = x
        return torch.lerp(pad, delayed, mix)

    rows = []
    print(f"{'config':40s} {'regime':8s} {'ms/call':>9s} {'of copy':>8s} {'torch ms':>9s} {'speed-up':>8s} {'max|diff|':>10s}")
    for name, shape, dt, D, taps, pp in CONFIGS:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(shape, generator=g, device="cuda", dtype=dt) * 2 - 1
        fb, mix = 0.6, 0.35
        y = E.delay_forward(x, D, taps, fb, mix, pp)
        ref = composition(x, D, taps, fb, mix, pp)
        diff = float((y.double() - ref.double()).abs().max())
        del ref
        ms = time_ms(lambda: E.delay_forward(x, D, taps, fb, mix, pp))
        ms_ref = time_ms(lambda: composition(x, D, taps, fb, mix, pp))
        nrows, T = x.numel() // shape[-1], shape[-1]
        floor = nrows * x.element_size() * (2 * T + taps * D)
        frac = floor / (ms * 1e-3) / (COPY_TBS * 1e12)
        regime = E.delay_regime(D, taps, dt, pp)
        rows.append(dict(config=name, regime=regime, ms=ms, copy_fraction=frac, torch_ms=ms_ref, max_abs_diff=diff))
        print(f"{name:40s} {regime:8s} {ms:9.3f} {frac:8.2f} {ms_ref:9.3f} {ms_ref / ms:7.1f}x {diff:10.2e}", flush=True)
        del x, y
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
