"""Distortion() at its defaults (tanh, +12 dB of drive) on one MI355X in float32 at oversample 2, 4 and 8: [64, 2 880 000] and
[2, 28 800 000].

It times, in the same run and alternating,
  (a) ``Distortion(oversample=L)`` -- one launch of waveshaper_kernel: 4 B read and 4 B written per sample, the oversampled
      signal in LDS only;
  (b) ``gain_forward`` on the same tensor -- the read-once / write-once floor of anything that maps a signal to a signal;
  (c) the composition from the library's own ops on the device, ``resample_poly(tanh(resample_poly(x, L, 1) * drive), 1, L)``,
      which moves (2 + 4 L) signal-sized arrays;
  (d) ``Distortion(shape="hard", oversample=L)`` -- the same launch with the cheapest transfer function: (a) - (d) is what
      the rational tanh costs.
Times are device events around one call; min / median / max of --repeats (default 7) are all recorded, and the comparison uses
the minima next to the spread.  Nothing is gated on a time fixed in advance: the report says, per row, whether the slowest
repeat of (a) beats the fastest of (c), and the largest difference between (a) and (c) (two float32 tanh forms apart).

    python tools/waveshaper_bench.py --out profiles/waveshaper_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 2_880_000), (2, 28_800_000)]
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("waveshaper_bench needs a ROCm device")
    from torchfx_amd import Distortion, resample_poly, torchfx_ext as E

    lines = [f"Distortion() (tanh, +12 dB), float32 on {torch.cuda.get_device_name(0)}; device events around one call, "
             f"min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    for rows, T in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(rows, T, generator=g, device="cuda", dtype=torch.float32).mul_(2.0).sub_(1.0)
        for L in (2, 4, 8):
            eff, hard = Distortion(oversample=L), Distortion(shape="hard", oversample=L)
            drive = 10.0 ** (eff.drive_db / 20.0)

            def composition():
                return resample_poly(torch.tanh(resample_poly(x, L, 1) * drive), 1, L)

            dev = float((eff(x) - composition()).abs().max())
            torch.cuda.empty_cache()
            a, b, c, d = time_alternating([lambda: eff(x), lambda: E.gain_forward(x, 0.5), composition, lambda: hard(x)], args.repeats)
            torch.cuda.empty_cache()
            info = E.waveshaper_plan_info(T, L, 20 * L + 1, 20 * L + 1, 0, torch.float32)
            n = rows * T
            fmas = L * info["taps_up"] + info["taps_dn"]
            row = dict(rows=rows, length=T, oversample=L, tile=info["tile"], tiles=info["tiles"], lds_bytes=info["lds_bytes"],
                       distortion_ms=a, gain_ms=b, composition_ms=c, hard_ms=d, distortion_over_gain=a[0] / b[0], composition_over_distortion=c[0] / a[0],
                       slowest_distortion_beats_fastest_composition=a[2] < c[0], fma_per_sample=fmas,
                       tfma_per_s=fmas * n / a[0] * 1e-9, distortion_TBs=8.0 * n / a[0] * 1e-9, gain_TBs=8.0 * n / b[0] * 1e-9,
                       largest_difference_to_composition=dev)
            lines.append(json.dumps(row))
            lines.append(f"{rows} x {T}, L = {L}: (a) Distortion {fmt(a)}   (b) gain_forward {fmt(b)}   (c) composition {fmt(c)}   (d) hard clipper {fmt(d)}   "
                         f"a/b {a[0] / b[0]:.2f}x   c/a {c[0] / a[0]:.2f}x   (a) runs {fmas} fma per sample at "
                         f"{fmas * n / a[0] * 1e-9:.1f} Tfma/s and moves 8 B/sample at {8.0 * n / a[0] * 1e-9:.2f} TB/s; slowest (a) "
                         f"{'<' if a[2] < c[0] else '>='} fastest (c); largest |a - c| {dev:.2e}")
        del x
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
