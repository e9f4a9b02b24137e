"""BS.1770 block energies on one MI355X: 64 rows x 2 880 000 float32 samples (cfg-2 size, 60 s at 48 kHz) and 2 rows x
28 800 000 (a ten-minute stereo file).

It times, in the same run and alternating,
  (a) ``block_energy`` -- one launch of the measuring cascade kernel: reads 4 B per sample, writes 8 B per 4800 samples;
  (b) the composition a caller had to write from the library's existing ops: ``sos_forward`` with the K-weighting cascade
      and a float64 result (4 + 8 B per sample), then ``square`` and a segment ``sum`` in torch (8 + 8, 8 B per sample);
  (b32) the same with a float32 ``sos_forward`` result (4 + 4, then 4 + 4, 4): cheaper, and every sample rounded to 2^-24;
  (c) one plain ``sos_forward`` float32 -> float32 of the same two sections (8 B per sample),
and checks (a) against (b) to 1e-9 relative.  Times are device events around one call; min / median / max of --repeats are
all recorded, max - min being the run-to-run spread of this run.  The gate: every repeat of (a) is faster than every repeat
of (b) at both shapes.  The ratio (a) / (c) is recorded only.

    python tools/loudness_bench.py --out profiles/loudness_bench.txt
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
SHAPES = [(64, 2_880_000), (2, 28_800_000)]
WARM = 3


def composition(x, sos, nblk, block, out_dtype):
    from torchfx_amd import torchfx_ext as E

    y = E.sos_forward(x, None, sos, None, None, out_dtype=out_dtype)[0]
    return y[:, :nblk * block].view(x.shape[0], nblk, block).square().sum(-1, dtype=torch.float64)


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
        raise SystemExit("loudness_bench needs a ROCm device")
    from torchfx_amd import block_energy, kweighting_sos, torchfx_ext as E

    sos_np = kweighting_sos(FS)
    sos = torch.from_numpy(sos_np)
    block = FS // 10
    lines = [f"K-weighting at {FS} Hz, 100 ms sub-blocks, float32 signals on {torch.cuda.get_device_name(0)}; device events around one "
             f"call, min / median / max of {args.repeats} alternating repeats, ms"]
    ok = True
    for rows, length in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(rows, length, generator=g, device="cuda", dtype=torch.float32) * 2 - 1
        nblk = length * 10 // FS
        info = E.sos_block_energy_plan_info(sos_np, rows, length, FS, 10)
        sa = block_energy(x, FS)
        sb = composition(x, sos, nblk, block, torch.float64)
        diff = float(((sa - sb).abs() / sb).max())
        del sa, sb
        a, b, b32, c = time_alternating(
            [lambda: block_energy(x, FS), lambda: composition(x, sos, nblk, block, torch.float64),
             lambda: composition(x, sos, nblk, block, torch.float32), lambda: E.sos_forward(x, None, sos, None, None)[0]], args.repeats)
        n = rows * length
        row = dict(rows=rows, length=length, nblk=info["nblk"], nseg=info["nseg"], warm=info["warm"], block_energy_ms=a,
                   composition_f64_ms=b, composition_f32_ms=b32, forward_ms=c, composition_over_block_energy=b[0] / a[0],
                   block_energy_over_forward=a[0] / c[0], block_energy_GBs_at_4B=4.0 * n / a[0] * 1e-6, max_rel_diff=diff)
        lines.append(json.dumps(row))
        fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"      # noqa: E731
        lines.append(f"{rows} x {length}, {info['nseg']} segments per row: (a) block_energy {fmt(a)}   (b) sos_forward to float64 + square + "
                     f"segment sum {fmt(b)}   (b32) the same through float32 {fmt(b32)}   (c) one forward pass {fmt(c)}   "
                     f"b/a {b[0] / a[0]:.2f}x   a/c {a[0] / c[0]:.2f}x   spread of (a) {a[2] - a[0]:.3f}, of (b) {b[2] - b[0]:.3f}   "
                     f"(a) reads 4 B/sample at {4.0 * n / a[0] * 1e-9:.2f} TB/s   max rel |a - b| {diff:.2e}")
        ok = ok and diff <= 1e-9 and a[2] < b[0]
        del x
        torch.cuda.empty_cache()
    lines.append("gate: " + ("PASS" if ok else "FAIL") + " (block_energy within 1e-9 of the composition, and its slowest repeat faster than "
                 "the composition's fastest, both shapes)")
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
