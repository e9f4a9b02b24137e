"""Chorus() at its defaults (3 voices, sine LFO, cubic interpolation, 20 ms +- 3 ms at 1.5 Hz, spread 0.25) on one MI355X at
float32 and 48 kHz: [32, 2, 2 880 000] (32 minutes of stereo in one-minute items), [1, 2, 28 800 000] (a ten-minute stereo file)
and [1024, 2, 96 000] (many short items).

It times, in the same run and alternating,
  (a) ``Chorus()`` -- one launch of modulated_delay_kernel: reads 4 B per sample-channel from HBM (the voices' re-reads are
      cache hits) and writes 4;
  (b) ``gain_forward`` on the same tensor -- the read-once / write-once floor of anything that maps a signal to a signal;
  (c) the composition a user writes today from torch ops on the device, in float64: ``arange``, ``sin``, ``floor``, four
      ``gather``s per voice and channel, the Lagrange weights and the blend;
and, in a second alternating loop of the same run, (a) again next to (a') ``Chorus()`` on the same memory viewed as
[1, B * C, T]: the same kernel and traffic, but every workgroup holds one row, so no LFO value is shared between batch items --
what the reuse across the batch buys (for B = 1 the two are the same call: the ratio shows the loop's noise).  Times are
device events around one call; min / median / max of --repeats are all recorded.

Gate: (a) agrees with (c) within the bound of tests/modulation_reference.py (float32: 2^-24 |ref| + tol, ref = (c) unrounded),
and the slowest repeat of (a) is faster than the fastest of (c).  (a) / (b) is recorded, not gated.

    python tools/modulation_bench.py --out profiles/modulation_bench.txt
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

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
    return torch.rand(B, C, T, generator=g, device="cuda", dtype=torch.float32).mul_(2.0).sub_(1.0)


def torch_composition(x, P, rounded=True):
    """The modulated delay from torch ops, float64: what a user writes without the kernel.  x [B, C, T] float32."""
    B, C, T = x.shape
    idx = torch.arange(T, device=x.device)
    n = idx.to(torch.float64)
    y = torch.empty(B, C, T, dtype=torch.float64, device=x.device)
    for c in range(C):
        xc = x[:, c, :].to(torch.float64)
        acc = P.dry * xc
        for base, depth, inc, phase, gain in P.table.tolist():
            z = phase + float(c) * P.spread
            t = n * inc
            a = (t - torch.floor(t)) + (z - math.floor(z))
            d = base + depth * torch.sin(2.0 * math.pi * a)
            i = torch.floor(d)
            f = d - i
            m = idx - i.to(torch.int64)

            def at(k):
                return torch.gather(xc, 1, k.clamp(0, T - 1).expand(B, T)) * (k >= 0)

            xd = ((-f * (f - 1.0) * (f - 2.0) / 6.0) * at(m + 1) + ((f + 1.0) * (f - 1.0) * (f - 2.0) / 2.0) * at(m)
                  + (-(f + 1.0) * f * (f - 2.0) / 2.0) * at(m - 1) + ((f + 1.0) * f * (f - 1.0) / 6.0) * at(m - 2))
            acc = acc + gain * xd
        y[:, c, :] = acc
    return y.to(torch.float32) if rounded else y


def excess_over_bound(got, ref, x, P):
    """Largest |got - ref| - (2^-24 |ref| + tol) over the tensor, tol per row from max|x| of the row (the tests' bound)."""
    rows = P.table.tolist()
    G = sum(abs(r[4]) for r in rows)
    k = 2.0 ** -47 * (abs(P.dry) + 1.25 * G) + 2.4 * sum(abs(r[4]) * (r[1] * 2.0 ** -47 + (r[0] + r[1]) * 2.0 ** -52) for r in rows)
    worst, dev = -math.inf, 0.0
    for b in range(x.shape[0]):                                       # item by item: bounds the float64 temporaries
        tol = x[b].abs().amax(-1, keepdim=True).to(torch.float64) * k
        d = (got[b].to(torch.float64) - ref[b]).abs()
        worst = max(worst, float((d - (2.0 ** -24 * ref[b].abs() + tol)).max()))
        dev = max(dev, float(d.max()))
    return worst, dev


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("modulation_bench needs a ROCm device")
    from torchfx_amd import Chorus, torchfx_ext as E

    eff = Chorus(fs=FS)
    P = eff.params(torch.float32)
    lines = [f"Chorus() at {FS} Hz, defaults ({len(P.table)} voices, {P.shape} LFO, {P.interpolation} interpolation, spread {P.spread}), "
             f"float32 on {torch.cuda.get_device_name(0)}; device events around one call, min / median / max of {args.repeats} "
             "alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    ok = True
    for B, C, T in SHAPES:
        x = signal(B, C, T)
        flat = x.view(1, B * C, T)
        info = E.modulated_delay_plan_info(T, P.table, B, C, P.interpolation)
        ref = torch_composition(x, P, rounded=False)
        excess, dev = excess_over_bound(eff(x), ref, x, P)
        del ref
        torch.cuda.empty_cache()
        a, b, c = time_alternating([lambda: eff(x), lambda: E.gain_forward(x, 0.5), lambda: torch_composition(x, P)], args.repeats)
        torch.cuda.empty_cache()
        # the reuse across the batch, in a loop of its own: next to (c) whichever call follows it pays for (c)'s cache footprint
        a2, a1 = time_alternating([lambda: eff(x), lambda: eff(flat)], args.repeats)
        n = B * C * T
        agrees, faster = excess <= 0.0, a[2] < c[0]
        ok = ok and agrees and faster
        row = dict(batch=B, channels=C, length=T, tile=info["tile"], tiles=info["tiles"], batch_items=info["batch_items"],
                   batch_groups=info["batch_groups"], chorus_ms=a, gain_ms=b, torch_ms=c, chorus_again_ms=a2, chorus_no_reuse_ms=a1,
                   chorus_over_gain=a[0] / b[0], torch_over_chorus=c[0] / a[0], no_reuse_over_reuse=a1[0] / a2[0],
                   chorus_TBs=8.0 * n / a[0] * 1e-9, gain_TBs=8.0 * n / b[0] * 1e-9, voice_samples_per_ns=len(P.table) * n / a[0] * 1e-6,
                   largest_deviation=dev, largest_excess_over_bound=excess, agrees=agrees, faster=faster)
        lines.append(json.dumps(row))
        lines.append(f"{B} x {C} x {T}, {info['tiles']} tiles per row, {info['batch_groups']} batch group(s) of up to {info['batch_items']}: "
                     f"(a) Chorus {fmt(a)}   (b) gain_forward {fmt(b)}   (c) torch float64 composition {fmt(c)}   "
                     f"second loop: (a) {fmt(a2)}   (a') Chorus without reuse across the batch {fmt(a1)}   a/b {a[0] / b[0]:.2f}x (by bytes: 1)   "
                     f"c/a {c[0] / a[0]:.1f}x   a'/a {a1[0] / a2[0]:.2f}x   (a) moves 8 B/sample-channel at {8.0 * n / a[0] * 1e-9:.2f} TB/s, (b) at "
                     f"{8.0 * n / b[0] * 1e-9:.2f} TB/s; (a) against (c): largest deviation {dev:.3e}, largest excess over the bound "
                     f"{excess:.3e} (<= 0 agrees); slowest (a) {'<' if faster else '>='} fastest (c)")
        del x, flat
        torch.cuda.empty_cache()
    lines.append("GATE: " + ("PASS" if ok else "FAIL") + " -- (a) agrees with (c) within the bound and the slowest repeat of (a) is faster "
                 "than the fastest of (c), on every shape")
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
