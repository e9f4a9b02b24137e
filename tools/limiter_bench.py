"""Look-ahead true-peak limiter (defaults: -1 dBTP, 72 samples of look-ahead, 480 of hold, 4x oversampled detector, linked
stereo) on one MI355X: float32 [32, 2, 2 880 000] (32 minutes of stereo in one-minute items) and [1, 2, 28 800 000] (a ten-minute
stereo file) at 48 kHz.

It times, in the same run and alternating,
  (a) ``limit`` -- one launch: reads 4 B per sample-channel and writes 4;
  (b) the composition from existing device ops: ``resample_poly(x, 4, 1)`` (a temporary of 4x the signal), ``abs``, two ``amax``
      (over the phases, over the channels), a division, ``max_pool1d`` (the windowed minimum), ``conv1d`` (the smoothing) and
      the multiply;
  (c) ``gain_forward`` -- the read-once / write-once floor of anything that scales a signal,
and checks (a) against (b) to the smoothing sum's rounding.  Times are device events around one call; min / median / max of
--repeats are all recorded.  The gate: every repeat of (a) is faster than every repeat of (b) at both shapes.  The ratio
(a) / (c) is recorded only.

    python tools/limiter_bench.py --out profiles/limiter_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 48000
SHAPES = [(32, 2, 2_880_000), (1, 2, 28_800_000)]
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


def composition(x, P, w_flipped):
    """Steps 1-7 of ``limit`` for linked ``x [B, C, T]`` from the library's resampler and torch ops."""
    from torchfx_amd import resample_poly

    B, C, T = x.shape
    q = resample_poly(x, P.up, 1).abs().reshape(B, C, T, P.up).amax(-1)
    p = torch.maximum(torch.maximum(x.abs(), q), F.pad(q, (1, 0))[..., :-1]).amax(1, keepdim=True)
    del q
    r = torch.where(p > P.c, P.c / p, torch.ones_like(p))
    m = -F.max_pool1d(-F.pad(r, (P.H - 1 + P.A - 1, P.A - 1), value=1.0), P.A + P.H - 1, 1)
    s = F.conv1d(1 - m, w_flipped)
    return torch.minimum((1 - s).clamp_min(0), r) * x


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("limiter_bench needs a ROCm device")
    from torchfx_amd import limit, torchfx_ext as E
    from torchfx_amd.limiter import LimiterParams

    P = LimiterParams(FS, torch.float32)
    w_flipped = torch.from_numpy(P.w.copy()).flip(0).reshape(1, 1, -1).cuda()
    lines = [f"limiter at {FS} Hz: ceiling -1 dBTP, look-ahead {P.A}, hold {P.H} samples, {P.up}x oversampled detector "
             f"({P.taps.numel()} taps), linked stereo, float32 on {torch.cuda.get_device_name(0)}; device events around one call, "
             f"min / median / max of {args.repeats} alternating repeats, ms"]
    ok = True
    for B, C, T in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = (torch.rand(B, C, T, generator=g, device="cuda", dtype=torch.float32) * 2 - 1) * 1.5
        info = E.limiter_plan_info(T, P.A, P.H, P.up, int(P.taps.numel()))
        err = float((limit(x, FS) - composition(x, P, w_flipped)).abs().max())
        a, b, c = time_alternating([lambda: limit(x, FS), lambda: composition(x, P, w_flipped), lambda: E.gain_forward(x, 0.5)],
                                   args.repeats)
        n = B * C * T
        fma = n * (P.up * info["Lp"] + P.A / C)                          # useful fmas per sample-channel: the chain + A / C
        row = dict(batch=B, channels=C, length=T, Lp=info["Lp"], tile=info["tile"], tiles=info["tiles"], lds_bytes=info["lds_bytes"],
                   limit_ms=a, composition_ms=b, gain_ms=c, composition_over_limit=b[0] / a[0], limit_over_gain=a[0] / c[0],
                   limit_GBs_at_8B=8.0 * n / a[0] * 1e-6, limit_Gfma_per_s=fma / a[0] * 1e-6, max_abs_diff=err)
        lines.append(json.dumps(row))
        fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"      # noqa: E731
        lines.append(f"{B} x {C} x {T}, {info['tiles']} tiles of {info['tile']} per group: (a) limit {fmt(a)}   (b) composition {fmt(b)}   "
                     f"(c) gain_forward {fmt(c)}   b/a {b[0] / a[0]:.2f}x   a/c {a[0] / c[0]:.2f}x   spread of (a) {a[2] - a[0]:.3f}, "
                     f"of (b) {b[2] - b[0]:.3f}, of (c) {c[2] - c[0]:.3f}   (a) moves 8 B/sample at {8.0 * n / a[0] * 1e-9:.2f} TB/s and "
                     f"runs {fma / a[0] * 1e-9:.1f} T fma/s   max |a - b| {err:.2e}")
        ok = ok and err <= 2e-5 and a[2] < b[0]
        del x
        torch.cuda.empty_cache()
    lines.append("gate: " + ("PASS" if ok else "FAIL") + " (limit within 2e-5 of the composition, and its slowest repeat faster than the "
                 "composition's fastest, both shapes)")
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
