"""Inverse short-time Fourier transform (Hann window, centred, float32) on one MI355X: n_fft / hop = 1024 / 256 and 2048 / 512,
each on the spectrum of 64 x 2 880 000 samples (64 rows of one minute at 48 kHz) and of 2 x 28 800 000 (a ten-minute stereo file)
-- the four shapes of tools/stft_bench.py, read back.

It times, in the same run and alternating, on the same device tensors,
  (a) ``torchfx_amd.istft`` -- the one-launch overlap-add route: the spectrum read once (plus the frames at the tile edges, which
      two workgroups transform), the signal written once, the envelope flag read back (one synchronisation, as torch has);
  (b) ``torch.istft`` on the same spectrum: the library inverse FFT into a frame matrix (n_fft / hop times the signal), the window
      product, the fold, a second folded array for the envelope, the division and its own envelope check;
  (c) one ``gain_forward`` pass over the output -- the read-once / write-once floor of the signal itself.
Times are device events around one call; min / median / max of --repeats are all recorded and the minimum is the figure.  No time
is gated.  The byte model of (a) is the spectrum once, times 1 / (1 - redundant share) for the frames read twice, plus the output
once; its rate is printed beside the rate (c) reaches.

    python tools/istft_bench.py --out profiles/istft_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMETRIES = [(1024, 256), (2048, 512)]
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
        raise SystemExit("istft_bench needs a ROCm device")
    from torchfx_amd import istft, stft, torchfx_ext as E
    from torchfx_amd.spectral import named_window

    lines = [f"istft, Hann window, centred, float32 on {torch.cuda.get_device_name(0)}; device events around one call, "
             f"min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    faster = 0
    for rows, T in SHAPES:
        for n_fft, hop in GEOMETRIES:
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn(rows, T, generator=g, device="cuda", dtype=torch.float32) * 0.25
            w = named_window("hann", n_fft, torch.float32, x.device)
            X = stft(x, n_fft, hop, window=w)
            del x
            frames = X.shape[-1]
            info = E.istft_plan_info(n_fft, hop, n_fft, frames, rows)
            assert info["route"] == "lds"
            ours = lambda: istft(X, n_fft, hop, window=w)                                                     # noqa: E731
            ref = lambda: torch.istft(X, n_fft, hop, window=w)                                                # noqa: E731
            got, exp = ours(), ref()
            diff = float((got - exp).abs().max()) / float(exp.abs().max())
            y = got
            del exp
            a, b, c = time_alternating([ours, ref, lambda: E.gain_forward(y, 0.5)], args.repeats)
            in_bytes = 8.0 * rows * frames * (n_fft // 2 + 1)
            out_bytes = 4.0 * rows * info["length"]
            model = in_bytes / (1.0 - info["redundant_share"]) + out_bytes
            gain_rate = 2 * out_bytes / c[0] * 1e-9                          # TB/s of the read-once / write-once pass
            faster += a[0] < b[0]
            row = dict(rows=rows, samples=T, n_fft=n_fft, hop=hop, frames=frames, length=info["length"], tile=info["tile"],
                       frames_per_batch=info["frames_per_batch"], lds_bytes=info["lds_bytes"], workgroups=info["workgroups"],
                       redundant_share=info["redundant_share"], istft_ms=a, torch_ms=b, gain_ms=c, torch_over_ours=b[0] / a[0],
                       ours_over_gain=a[0] / c[0], model_bytes=model, ours_TBs=model / a[0] * 1e-9, gain_TBs=gain_rate,
                       model_floor_ms=model / gain_rate * 1e-9, share_of_model_floor=model / gain_rate * 1e-9 / a[0],
                       max_rel_diff_to_torch=diff)
            lines.append(json.dumps(row))
            lines.append(f"{rows} x {T}, n_fft {n_fft} hop {hop} ({frames} frames, tile {info['tile']}, redundant share "
                         f"{info['redundant_share']:.3f}): (a) ours {fmt(a)}   (b) torch.istft {fmt(b)}   (c) gain_forward {fmt(c)}   "
                         f"b/a {b[0] / a[0]:.2f}x   (a) moves {model * 1e-9:.2f} GB by the model at {model / a[0] * 1e-9:.2f} TB/s "
                         f"((c): {gain_rate:.2f} TB/s); the model's bytes at (c)'s rate take {model / gain_rate * 1e-9:.3f} ms = "
                         f"{model / gain_rate * 1e-9 / a[0]:.2f} of (a); differs from (b) by {diff:.1e} of its peak")
            del X, y, got
            torch.cuda.empty_cache()
    lines.append(f"the one-launch route is faster than torch.istft in {faster} of {len(SHAPES) * len(GEOMETRIES)} cases")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
