"""Short-time Fourier transform (Hann window, centred, reflect padding, float32) on one MI355X: n_fft / hop = 1024 / 256 and
2048 / 512, each on 64 x 2 880 000 samples (64 rows of one minute at 48 kHz) and on 2 x 28 800 000 (a ten-minute stereo file),
each as the complex STFT (``power=None``) and as the power spectrogram (``power=2``).

It times, in the same run and alternating, on the same device tensors,
  (a) ``torchfx_amd.spectrogram`` -- the one-launch LDS route: the signal read once, the result written once;
  (b) the composition ``torch.stft(..., return_complex=True)`` (plus ``.abs().square()`` for power): a padded copy, the frame
      matrix (n_fft / hop times the signal), the library FFT over it and, for power, another pass;
  (c) one ``gain_forward`` pass over the input -- the read-once / write-once floor of the signal itself.
Times are device events around one call; min / median / max of --repeats are all recorded and the minimum is the figure.  No time
is gated.  The byte model of (a) is the input once plus the output once; its rate and the share of the output-write floor
(output bytes at the rate (c) reaches) are printed beside it.

    python tools/stft_bench.py --out profiles/stft_bench.txt
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
        raise SystemExit("stft_bench needs a ROCm device")
    from torchfx_amd import spectrogram, torchfx_ext as E
    from torchfx_amd.spectral import named_window

    lines = [f"stft / spectrogram, Hann window, centred (reflect), float32 on {torch.cuda.get_device_name(0)}; device events around "
             f"one call, min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    faster = 0
    for rows, T in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(rows, T, generator=g, device="cuda", dtype=torch.float32) * 0.25
        for n_fft, hop in GEOMETRIES:
            w = named_window("hann", n_fft, torch.float32, x.device)
            info = E.stft_plan_info(n_fft, hop, n_fft, T, rows)
            assert info["route"] == "lds"
            for power in (None, 2.0):
                if power is None:
                    ref = lambda: torch.stft(x, n_fft, hop, window=w, return_complex=True)                     # noqa: E731
                else:
                    ref = lambda: torch.stft(x, n_fft, hop, window=w, return_complex=True).abs().square()      # noqa: E731
                ours = lambda: spectrogram(x, n_fft, hop, window=w, power=power)                               # noqa: E731
                got, exp = ours(), ref()
                scale = float(exp.abs().max())
                diff = float((got - exp).abs().max()) / scale
                del got, exp
                a, b, c = time_alternating([ours, ref, lambda: E.gain_forward(x, 0.5)], args.repeats)
                torch.cuda.empty_cache()
                in_bytes = 4.0 * rows * T
                out_bytes = (8.0 if power is None else 4.0) * rows * info["frames"] * (n_fft // 2 + 1)
                gain_rate = 2 * in_bytes / c[0] * 1e-9                       # TB/s of the read-once / write-once pass
                floor_ms = out_bytes / gain_rate * 1e-9
                faster += a[0] < b[0]
                row = dict(rows=rows, length=T, n_fft=n_fft, hop=hop, power=power, frames=info["frames"],
                           frames_per_workgroup=info["frames_per_workgroup"], lds_bytes=info["lds_bytes"], workgroups=info["workgroups"],
                           stft_ms=a, torch_ms=b, gain_ms=c, torch_over_ours=b[0] / a[0], ours_over_gain=a[0] / c[0],
                           model_bytes=in_bytes + out_bytes, ours_TBs=(in_bytes + out_bytes) / a[0] * 1e-9, gain_TBs=gain_rate,
                           output_write_floor_ms=floor_ms, share_of_output_write_floor=floor_ms / a[0], max_rel_diff_to_torch=diff)
                lines.append(json.dumps(row))
                lines.append(f"{rows} x {T}, n_fft {n_fft} hop {hop}, power {power}: (a) ours {fmt(a)}   (b) torch composition {fmt(b)}   "
                             f"(c) gain_forward {fmt(c)}   b/a {b[0] / a[0]:.2f}x   (a) moves {(in_bytes + out_bytes) * 1e-9:.2f} GB by the "
                             f"model at {(in_bytes + out_bytes) / a[0] * 1e-9:.2f} TB/s ((c): {gain_rate:.2f} TB/s); writing the output alone "
                             f"at (c)'s rate takes {floor_ms:.3f} ms = {floor_ms / a[0]:.2f} of (a); differs from (b) by {diff:.1e} of its peak")
        del x
        torch.cuda.empty_cache()
    lines.append(f"the one-launch route is faster than the composition in {faster} of {len(SHAPES) * len(GEOMETRIES) * 2} cases")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
