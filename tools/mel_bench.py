"""Mel spectrogram (Hann window, centred, reflect padding, float32, power 2, log "db") on one MI355X, 80 and 128 htk mels:
n_fft / hop = 1024 / 256 and 2048 / 512, each on 64 x 2 880 000 samples (64 rows of one minute at 48 kHz) and on 2 x 28 800 000
(a ten-minute stereo file), and a speech front end: 256 x 160 000 samples at 16 kHz, n_fft 512, hop 160, win_length 400.

It times, in the same run and alternating, on the same device tensors,
  (a) ``torchfx_amd.mel_spectrogram`` -- the one-launch LDS route: the signal read once, [rows, frames, n_mels] written once;
  (b) the composition: ``spectrogram(power=2)``, ``matmul`` with the filterbank, and the logarithm in torch ops -- the power
      spectrogram written, read back, and two more passes over the small result;
  (c) ``spectrogram(power=2)`` alone.
Times are device events around one call; min / median / max of --repeats are all recorded and the minimum is the figure.  No time
is gated; a/b and a/c are reported.

    python tools/mel_bench.py --out profiles/mel_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# rows, samples, sample rate, n_fft, hop, win_length
CASES = [(64, 2_880_000, 48000, 1024, 256, None), (64, 2_880_000, 48000, 2048, 512, None), (2, 28_800_000, 48000, 1024, 256, None),
         (2, 28_800_000, 48000, 2048, 512, None), (256, 160_000, 16000, 512, 160, 400)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mel_bench needs a ROCm device")
    from stft_bench import time_alternating
    from torchfx_amd import mel_filterbank, mel_spectrogram, spectrogram, torchfx_ext as E

    lines = [f"mel spectrogram, Hann window, centred (reflect), float32, power 2, log db on {torch.cuda.get_device_name(0)}; device events "
             f"around one call, min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    not_slower, x, shape = 0, None, None
    for rows, T, rate, n_fft, hop, wl in CASES:
        if shape != (rows, T):
            del x
            torch.cuda.empty_cache()
            x = torch.randn(rows, T, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda", dtype=torch.float32) * 0.25
            shape = (rows, T)
        for n_mels in (80, 128):
            fb = mel_filterbank(n_fft // 2 + 1, rate, n_mels, device=x.device)
            total = E.mel_band_table(fb.cpu().numpy())[1]
            info = E.mel_plan_info(n_fft, hop, wl or n_fft, T, rows, n_filters=n_mels, total_band=total)
            assert info["route"] == "lds", info
            ours = lambda: mel_spectrogram(x, rate, n_fft, hop, wl, n_mels=n_mels, log="db")                          # noqa: E731
            spec = lambda: spectrogram(x, n_fft, hop, wl, power=2.0)                                                   # noqa: E731

            def composed():
                v = torch.matmul(spec().transpose(-1, -2), fb).transpose(-1, -2)
                return torch.where(v < 1e-10, torch.full_like(v, 1e-10), v).log10() * 10.0

            got, exp = ours(), composed()
            diff = float((got - exp).abs().max())
            del got, exp
            a, b, c = time_alternating([ours, composed, spec], args.repeats)
            torch.cuda.empty_cache()
            in_bytes, out_bytes = 4.0 * rows * T, 4.0 * rows * info["frames"] * n_mels
            not_slower += a[0] <= b[0]
            row = dict(rows=rows, length=T, n_fft=n_fft, hop=hop, win_length=wl or n_fft, n_mels=n_mels, frames=info["frames"],
                       frames_per_workgroup=info["frames_per_workgroup"], lanes_per_filter=info["lanes_per_filter"], total_band=total,
                       lds_bytes=info["lds_bytes"], workgroups=info["workgroups"], mel_ms=a, composition_ms=b, spectrogram_ms=c,
                       composition_over_mel=b[0] / a[0], mel_over_spectrogram=a[0] / c[0], model_bytes=in_bytes + out_bytes,
                       mel_TBs=(in_bytes + out_bytes) / a[0] * 1e-9, max_abs_diff_db=diff)
            lines.append(json.dumps(row))
            lines.append(f"{rows} x {T}, n_fft {n_fft} hop {hop} win {wl or n_fft}, {n_mels} mels: (a) fused {fmt(a)}   (b) composition {fmt(b)}   "
                         f"(c) spectrogram alone {fmt(c)}   b/a {b[0] / a[0]:.2f}x   a/c {a[0] / c[0]:.2f}   (a) moves "
                         f"{(in_bytes + out_bytes) * 1e-9:.2f} GB by the model at {(in_bytes + out_bytes) / a[0] * 1e-9:.2f} TB/s; differs from (b) "
                         f"by {diff:.1e} dB")
    lines.append(f"the fused call takes no longer than the composition in {not_slower} of {2 * len(CASES)} cases")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
