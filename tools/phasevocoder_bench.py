"""Phase vocoder (float32) on one MI355X: the spectra of 64 x 2 880 000 samples (64 rows of one minute at 48 kHz) and of
2 x 28 800 000 (a ten-minute stereo file) at n_fft / hop = 2048 / 512 and 1024 / 256 (Hann, centred), stretched at rate 0.8 and 1.25.

It times, in the same run and alternating, on the same device tensors,
  (a) ``torchfx_amd.phase_vocoder`` -- one or two launches: the spectrum read once, the stretched one written once;
  (b) the torch-ops composition on the same spectrum: ``torchaudio.functional.phase_vocoder``'s formula written out below (pad,
      two ``index_select`` gathers, ``angle`` / ``abs``, the wrap, ``cumsum`` along the strided frame axis, ``polar``), so
      torchaudio need not be installed;
  (c) ``torchfx_amd.time_stretch`` whole -- stft, (a), istft, no copy between them;
  (d) ``stft`` + (b) + ``torch.istft``;
  (e) one ``gain_forward`` pass over the stretched spectrum, for scale: its read-once / write-once rate.
Times are device events around one call; min / median / max of --repeats are all recorded and the minimum is the figure.  No time
is gated.  The byte model of (a) is the input once (rate > 1: the frames an output stands on, at most two per output) plus the
output once; beside it stands what (e)'s rate would make of those bytes -- the rest is float64 atan2 and sincospi.

With --lock it times instead, on the same eight cases and tensors: (a) the identity phase-locked kernel, (b) the plain kernel,
(c) ``time_stretch(..., phase_lock="identity")`` whole, (d) ``time_stretch`` whole; --plain times the plain kernel alone (what a
build without the locked route can run, for the same-session comparison of the untouched code).

    python tools/phasevocoder_bench.py --out profiles/phasevocoder_bench.txt
    python tools/phasevocoder_bench.py --lock --out profiles/phasevocoder_lock_bench.txt
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

GEOMETRIES = [(2048, 512), (1024, 256)]
SHAPES = [(64, 2_880_000), (2, 28_800_000)]
RATES = [0.8, 1.25]
WARM = 2


def composition(X: torch.Tensor, rate: float, phase_advance: torch.Tensor) -> torch.Tensor:
    """torchaudio.functional.phase_vocoder, line by line."""
    real = torch.float32 if X.dtype == torch.complex64 else torch.float64
    time_steps = torch.arange(0, X.shape[-1], rate, device=X.device, dtype=real)
    alphas = time_steps % 1.0
    phase_0 = X[..., :1].angle()
    Xp = torch.nn.functional.pad(X, [0, 2])
    c0 = Xp.index_select(-1, time_steps.long())
    c1 = Xp.index_select(-1, (time_steps + 1).long())
    angle_0, angle_1, norm_0, norm_1 = c0.angle(), c1.angle(), c0.abs(), c1.abs()
    phase = angle_1 - angle_0 - phase_advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + phase_advance
    phase = torch.cat([phase_0, phase[..., :-1]], dim=-1)
    phase_acc = torch.cumsum(phase, -1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    return torch.polar(mag, phase_acc)


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


def lock_report(repeats: int, plain_only: bool) -> list[str]:
    """The locked route beside the plain one (or, ``plain_only``, the plain kernel alone)."""
    from torchfx_amd import phase_vocoder, stft, time_stretch, torchfx_ext as E
    from torchfx_amd.spectral import named_window

    lines = [f"phase vocoder, {'plain kernel alone' if plain_only else 'identity phase locking beside the plain kernel'}, float32 on "
             f"{torch.cuda.get_device_name(0)}; device events around one call, min / median / max of {repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    for rows, T in SHAPES:
        for n_fft, hop in GEOMETRIES:
            x = torch.randn(rows, T, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda", dtype=torch.float32) * 0.25
            w = named_window("hann", n_fft, torch.float32, x.device)
            X = stft(x, n_fft, hop, window=w)
            bins, frames = X.shape[-2:]
            for rate in RATES:
                case = f"{rows} x {T}, n_fft {n_fft} hop {hop}, rate {rate}"
                if plain_only:
                    b, = time_alternating([lambda: phase_vocoder(X, rate)], repeats)
                    lines.append(f"{case}: plain kernel {fmt(b)}")
                    continue
                p = E.phase_vocoder_plan_info(frames, bins, rate, rows, torch.float32, 0, 1)
                a, b, c, d = time_alternating([lambda: phase_vocoder(X, rate, phase_lock="identity"), lambda: phase_vocoder(X, rate),
                                               lambda: time_stretch(x, rate, n_fft, hop, window=w, phase_lock="identity"),
                                               lambda: time_stretch(x, rate, n_fft, hop, window=w)], repeats)
                lines.append(json.dumps(dict(rows=rows, samples=T, n_fft=n_fft, hop=hop, rate=rate, frames=frames, plan=p, locked_ms=a,
                                             plain_ms=b, time_stretch_locked_ms=c, time_stretch_ms=d, locked_over_plain=a[0] / b[0])))
                lines.append(f"{case} ({frames} -> {p['out_frames']} frames; {p['threads']} lanes x {p['bins_per_thread']} bins, "
                             f"{p['lds_bytes']} B LDS, {p['segments']} segments of {p['seg_frames']}, {p['workgroups']} workgroups): "
                             f"(a) locked {fmt(a)}   (b) plain {fmt(b)}   a/b {a[0] / b[0]:.2f}x   (c) time_stretch locked {fmt(c)}   "
                             f"(d) time_stretch {fmt(d)}   c/d {c[0] / d[0]:.2f}x")
            del X, x
            torch.cuda.empty_cache()
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lock", action="store_true", help="the locked route beside the plain one")
    ap.add_argument("--plain", action="store_true", help="the plain kernel alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("phasevocoder_bench needs a ROCm device")
    if args.lock or args.plain:
        text = "\n".join(lock_report(args.repeats, args.plain))
        print(text, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    from torchfx_amd import phase_vocoder, stft, time_stretch, torchfx_ext as E
    from torchfx_amd.spectral import named_window

    lines = [f"phase vocoder, float32 on {torch.cuda.get_device_name(0)}; device events around one call, "
             f"min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    faster = faster_whole = cases = 0
    for rows, T in SHAPES:
        for n_fft, hop in GEOMETRIES:
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn(rows, T, generator=g, device="cuda", dtype=torch.float32) * 0.25
            w = named_window("hann", n_fft, torch.float32, x.device)
            X = stft(x, n_fft, hop, window=w)
            bins, frames = X.shape[-2:]
            pa = torch.linspace(0, math.pi * hop, bins, device=x.device)[..., None]
            for rate in RATES:
                info = E.phase_vocoder_plan_info(frames, bins, rate, rows)
                length = int(round(T / rate))
                ours = lambda: phase_vocoder(X, rate)                                                         # noqa: E731
                ref = lambda: composition(X, rate, pa)                                                        # noqa: E731
                whole = lambda: time_stretch(x, rate, n_fft, hop, window=w)                                   # noqa: E731
                whole_ref = lambda: torch.istft(composition(stft(x, n_fft, hop, window=w), rate, pa), n_fft, hop, window=w,   # noqa: E731
                                                length=length)
                Y, Yc = ours(), ref()
                head = float((Y[..., :16] - Yc[..., :16]).abs().max()) / float(Yc[..., :16].abs().max())
                Yr = torch.view_as_real(Y.transpose(-1, -2))                 # the contiguous buffer [rows, Fo, bins, 2]
                del Yc
                a, b, c, d, e = time_alternating([ours, ref, whole, whole_ref, lambda: E.gain_forward(Yr, 0.5)], args.repeats)
                read = min(frames, 2 * info["out_frames"]) if rate > 1 else frames
                model = 8.0 * rows * bins * (read + info["out_frames"])
                gain_rate = 2 * 8.0 * rows * bins * info["out_frames"] / e[0] * 1e-9
                cases += 1
                faster += a[0] < b[0]
                faster_whole += c[0] < d[0]
                row = dict(rows=rows, samples=T, n_fft=n_fft, hop=hop, rate=rate, frames=frames, out_frames=info["out_frames"],
                           bin_tile=info["bin_tile"], segments=info["segments"], seg_frames=info["seg_frames"], launches=info["launches"],
                           workgroups=info["workgroups"], scratch_bytes=info["scratch_bytes"], vocoder_ms=a, composition_ms=b,
                           time_stretch_ms=c, torch_chain_ms=d, gain_ms=e, composition_over_ours=b[0] / a[0],
                           torch_chain_over_ours=d[0] / c[0], model_bytes=model, ours_TBs=model / a[0] * 1e-9, gain_TBs=gain_rate,
                           model_floor_ms=model / gain_rate * 1e-9, share_of_model_floor=model / gain_rate * 1e-9 / a[0],
                           max_rel_diff_first_16_frames=head)
                lines.append(json.dumps(row))
                lines.append(f"{rows} x {T}, n_fft {n_fft} hop {hop}, rate {rate} ({frames} -> {info['out_frames']} frames, "
                             f"{info['segments']} segments, {info['launches']} launches): (a) phase_vocoder {fmt(a)}   (b) composition {fmt(b)}   "
                             f"b/a {b[0] / a[0]:.2f}x   (c) time_stretch {fmt(c)}   (d) stft + composition + torch.istft {fmt(d)}   "
                             f"d/c {d[0] / c[0]:.2f}x   (e) gain_forward {fmt(e)}   (a) moves {model * 1e-9:.2f} GB by the model at "
                             f"{model / a[0] * 1e-9:.2f} TB/s ((e): {gain_rate:.2f} TB/s); the model's bytes at (e)'s rate take "
                             f"{model / gain_rate * 1e-9:.3f} ms = {model / gain_rate * 1e-9 / a[0]:.2f} of (a); the first 16 frames differ "
                             f"from (b) by {head:.1e} of their peak")
                del Y, Yr
                torch.cuda.empty_cache()
            del X, x
            torch.cuda.empty_cache()
    lines.append(f"phase_vocoder is faster than the composition in {faster} of {cases} cases, time_stretch faster than "
                 f"stft + composition + torch.istft in {faster_whole} of {cases}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
