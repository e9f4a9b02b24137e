"""YIN pitch detection (float32, centred, zero padding, fmin 65 Hz) on one MI355X: 64 x 2 880 000 and 2 x 28 800 000 samples at
48 kHz with frame / window / hop = 2048 / 1024 / 512, and 256 x 160 000 at 16 kHz with 1024 / 512 / 160 (gcd = 32: the plan sums every frame alone),
each with and without ``return_cmndf``.

It times, in the same run and alternating, on the same device tensors,
  (a) ``torchfx_amd.yin`` -- one launch of csrc/yin.hip, partial sums shared between overlapping frames;
  (b) the same kernel with ``block = win_length``: every frame sums on its own (what the sharing buys);
  (c) the float32 autocorrelation-form composition in torch ops: ``unfold``-ed frames, ``rfft`` / ``irfft`` for r(tau), a running
      energy from a cumulative sum, d = E(0) + E(tau) - 2 r(tau), the normalisation and the same pick;
  (d) one ``gain_forward`` pass over the input -- the read-once / write-once floor of the signal itself.
Times are device events around one call, every shape warmed up; min / median / max of --repeats are recorded and the minimum is
the figure.  No time is gated.  The (sample, lag) pairs of the definition, rows x frames x W x (Lmax + 1), over (a)'s time are
set against the packed-float32 rate of the part (157.3 TFLOP/s: 39.3e12 subtract + multiply-add pairs a second; the scalar
instructions the kernel uses reach 30.9e12, tools/ubench/valu_rate.hip).  Accuracy: the largest |d' - d'_64| of (a) and of (c) against the
float64 kernel on the first two rows' first 400 000 samples.

    python tools/yin_bench.py --out profiles/yin_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (rows, T, fs, frame_length, win_length, hop)
CASES = [(64, 2_880_000, 48000.0, 2048, 1024, 512), (2, 28_800_000, 48000.0, 2048, 1024, 512), (256, 160_000, 16000.0, 1024, 512, 160)]
FMIN, FMAX, THRESHOLD, WARM = 65.0, 2093.0, 0.1, 2
PACKED_PAIRS = 157.3e12 / 4            # a pair is a subtraction and a fused multiply-add: 4 of the peak's flops per packed lane pair


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


def composition(x, fs, n, W, hop, tau_min, tau_max, want_cmndf):
    """YIN from torch ops in float32, the autocorrelation form: (f0, aperiodicity[, cmndf])."""
    Lmax = tau_max + 1
    fr = torch.nn.functional.pad(x, (n // 2, n // 2)).unfold(-1, n, hop)[..., :W + Lmax]
    nfft = 1 << (W + Lmax - 1).bit_length()
    r = torch.fft.irfft(torch.fft.rfft(fr[..., :W], nfft).conj() * torch.fft.rfft(fr, nfft), nfft)[..., :Lmax + 1]
    c = torch.nn.functional.pad(fr.square().cumsum(-1), (1, 0))
    E = c[..., W:W + Lmax + 1] - c[..., :Lmax + 1]
    d = E[..., :1] + E - 2 * r
    lag = torch.arange(1, Lmax + 1, device=x.device, dtype=x.dtype)
    S = d[..., 1:].cumsum(-1)
    cm = torch.cat([torch.ones_like(d[..., :1]), torch.where(S == 0, torch.ones_like(S), lag * d[..., 1:] / S)], -1)
    win = cm[..., tau_min:tau_max + 1]
    under = win < THRESHOLD
    first = under.float().argmax(-1, keepdim=True)
    idx = torch.arange(win.shape[-1], device=x.device)
    stop = (cm[..., tau_min + 1:tau_max + 2] >= win) | (idx == win.shape[-1] - 1)            # where the walk down ends
    walked = (stop & (idx >= first)).float().argmax(-1, keepdim=True)
    tau = tau_min + torch.where(under.any(-1, keepdim=True), walked, win.argmin(-1, keepdim=True))
    a, b, cc = cm.gather(-1, tau - 1), cm.gather(-1, tau), cm.gather(-1, tau + 1)
    den = a - 2 * b + cc
    delta = torch.where((den > 0) & (b <= a) & (b <= cc), 0.5 * (a - cc) / den, torch.zeros_like(den))
    out = ((fs / (tau + delta)).squeeze(-1), b.squeeze(-1))
    return out + (cm,) if want_cmndf else out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yin_bench needs a ROCm device")
    from torchfx_amd import torchfx_ext as E, yin

    lines = [f"yin, float32, centred (zeros), fmin {FMIN} on {torch.cuda.get_device_name(0)}; device events around one call, "
             f"min / median / max of {args.repeats} alternating repeats, ms"]
    fmt = lambda t: f"{t[0]:.3f} / {t[1]:.3f} / {t[2]:.3f}"          # noqa: E731
    faster = 0
    for rows, T, fs, n, W, hop in CASES:
        g = torch.Generator(device="cuda").manual_seed(1)
        t = torch.arange(T, device="cuda", dtype=torch.float64) / fs
        x = sum(torch.sin(2 * torch.pi * 110.0 * k * t) / k for k in range(1, 5)).to(torch.float32) * 0.4
        x = (x + 0.05 * torch.randn(rows, T, generator=g, device="cuda", dtype=torch.float32)).contiguous()
        del t
        info = E.yin_plan_info(T, fs, FMIN, FMAX, n, W, hop, rows)
        alone = E.yin_plan_info(T, fs, FMIN, FMAX, n, W, hop, rows, block=W)
        tau_min, tau_max = info["tau_min"], info["tau_max"]
        small = x[:2, :min(T, 400_000)].contiguous()
        kw = dict(fmin=FMIN, fmax=FMAX, frame_length=n, win_length=W, hop_length=hop)
        ref = yin(small.double(), fs, return_cmndf=True, **kw)[1]
        err_ours = float((yin(small, fs, return_cmndf=True, **kw)[1].double() - ref).abs().max())
        comp = composition(small, fs, n, W, hop, tau_min, tau_max, True)
        err_comp = float((comp[2].double() - ref).abs().max())
        voiced = yin(small, fs, return_aperiodicity=True, **kw)
        same_f0 = float(((voiced[0] - comp[0]).abs() < 0.5).float().mean())
        del ref, comp, voiced
        for want in (False, True):
            ours = lambda: yin(x, fs, return_aperiodicity=True, return_cmndf=want, **kw)                                       # noqa: E731
            direct = lambda: E.yin_forward(x, fs, n, W, hop, tau_min, tau_max, THRESHOLD, n // 2, "constant", want, W)      # noqa: E731
            torch_ops = lambda: composition(x, fs, n, W, hop, tau_min, tau_max, want)                                          # noqa: E731
            a, b, c, d = time_alternating([ours, direct, torch_ops, lambda: E.gain_forward(x, 0.5)], args.repeats)
            torch.cuda.empty_cache()
            pairs = float(rows) * info["frames"] * W * info["lags"]
            faster += a[0] < c[0]
            row = dict(rows=rows, length=T, fs=fs, frame_length=n, win_length=W, hop=hop, return_cmndf=want, frames=info["frames"],
                       lags=info["lags"], block=info["block"], blocks_per_frame=info["blocks_per_frame"],
                       frames_per_workgroup=info["frames_per_workgroup"], lds_bytes=info["lds_bytes"], workgroups=info["workgroups"],
                       unshared_frames_per_workgroup=alone["frames_per_workgroup"], yin_ms=a, unshared_ms=b, composition_ms=c, gain_ms=d,
                       composition_over_ours=c[0] / a[0], unshared_over_ours=b[0] / a[0], ours_over_gain=a[0] / d[0], pairs=pairs,
                       pairs_per_s=pairs / a[0] * 1e3, share_of_packed_rate=pairs / a[0] * 1e3 / PACKED_PAIRS,
                       unshared_pairs_per_s=pairs / b[0] * 1e3, unshared_share_of_packed_rate=pairs / b[0] * 1e3 / PACKED_PAIRS,
                       max_cmndf_err_ours=err_ours, max_cmndf_err_composition=err_comp, frames_within_half_hz_of_composition=same_f0)
            lines.append(json.dumps(row))
            lines.append(f"{rows} x {T} at {fs:.0f} Hz, {n} / {W} / {hop}, cmndf {want}: (a) yin {fmt(a)}   (b) unshared {fmt(b)}   "
                         f"(c) torch composition {fmt(c)}   (d) gain_forward {fmt(d)}   c/a {c[0] / a[0]:.2f}x   b/a {b[0] / a[0]:.2f}x   "
                         f"{pairs:.3e} pairs: {pairs / a[0] * 1e-9:.2f}e12 /s = {pairs / a[0] * 1e3 / PACKED_PAIRS:.3f} of the packed rate "
                         f"(unshared {pairs / b[0] * 1e3 / PACKED_PAIRS:.3f}); max |d' - d'_64|: ours {err_ours:.2e}, composition {err_comp:.2e}")
        del x
        torch.cuda.empty_cache()
    lines.append(f"the kernel is faster than the composition in {faster} of {2 * len(CASES)} cases")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
