"""The forward SOS cascade on filters with long memory, with and without the hand-off route (csrc/sos_route.h).

``sos_forward`` float32 -> float32 on 64 x 2 880 000 and 2 x 28 800 000 samples (60 s / 600 s at 48 kHz) for cfg 2's cascade (the
control: its halo plan must not move), four designs of the accuracy grid whose warm-up is in the hundred-thousands, and the
six-filter chain of the reference's API benchmark (three 20-65 Hz Chebyshev high-passes, three 5 kHz Butterworth low-passes).
Each is timed with ``TFX_SOS_HANDOFF=0`` (the halo plan alone) and automatically, alternating in the same run; device events
around one call, minimum / median of --repeats.  Then the library's own events split an automatic call into its launches
(end-state passes, scans, result pass).  On a checkout that has no hand-off route (no ``sos_route_info``) the tool times what
is there, so the same file measures the parent commit.

    python tools/sos_hard_bench.py --out profiles/sos_hard_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("TFX_ENV_DYNAMIC", "1")      # this tool flips TFX_SOS_HANDOFF inside one process

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 48000
SHAPES = ((64, 2_880_000), (2, 28_800_000))
WARM = 2
ROOFLINE = 8.0e12            # B/s


def cascades():
    import scipy.signal as sg

    from torchfx_amd import filter as F

    def sos_of(*fs_):
        for f in fs_:
            f.compute_coefficients()
        return torch.cat([f._sos for f in fs_]).contiguous().double()

    api = [F.HiChebyshev1(20, fs=FS), F.HiChebyshev1(60, fs=FS), F.HiChebyshev1(65, fs=FS),
           F.LoButterworth(5000, fs=FS), F.LoButterworth(4900, fs=FS), F.LoButterworth(4850, fs=FS)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))      # noqa: E731
    return {
        "cfg2 (control)": sos_of(F.LoButterworth(2000, order=6, fs=FS), F.ParametricEQ(frequency=1000, q=2.0, gain=3.0, fs=FS)),
        "hp20_butter4": t(sg.butter(4, 20, "highpass", fs=FS, output="sos")),
        "hp20_cheby1_4": t(sg.cheby1(4, 0.1, 20, "highpass", fs=FS, output="sos")),
        "notch50_q30": t(np.concatenate(sg.iirnotch(50, 30, fs=FS))[None]),
        "lp40_butter8": t(sg.butter(8, 40, fs=FS, output="sos")),
        "api chain (6 filters)": sos_of(*api),
    }


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
    return [(min(t), statistics.median(t)) for t in ts]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sos_hard_bench needs a ROCm device")
    from torchfx_amd import _lib, torchfx_ext as E

    lib = _lib.load()
    has_route = hasattr(E, "sos_route_info")
    lines = [f"sos_forward float32 -> float32 on {torch.cuda.get_device_name(0)}; device events around one call, min / median of "
             f"{args.repeats} alternating repeats, ms" + ("" if has_route else "   [no hand-off route in this checkout: one column]")]
    ok = True
    for rows, length in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(rows, length, generator=g, device="cuda", dtype=torch.float32) * 2 - 1
        n = rows * length
        lines.append(f"--- {rows} x {length}")
        for name, sos in cascades().items():
            def run(knob):
                def fn():
                    if knob is None:
                        os.environ.pop("TFX_SOS_HANDOFF", None)
                    else:
                        os.environ["TFX_SOS_HANDOFF"] = knob
                    return E.sos_forward(x, None, sos, None, None)[0]
                return fn
            row = dict(cascade=name, rows=rows, length=length, sections=int(sos.shape[0]), warmup=E.sos_plan_info(sos, refine=False)["warmup"])
            if not has_route:
                (t_min, t_med), = time_alternating([run(None)], args.repeats)
                row.update(ms=(t_min, t_med))
                lines.append(json.dumps(row))
                lines.append(f"{name}: {t_min:.3f} / {t_med:.3f} ms   {8.0 * n / t_min * 1e-9:.2f} TB/s of 8 B/sample")
                continue
            os.environ["TFX_SOS_HANDOFF"] = "0"
            off = E.sos_route_info(sos.numpy(), rows, length)
            os.environ.pop("TFX_SOS_HANDOFF")
            auto = E.sos_route_info(sos.numpy(), rows, length)
            (o_min, o_med), (a_min, a_med) = time_alternating([run("0"), run(None)], args.repeats)
            y0, y1 = run("0")(), run(None)()
            diff = float((y0.double() - y1.double()).abs().max()) / max(1.0, float(y0.abs().max()))
            del y0, y1
            # the launches of one automatic call, by the library's own events
            lib.tfx_prof_enable(1)
            lib.tfx_prof_collect()
            for _ in range(3):
                run(None)()
            torch.cuda.synchronize()
            prof = {k: v["total_ms"] / 3 for k, v in json.loads(lib.tfx_prof_collect().decode()).items()}
            lib.tfx_prof_enable(0)
            bps = auto["bytes_per_sample"]
            row.update(off=off, auto=auto, off_ms=(o_min, o_med), auto_ms=(a_min, a_med), speedup=o_min / a_min, launches_ms=prof,
                       auto_TBs=bps * n / a_min * 1e-9, auto_roofline=bps * n / a_min * 1e3 / ROOFLINE, max_diff=diff)
            lines.append(json.dumps(row))
            lines.append(f"{name}: HANDOFF=0 {off['route']} x{off['nseg']} {o_min:.3f} / {o_med:.3f}   automatic {auto['route']} x{auto['nseg']} "
                         f"of {auto['seg_len']}, {auto['passes']} pass(es) {a_min:.3f} / {a_med:.3f}   speed-up {o_min / a_min:.2f}x   "
                         f"{bps:.0f} B/sample at {bps * n / a_min * 1e-9:.2f} TB/s = {bps * n / a_min * 1e3 / ROOFLINE:.2f} of 8 TB/s   "
                         f"max |difference| {diff:.1e} of the scale   launches: " + "  ".join(f"{k} {v:.3f}" for k, v in prof.items()))
            if auto["route"] == "handoff":
                ok = ok and a_min < o_min
            else:
                ok = ok and auto == off
        del x
        torch.cuda.empty_cache()
    if has_route:
        lines.append("gate: " + ("PASS" if ok else "FAIL") + " (every cascade that hands off is faster than with TFX_SOS_HANDOFF=0; the others keep their plan)")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
