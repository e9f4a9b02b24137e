"""The polyphase resampler on one MI355X: 64 rows x 60 s of float32 at the source rate, four rate pairs.

For each pair it prints
  * the call time of ``resample_poly`` on the device (device events around one call, min / median of --repeats);
  * the kernel time, from ``rocprofv3 --kernel-trace`` in a run of its own (``--hip-only`` is that run's workload,
    ``--trace`` reads its kernel_trace CSV back);
  * the HBM floor 4 * rows * (T + n_out) bytes at 6.3 TB/s and the share of it the kernel reaches;
  * two baselines: the strided-conv1d polyphase form (torchaudio's shape: conv1d(x[:, None], w[up, 1, W], stride=down),
    then transpose), built from the same taps and run by PyTorch on the same GPU; and SciPy's resample_poly on the host CPU.

    python tools/resample_bench.py --json out.json                       # timings and baselines
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/resample_bench.py --hip-only
    python tools/resample_bench.py --report out.json --trace DIR         # the table, with kernel times
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3
ROWS, SECONDS = 64, 60
PAIRS = [(44100, 48000), (48000, 44100), (48000, 16000), (16000, 48000)]
WARM = 3


def ratio(src, dst):
    g = math.gcd(src, dst)
    return dst // g, src // g


def signal(rows, T, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(rows, T, generator=g, device="cuda", dtype=torch.float32) * 2 - 1


def conv1d_weights(up, down, h, T):
    """Polyphase weights for conv1d(stride=down): output channel p at conv step k is y[k*up + p]."""
    from torchfx_amd import torchfx_ext

    info = torchfx_ext.resample_plan_info(T, up, down, h.numel())
    Lp, pre = info["Lp"], info["n_pre_remove"]
    half = (h.numel() - 1) // 2
    pre_pad = down - half % down
    hp = np.zeros(Lp * up)
    hp[pre_pad:pre_pad + h.numel()] = h.double().numpy()
    c = [(p + pre) * down // up for p in range(up)]
    W = Lp + max(c)
    w = np.zeros((up, 1, W))
    for p in range(up):
        ph = (p + pre) * down % up
        for j in range(Lp):
            w[p, 0, Lp - 1 + c[p] - j] = hp[ph + j * up]
    K = math.ceil(info["n_out"] / up)
    right = max(0, (K - 1) * down + W - T - (Lp - 1))
    return torch.from_numpy(w).float(), Lp - 1, right, info["n_out"]


def conv1d_resample(x, w, left, right, down, n_out):
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x[:, None], (left, right)), w, stride=down)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out]


def time_call(fn, repeats):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), statistics.median(ts)


def floor_ms(rows, T, n_out):
    return 4.0 * rows * (T + n_out) / (HBM_TBS * 1e12) * 1e3


def run(args):
    from scipy.signal import resample_poly as scipy_resample_poly

    from torchfx_amd import resample_poly, torchfx_ext
    from torchfx_amd.resample import design_taps

    out = []
    for src, dst in PAIRS:
        up, down = ratio(src, dst)
        T = src * SECONDS
        x = signal(ROWS, T)
        h = design_taps(up, down, ("kaiser", 5.0), torch.float32)
        info = torchfx_ext.resample_plan_info(T, up, down, h.numel())
        y = resample_poly(x, up, down)
        w, left, right, n_out = conv1d_weights(up, down, h, T)
        w = w.cuda()
        yc = conv1d_resample(x, w, left, right, down, n_out)
        diff = float((y - yc).abs().max())
        hip = time_call(lambda: resample_poly(x, up, down), args.repeats)
        conv = time_call(lambda: conv1d_resample(x, w, left, right, down, n_out), args.repeats)
        del yc
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        ys = scipy_resample_poly(xh, up, down, axis=-1)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        sdiff = float(np.abs(y.cpu().numpy() - ys).max())
        row = dict(pair=f"{src}->{dst}", up=up, down=down, rows=ROWS, T=T, n_out=n_out, taps=h.numel(), Lp=info["Lp"],
                   kernel=info["kernel"], lds_bytes=info["lds_bytes"], call_ms_min=hip[0], call_ms_median=hip[1],
                   floor_ms=floor_ms(ROWS, T, n_out), conv1d_ms_min=conv[0], conv1d_ms_median=conv[1],
                   scipy_cpu_ms=cpu_ms, max_diff_conv1d=diff, max_diff_scipy=sdiff)
        out.append(row)
        print(json.dumps(row), flush=True)
        del x, y, w, xh, ys
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def hip_only(args):
    """The profiled run: WARM + repeats resample calls per pair, pairs in PAIRS order, nothing else from the library."""
    from torchfx_amd import resample_poly

    for src, dst in PAIRS:
        up, down = ratio(src, dst)
        x = signal(ROWS, src * SECONDS)
        for _ in range(WARM + args.repeats):
            resample_poly(x, up, down)
        torch.cuda.synchronize()
        del x
        torch.cuda.empty_cache()


def kernel_times(trace_dir, repeats):
    """Per pair: (name, [ms per dispatch]) of the resample kernels in the trace, in dispatch order, warm-up calls dropped."""
    import csv

    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if "resample_kernel" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per = WARM + repeats
    if len(rows) != per * len(PAIRS):
        raise SystemExit(f"expected {per * len(PAIRS)} resample dispatches, found {len(rows)}")
    res = []
    for i in range(len(PAIRS)):
        grp = rows[i * per + WARM:(i + 1) * per]
        res.append((grp[0][2], [(e - s) * 1e-6 for s, e, _ in grp]))
    return res


def report(args):
    with open(args.report) as f:
        rows = json.load(f)
    kt = kernel_times(args.trace, args.repeats) if args.trace else [(None, None)] * len(rows)
    print(f"{ROWS} rows x {SECONDS} s float32, kaiser(5.0) taps; times in ms; floor = 4*rows*(T+n_out) B at {HBM_TBS} TB/s")
    hdr = (f"{'pair':14s} {'up/down':>9s} {'Lp':>4s} {'call min':>9s} {'call med':>9s} {'kernel min':>10s} {'kernel med':>10s} "
           f"{'floor':>7s} {'floor/kernel':>12s} {'conv1d min':>10s} {'conv1d/call':>11s} {'scipy CPU':>10s}")
    print(hdr)
    for r, (name, ks) in zip(rows, kt):
        kmin = min(ks) if ks else float("nan")
        kmed = statistics.median(ks) if ks else float("nan")
        r.update(kernel=r["kernel"], kernel_ms_min=kmin, kernel_ms_median=kmed, kernel_name=name)
        print(f"{r['pair']:14s} {str(r['up']) + '/' + str(r['down']):>9s} {r['Lp']:4d} {r['call_ms_min']:9.3f} {r['call_ms_median']:9.3f} "
              f"{kmin:10.3f} {kmed:10.3f} {r['floor_ms']:7.3f} {r['floor_ms'] / kmin:12.2f} {r['conv1d_ms_min']:10.3f} "
              f"{r['conv1d_ms_min'] / r['call_ms_min']:10.1f}x {r['scipy_cpu_ms']:10.0f}")
    print("conv1d: torch.nn.functional.conv1d(x[:, None], w[up, 1, W], stride=down) + transpose, same taps, same GPU; "
          "scipy CPU: scipy.signal.resample_poly on the host, one call over all rows")
    print("max |HIP - conv1d|: " + ", ".join(f"{r['pair']} {r['max_diff_conv1d']:.1e}" for r in rows)
          + "; max |HIP - scipy|: " + ", ".join(f"{r['pair']} {r['max_diff_scipy']:.1e}" for r in rows))
    if kt[0][0]:
        print("kernels (rocprofv3 --kernel-trace, a separate run): " + ", ".join(f"{r['pair']} {r['kernel_name']}" for r in rows))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--report", default=None, help="the --json file of a timing run")
    ap.add_argument("--trace", default=None, help="rocprofv3 output directory of a --hip-only run")
    args = ap.parse_args()
    if args.report:
        report(args)
    elif args.hip_only:
        hip_only(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
