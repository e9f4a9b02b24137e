"""StatefulResample on one MI355X: a long signal converted chunk by chunk against one ``resample_poly`` call on the whole of it.

For each rate pair (64 rows x 60 s of float32 at the source rate, chunks of 65 536 frames) it prints
  * the wall time of the whole chunked pass (every chunk, then ``flush()``; chunks are contiguous device tensors made
    beforehand, as a decoder hands them over), host clock around a synchronised pass, min / median of --repeats;
  * the wall time of one ``resample_poly`` call on the whole signal (device events), min / median;
  * whether the chunked pass is ``torch.equal`` to the one-shot call;
  * with --trace: the resample kernels' time from ``rocprofv3 --kernel-trace`` in a run of its own (``--hip-only`` is that
    run's workload): the stream kernels summed over one pass against the one-shot kernel, and their ratio (goal <= 1.25).
A second table is the real-time case: 2 x 512-frame chunks at 44.1k -> 48k and 48k -> 44.1k, eager, time per chunk (host
clock around a synchronised loop of chunks, after warm-up, median of --groups groups), next to ``resample_poly`` on one chunk.

    python tools/stream_resample_bench.py --json out.json                        # timings
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/stream_resample_bench.py --hip-only
    python tools/stream_resample_bench.py --report out.json --trace DIR          # the table, with kernel times
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import re
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, SECONDS, CHUNK = 64, 60, 65536
PAIRS = [(44100, 48000), (48000, 44100), (48000, 8000)]
RT_PAIRS = [(44100, 48000), (48000, 44100)]
WARM = 2


def signal(rows, T, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(rows, T, generator=g, device="cuda", dtype=torch.float32) * 2 - 1


def chunks_of(x, size):
    return [x[:, o:o + size].contiguous() for o in range(0, x.shape[-1], size)]


def stream_pass(r, chunks):
    outs = [r(c) for c in chunks]
    outs.append(r.flush())
    return outs


def time_pass(fn, repeats):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), statistics.median(ts)


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


def per_chunk_us(fn, chunk, groups, per_group=200):
    for _ in range(20):
        fn(chunk)
    torch.cuda.synchronize()
    ts = []
    for _ in range(groups):
        t0 = time.perf_counter()
        for _ in range(per_group):
            fn(chunk)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / per_group * 1e6)
    return statistics.median(ts)


def run(args):
    from torchfx_amd import resample_poly, torchfx_ext
    from torchfx_amd.realtime import StatefulResample
    from torchfx_amd.resample import design_taps

    out = []
    for src, dst in PAIRS:
        r = StatefulResample(dst, src)
        up, down = r.up, r.down
        T = src * SECONDS
        x = signal(ROWS, T)
        chunks = chunks_of(x, CHUNK)
        taps = design_taps(up, down, r.window, torch.float32).numel()
        ref = resample_poly(x, up, down)
        got = torch.cat(stream_pass(r, chunks), dim=-1)
        equal = bool(torch.equal(got, ref))
        del got
        st = time_pass(lambda: stream_pass(r, chunks), args.repeats)
        one = time_call(lambda: resample_poly(x, up, down), args.repeats)
        row = dict(pair=f"{src}->{dst}", up=up, down=down, rows=ROWS, T=T, chunk=CHUNK, n_chunks=len(chunks),
                   n_out=ref.shape[-1], latency=r.latency, history=r.history_length,
                   stream_kernel=torchfx_ext.resample_stream_plan_info(0, CHUNK, up, down, taps)["kernel"],
                   one_shot_kernel=torchfx_ext.resample_plan_info(T, up, down, taps)["kernel"],
                   stream_pass_ms_min=st[0], stream_pass_ms_median=st[1], one_shot_ms_min=one[0], one_shot_ms_median=one[1],
                   torch_equal=equal)
        out.append(row)
        print(json.dumps(row), flush=True)
        del x, chunks, ref
        torch.cuda.empty_cache()
    for src, dst in RT_PAIRS:
        r = StatefulResample(dst, src)
        w = signal(2, 512, seed=2)
        st = per_chunk_us(r, w, args.groups)
        one = per_chunk_us(lambda c: resample_poly(c, r.up, r.down), w, args.groups)
        row = dict(pair=f"{src}->{dst}", rows=2, chunk=512, mode="eager", stream_us_per_chunk=st, one_shot_us_per_chunk=one)
        out.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def hip_only(args):
    """The profiled run, pair by pair in PAIRS order: WARM + repeats one-shot calls, then WARM + repeats chunked passes."""
    from torchfx_amd import resample_poly
    from torchfx_amd.realtime import StatefulResample

    for src, dst in PAIRS:
        r = StatefulResample(dst, src)
        x = signal(ROWS, src * SECONDS)
        chunks = chunks_of(x, CHUNK)
        for _ in range(WARM + args.repeats):
            resample_poly(x, r.up, r.down)
        for _ in range(WARM + args.repeats):
            stream_pass(r, chunks)
        torch.cuda.synchronize()
        del x, chunks
        torch.cuda.empty_cache()


def _is_stream(name: str) -> bool:
    """The STREAM template argument of a resample_kernel dispatch, demangled (``<float, 24, true, true>``) or mangled."""
    m = re.search(r"resample_kernel<([^>]*)>", name)
    if m:
        return m.group(1).replace(" ", "").split(",")[-1] == "true"
    m = re.search(r"resample_kernelI.*Lb([01])EEEv", name)
    if m:
        return m.group(1) == "1"
    raise SystemExit(f"cannot read the kernel variant of {name!r}")


def kernel_times(trace_dir, repeats):
    """Per pair: (one-shot kernel ms per call, stream kernels ms summed per pass), median over the repeats."""
    import csv

    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if "resample_kernel" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), _is_stream(r["Kernel_Name"])))
    rows.sort()
    res, i = [], 0
    for src, dst in PAIRS:
        per_pass = math.ceil(src * SECONDS / CHUNK) + 1              # the chunks and the flush
        one = rows[i:i + WARM + repeats]
        i += WARM + repeats
        st = rows[i:i + (WARM + repeats) * per_pass]
        i += (WARM + repeats) * per_pass
        if any(s for _, _, s in one) or not all(s for _, _, s in st) or len(st) != (WARM + repeats) * per_pass:
            raise SystemExit(f"{src}->{dst}: the trace's resample dispatches do not follow the --hip-only workload")
        one_ms = [(e - s) * 1e-6 for s, e, _ in one[WARM:]]
        passes = [sum((e - s) * 1e-6 for s, e, _ in st[k * per_pass:(k + 1) * per_pass]) for k in range(WARM, WARM + repeats)]
        res.append((statistics.median(one_ms), statistics.median(passes)))
    if i != len(rows):
        raise SystemExit(f"expected {i} resample dispatches, found {len(rows)}")
    return res


def report(args):
    with open(args.report) as f:
        rows = json.load(f)
    big = [r for r in rows if r.get("chunk") == CHUNK]
    rt = [r for r in rows if r.get("chunk") == 512]
    kt = kernel_times(args.trace, args.repeats) if args.trace else [(float("nan"), float("nan"))] * len(big)
    print(f"{ROWS} rows x {SECONDS} s float32, chunks of {CHUNK}, kaiser(5.0) taps; times in ms")
    print(f"{'pair':14s} {'up/down':>9s} {'chunks':>6s} {'pass min':>9s} {'pass med':>9s} {'1-shot min':>10s} {'1-shot med':>10s} "
          f"{'k stream':>9s} {'k 1-shot':>9s} {'k ratio':>7s} {'equal':>5s}  kernels")
    for r, (k1, ks) in zip(big, kt):
        r.update(kernel_one_shot_ms=k1, kernel_stream_pass_ms=ks, kernel_ratio=ks / k1)
        print(f"{r['pair']:14s} {str(r['up']) + '/' + str(r['down']):>9s} {r['n_chunks']:6d} {r['stream_pass_ms_min']:9.3f} "
              f"{r['stream_pass_ms_median']:9.3f} {r['one_shot_ms_min']:10.3f} {r['one_shot_ms_median']:10.3f} {ks:9.3f} {k1:9.3f} "
              f"{ks / k1:7.3f} {str(r['torch_equal']):>5s}  {r['stream_kernel']} / {r['one_shot_kernel']}")
    print("pass: every chunk then flush(), host clock around a synchronised pass; 1-shot: resample_poly on the whole signal, "
          "device events; k: kernel time from rocprofv3 --kernel-trace (a separate run), stream summed over one pass")
    print(f"\n{'real time':14s} {'rows x chunk':>12s} {'stream us':>9s} {'1-shot us':>9s}")
    for r in rt:
        print(f"{r['pair']:14s} {'2 x 512':>12s} {r['stream_us_per_chunk']:9.1f} {r['one_shot_us_per_chunk']:9.1f}")
    print("per chunk, eager: host clock around a synchronised loop of 200 chunks, median of the groups; "
          "1-shot: resample_poly on the chunk alone (no history: not a stream, the launch cost for comparison)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--groups", type=int, default=11)
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
