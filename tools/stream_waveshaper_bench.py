"""StatefulDistortion() (tanh, +12 dB, L = 4: latency 21, history 41) per chunk on one MI355X in float32, at 2 x 512 (a real-time
block) and 2 x 65 536 (a file-to-file chunk).

It times, in the same run and alternating,
  (a) ``StatefulDistortion()`` on the chunk -- one launch of waveshaper_stream_kernel, which reads [history | chunk] from their
      two buffers and writes the next history;
  (b) what a user could write without it: ``waveshape`` on ``torch.cat([history, chunk])``, the chunk's outputs sliced out, plus
      the history slice;
  (c) one ``gain_forward`` pass over the chunk -- the read-once / write-once floor of anything that maps a chunk to a chunk.
Times are device events around a loop of --inner calls (a 2 x 512 call is a few microseconds of device work: one pair of events
per call would time the events), divided by the loop length; min / median / max of --repeats (default 7) alternating repeats
are all recorded and the comparison uses the minima.  A second table times the kernels alone (the library's events around
each launch): the stream kernel on a 2 x 512 chunk against the one-shot kernel on the same ``Hs + 512`` samples.  Nothing is
gated on a time fixed in advance.

    python tools/stream_waveshaper_bench.py --out profiles/stream_waveshaper_bench.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNKS = [512, 65536]
WARM = 5


def time_alternating(fns, repeats: int, inner: int):
    for fn in fns:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b) / inner * 1e3)
    return [(min(t), statistics.median(t), max(t)) for t in ts]


def kernel_us(fn, name: str, n: int, repeats: int):
    """Device time per launch of kernel ``name`` (the library's own events around each launch, ``tfx_prof_collect``)."""
    from torchfx_amd import _lib

    lib = _lib.load()
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    times = []
    lib.tfx_prof_enable(1)
    lib.tfx_prof_collect()
    for _ in range(repeats):
        for _ in range(n):
            fn()
        prof = json.loads(lib.tfx_prof_collect().decode())[name]
        times.append(prof["total_ms"] / prof["calls"] * 1e3)
    lib.tfx_prof_enable(0)
    return min(times), statistics.median(times), max(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_waveshaper_bench needs a ROCm device")
    from torchfx_amd import torchfx_ext as E
    from torchfx_amd import waveshape
    from torchfx_amd.realtime import StatefulDistortion

    probe = StatefulDistortion()
    D, Hs = probe.latency, probe.history_length
    P = probe.params()
    up, dn = P.taps(torch.float32)
    fmt = lambda t: f"{t[0]:.2f} / {t[1]:.2f} / {t[2]:.2f}"          # noqa: E731
    lines = [f"StatefulDistortion() (tanh, +12 dB, L = 4: latency {D}, history {Hs}), float32, 2 rows, on {torch.cuda.get_device_name(0)}; "
             f"device events around {args.inner} calls, per call, min / median / max of {args.repeats} alternating repeats, microseconds"]
    for T in CHUNKS:
        g = torch.Generator(device="cuda").manual_seed(T)
        x = torch.rand(2, T, generator=g, device="cuda", dtype=torch.float32).mul_(2.0).sub_(1.0)
        fx = StatefulDistortion(aligned=False)
        while fx._pos < D + Hs:                               # a stream that has run for a while
            fx(x)
        state = {"hist": torch.zeros(2, Hs, device="cuda")}

        def cat_one_shot():
            v = torch.cat([state["hist"], x], dim=-1)
            y = waveshape(v, "tanh", drive_db=12.0)[..., Hs - D:Hs - D + T]
            state["hist"] = v[:, T:]
            return y

        a, b, c = time_alternating([lambda: fx(x), cat_one_shot, lambda: E.gain_forward(x, 0.5)], args.repeats, args.inner)
        info = E.waveshaper_stream_plan_info(T, 4, up.numel(), dn.numel())
        row = dict(chunk=T, latency=D, history=Hs, tiles=info["tiles"], positions=info["positions"], stateful_us=a, cat_one_shot_us=b,
                   gain_us=c, cat_over_stateful=b[0] / a[0], stateful_over_gain=a[0] / c[0])
        lines.append(json.dumps(row))
        lines.append(f"2 x {T}: (a) StatefulDistortion {fmt(a)}   (b) cat + waveshape + slices {fmt(b)}   (c) gain_forward {fmt(c)}   "
                     f"b/a {b[0] / a[0]:.2f}x   a/c {a[0] / c[0]:.2f}x")
    # the kernels alone on a real-time block
    x = torch.rand(2, 512, device="cuda").mul_(2.0).sub_(1.0)
    h = torch.rand(2, Hs, device="cuda").mul_(2.0).sub_(1.0)
    v = torch.cat([h, x], dim=-1)
    info = E.waveshaper_stream_plan_info(512, 4, up.numel(), dn.numel())
    st = kernel_us(lambda: E.waveshaper_stream_forward(x, h, Hs + D, 4, "tanh", None, P.drive, P.bias, P.dry, P.wet, up, dn),
                   "waveshaper_stream_kernel", 100, args.repeats)
    one = kernel_us(lambda: E.waveshaper_forward(v, 4, "tanh", None, P.drive, P.bias, P.dry, P.wet, up, dn), "waveshaper_kernel", 100,
                    args.repeats)
    lines.append(json.dumps(dict(chunk=512, mode="kernel", stream_us=st, one_shot_us=one, positions=info["positions"])))
    lines.append(f"kernels alone (the library's events around each launch, 100 launches per repeat), a 2 x 512 chunk: "
                 f"waveshaper_stream_kernel ({info['positions']} of 2048 positions up-sampled, 2 of 8 decimator chains, writes the new "
                 f"history) {fmt(st)}   waveshaper_kernel on the same {Hs} + 512 samples {fmt(one)}   "
                 f"stream {'<' if st[0] < one[0] else '>='} one-shot")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
