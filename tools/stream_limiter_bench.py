"""StatefulLimiter per chunk on one MI355X, next to what a user could write without it: ``limit`` on
``torch.cat([hist, chunk])``, sliced to the chunk's outputs, plus the history slice.  float32 at 48 kHz, the default
parameters (look-ahead 72, hold 480, 4x detector: latency 81, history 642), linked stereo, chunks of 512 ... 65536 frames,
eager and as a replayed HIP graph (``StreamProcessor(use_graph=True)``'s step).  Time per chunk = host clock around a
synchronised loop of chunks, after warm-up: the median of the groups, with their minimum and maximum.  A second table times
the kernels alone (the library's events around each launch): the stream kernel on a 2 x 512 chunk against the one-shot kernel
on the same ``Hs + 512`` samples -- where the stream kernel's restricted sweep shows.

    python tools/stream_limiter_bench.py [--out profiles/stream_limiter_bench.txt] [--json out.json] [--groups 11]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS = 48000
CHUNKS = [512, 2048, 8192, 65536]


def baseline(D: int, Hs: int):
    """The user's composition: the one-shot limiter on [hist | chunk], the outputs the chunk completes, the history slice."""
    from torchfx_amd.effect import FX
    from torchfx_amd.limiter import limit

    class CatOneShot(FX):
        def __init__(self):
            super().__init__()
            self._hist = None

        def forward(self, x):
            if self._hist is None:
                self._hist = torch.zeros(x.shape[0], Hs, dtype=x.dtype, device=x.device)
            v = torch.cat([self._hist, x], dim=-1)
            y = limit(v, FS)[..., Hs - D:Hs - D + x.shape[-1]]
            self._hist = v[:, x.shape[-1]:]
            return y

    return CatOneShot()


def per_chunk_us(sp, w, graph: bool, groups: int, per_group: int) -> tuple[float, float, float]:
    step = (lambda: sp._graph_step(w)) if graph else (lambda: sp._run(w))
    while True:                                           # the carried state exists and the limiter's counter has saturated
        sp._run(w)
        if sp._graphable(w):
            break
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(groups):
        t0 = time.perf_counter()
        for _ in range(per_group):
            step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / per_group * 1e6)
    return statistics.median(times), min(times), max(times)


def kernel_us(fn, name: str, n=100, groups=11) -> tuple[float, float, float]:
    """Device time per launch of kernel ``name`` (the library's own events around each launch, ``tfx_prof_collect``), n calls
    per group after warm-up: median, minimum and maximum of the groups."""
    from torchfx_amd import _lib

    lib = _lib.load()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    lib.tfx_prof_enable(1)
    lib.tfx_prof_collect()
    for _ in range(groups):
        for _ in range(n):
            fn()
        prof = json.loads(lib.tfx_prof_collect().decode())[name]
        times.append(prof["total_ms"] / prof["calls"] * 1e3)
    lib.tfx_prof_enable(0)
    return statistics.median(times), min(times), max(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "stream_limiter_bench.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--groups", type=int, default=11)
    args = ap.parse_args()
    from torchfx_amd import torchfx_ext as E
    from torchfx_amd.limiter import LimiterParams
    from torchfx_amd.realtime import StatefulLimiter, StreamProcessor

    lines, rows = [], []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    probe = StatefulLimiter(fs=FS)
    D, Hs = probe.latency, probe.history_length
    say(f"StatefulLimiter, float32, 48 kHz, defaults (A 72, H 480, 4x detector): latency {D}, history {Hs}; linked stereo; "
        f"{torch.cuda.get_device_name(0)}")
    say(f"per chunk, host clock around a synchronised loop, median [min .. max] of {args.groups} groups, microseconds")
    say(f"{'chunk':>6s} {'mode':6s} {'stateful us':>26s} {'cat + one-shot us':>26s} {'speed-up':>8s}")
    for T in CHUNKS:
        g = torch.Generator(device="cuda").manual_seed(T)
        w = (torch.rand(2, T, generator=g, device="cuda") * 2 - 1) * 1.2        # over the ceiling now and then
        per_group = max(10, min(200, 2_000_000 // T))
        for graph in (False, True):
            res = []
            for fx in (StatefulLimiter(fs=FS), baseline(D, Hs)):
                sp = StreamProcessor([fx], chunk_size=T, device="cuda", use_graph=graph)
                if not isinstance(fx, StatefulLimiter):
                    sp._graphable = lambda w: True
                res.append(per_chunk_us(sp, w, graph, args.groups, per_group))
            mode = "graph" if graph else "eager"
            rows.append(dict(chunk=T, mode=mode, stateful_us=res[0], baseline_us=res[1]))
            fmt = lambda r: f"{r[0]:8.1f} [{r[1]:6.1f} .. {r[2]:6.1f}]"          # noqa: E731
            say(f"{T:6d} {mode:6s} {fmt(res[0]):>26s} {fmt(res[1]):>26s} {res[1][0] / res[0][0]:7.2f}x")
    say("")
    say("kernels alone (the library's events around each launch, 100 launches per group): a 2 x 512 chunk")
    P = LimiterParams(FS, torch.float32)
    wv = torch.from_numpy(P.w)
    x = (torch.rand(2, 512, device="cuda") * 2 - 1) * 1.2
    h = (torch.rand(2, Hs, device="cuda") * 2 - 1) * 1.2
    v = torch.cat([h, x], dim=-1)
    info = E.limiter_stream_plan_info(512, P.A, P.H, P.up, int(P.taps.numel()))
    st = kernel_us(lambda: E.limiter_stream_forward(x, h, Hs + D, P.c, P.A, P.H, wv, P.up, P.taps, 2),
                   "limiter_stream_kernel", groups=args.groups)
    one = kernel_us(lambda: E.limiter_forward(v, P.c, P.A, P.H, wv, P.up, P.taps, 2), "limiter_kernel", groups=args.groups)
    rows.append(dict(chunk=512, mode="kernel", stream_us=st, one_shot_us=one, positions=info["positions"]))
    say(f"limiter_stream_kernel ({info['positions']} of 8192 positions swept): {st[0]:7.2f} [{st[1]:.2f} .. {st[2]:.2f}] us")
    say(f"limiter_kernel on the same {Hs} + 512 samples:            {one[0]:7.2f} [{one[1]:.2f} .. {one[2]:.2f}] us")
    say("(the stream kernel also writes the new history)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
