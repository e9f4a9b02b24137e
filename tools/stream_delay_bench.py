"""StatefulDelay / StatefulReverb per chunk on one MI355X, next to what a user writes today without them: the one-shot
effect on ``torch.cat([hist, chunk])``, sliced to the chunk, plus the history slice.  Rows 2, chunks of 512 ... 65536
frames, eager and as a replayed HIP graph (``StreamProcessor(use_graph=True)``'s step).  Time per chunk = host clock around
a synchronised loop of chunks, after warm-up, median of 11 groups.  ``model us`` is the bytes model e*rows*(2T + 2H) of one
chunk (read chunk and history, write output and new history) at the 6.29 TB/s device-copy rate.  A second table times the
kernels alone (device events): the stream kernel on a chunk against the one-shot kernel the library picks for that chunk.

    python tools/stream_delay_bench.py [--json out.json] [--groups 11]
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

COPY_TBS = 6.29
CHUNKS = [512, 2048, 8192, 65536]


def effects():
    from torchfx_amd.effect import PingPongDelayStrategy
    from torchfx_amd.realtime import StatefulDelay, StatefulReverb
    return [  # name, factory of the stateful effect, H
        ("delay mono D=12000 taps=3", lambda: StatefulDelay(bpm=120, delay_time="1/8", fs=48000), 36000),
        ("delay pingpong D=12000 taps=3", lambda: StatefulDelay(bpm=120, delay_time="1/8", fs=48000,
                                                                strategy=PingPongDelayStrategy()), 36000),
        ("delay mono D=12000 taps=70", lambda: StatefulDelay(bpm=120, delay_time="1/8", fs=48000, taps=70), 840000),
        ("reverb D=4410", lambda: StatefulReverb(4410), 4410),
    ]


def baseline(make):
    """The user's composition: the one-shot effect (its plain class) on [hist | chunk], the chunk's part, the history slice."""
    from torchfx_amd.effect import FX, Delay, Reverb

    inner = make()
    one_shot = Reverb(inner.delay, inner.decay, inner.mix) if isinstance(inner, Reverb) else \
        Delay(delay_samples=inner.delay_samples, feedback=inner.feedback, mix=inner.mix, taps=inner.taps, strategy=inner.strategy)
    H = inner.delay if isinstance(inner, Reverb) else inner.taps * inner.delay_samples

    class CatOneShot(FX):
        def __init__(self):
            super().__init__()
            self._hist = None

        def forward(self, x):
            if self._hist is None:
                self._hist = torch.zeros(x.shape[0], H, dtype=x.dtype, device=x.device)
            v = torch.cat([self._hist, x], dim=-1)
            y = one_shot(v)[..., H:H + x.shape[-1]]
            self._hist = v[:, x.shape[-1]:]
            return y

    return CatOneShot()


def per_chunk_us(sp, w, graph: bool, groups: int, per_group: int) -> float:
    step = (lambda: sp._graph_step(w)) if graph else (lambda: sp._run(w))
    sp._run(w)                                            # creates the carried state (the processor's first chunk)
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
    return statistics.median(times)


def kernel_us(fn, n=200) -> float:
    """Device time per call (events around n back-to-back calls, after warm-up)."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def kernel_table(rows: list) -> None:
    """The stream kernel against the one-shot kernel the library picks for the chunk alone (span, lattice or gather:
    it reads the chunk once and writes T + H samples, about the traffic of a streaming span / lattice variant)."""
    from torchfx_amd import torchfx_ext as E
    print(f"\n{'kernel-only':32s} {'chunk':>6s} {'stream us':>9s} {'one-shot us':>11s} {'one-shot kernel':>15s}")
    for name, D, taps, pp in (("delay mono D=12000 taps=3", 12000, 3, False), ("delay pingpong D=12000 taps=3", 12000, 3, True),
                              ("delay mono D=12000 taps=70", 12000, 70, False), ("reverb D=4410", 4410, 1, False)):
        for T in CHUNKS:
            w = torch.rand(2, T, device="cuda") * 2 - 1
            if name.startswith("reverb"):
                h = torch.rand(2, D, device="cuda")
                st = kernel_us(lambda: E.delay_line_stream_forward(w, h, D, 0.5, 0.5))
                one = kernel_us(lambda: E.delay_line_forward(w, D, 0.5, 0.5))
                regime = "delay_line" if T > D else "none (T <= D)"
            else:
                h = torch.rand(2, taps * D, device="cuda")
                st = kernel_us(lambda: E.delay_stream_forward(w, h, D, taps, 0.3, 0.2, pp))
                one = kernel_us(lambda: E.delay_forward(w, D, taps, 0.3, 0.2, pp))
                regime = E.delay_regime(D, taps, w.dtype, pp)
            rows.append(dict(effect=name, chunk=T, mode="kernel", stream_us=st, one_shot_us=one, one_shot_kernel=regime))
            print(f"{name:32s} {T:6d} {st:9.2f} {one:11.2f} {regime:>15s}", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--groups", type=int, default=11)
    args = ap.parse_args()
    from torchfx_amd.realtime import StreamProcessor

    rows = []
    print(f"{'effect':32s} {'chunk':>6s} {'mode':6s} {'stateful us':>11s} {'cat+1shot us':>12s} {'speed-up':>8s} {'model us':>8s}")
    for name, make, H in effects():
        for T in CHUNKS:
            g = torch.Generator(device="cuda").manual_seed(T)
            w = torch.rand(2, T, generator=g, device="cuda") * 2 - 1
            model_us = 4 * 2 * (2 * T + 2 * H) / (COPY_TBS * 1e12) * 1e6
            per_group = max(10, min(200, 2_000_000 // T))
            for graph in (False, True):
                res = []
                for fx in (make(), baseline(make)):
                    sp = StreamProcessor([fx], chunk_size=T, device="cuda", use_graph=graph)
                    res.append(per_chunk_us(sp, w, graph, args.groups, per_group))
                mode = "graph" if graph else "eager"
                rows.append(dict(effect=name, chunk=T, mode=mode, stateful_us=res[0], baseline_us=res[1], model_us=model_us,
                                 bytes=4 * 2 * (2 * T + 2 * H)))
                print(f"{name:32s} {T:6d} {mode:6s} {res[0]:11.1f} {res[1]:12.1f} {res[1] / res[0]:7.2f}x {model_us:8.2f}", flush=True)
    kernel_table(rows)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
