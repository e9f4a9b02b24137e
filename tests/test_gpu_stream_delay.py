"""StatefulDelay / StatefulReverb on the device (csrc/delay.hip delay_stream_kernel, csrc/effects.hip
delay_line_stream_kernel): chunked output plus flush() is bit-identical (torch.equal) to the one-shot Delay / Reverb on the
same device and dtype, in real-time chunks (T <= D) and large chunks (T >> D), mono and ping-pong, with more than 64 taps,
on misaligned rows and with non-finite samples; HIP-graph replay equals eager; one launch per chunk."""
import json

import numpy as np
import pytest
import torch

from tests.gpu_common import DEV
from tests.test_stream_delay_host import _MemoryBackend, _random_sizes

pytestmark = pytest.mark.gpu


def _chunked(effect, x, sizes, flush=True):
    outs, o, n, sizes = [], 0, x.shape[-1], list(sizes)
    while o < n:
        k = sizes.pop(0) if sizes else n - o
        outs.append(effect(x[..., o:o + k]))
        o += k
    if flush:
        outs.append(effect.flush())
    return torch.cat(outs, dim=-1)


def _kw(D, taps, pp):
    from torchfx_amd.effect import PingPongDelayStrategy
    kw = dict(taps=taps, feedback=0.45, mix=0.35, strategy=PingPongDelayStrategy() if pp else None)
    if D == 0:
        kw.update(bpm=120.0, delay_time="1/8", fs=3)            # 0.25 s at 3 Hz: int(0.75) = 0 samples
    else:
        kw.update(delay_samples=D)
    from torchfx_amd import Delay
    assert Delay(**kw).delay_samples == D                    # the case is the delay it names (D = 0: no history)
    return kw


def _signal(shape, dtype, seed, offset=0):
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    base = torch.randn(n + offset, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    return base[offset:].view(*shape)                  # offset 1: rows that start off any 16-byte boundary


CASES = [  # (D, taps, length, chunk sizes)
    (12000, 3, 40000, [512] * 78),                     # real-time regime: 512-sample blocks against D = 12000
    (12000, 3, 140000, [65536, 65536]),                # T >> D
    (300, 8, 20000, [1, 7, 299, 300, 301, 905] * 4),
    (5, 70, 6000, [3, 500, 1000]),                     # taps > 64: amplitudes through the device table
    (0, 3, 3000, [7, 512]),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("pp", [False, True], ids=["mono", "pingpong"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_stream_equals_one_shot_on_device(dtype, pp, case):
    from torchfx_amd import Delay
    from torchfx_amd.realtime import StatefulDelay
    D, taps, n, sizes = CASES[case]
    for shape, off in (((2, n), 0), ((2, 2, n // 2), 1), ((n,), 1)):
        x = _signal(shape, dtype, case + 10 * off, off)
        ref = Delay(**_kw(D, taps, pp))(x)
        for sz in (sizes, _random_sizes(shape[-1], case, max(2 * D, 64))):
            y = _chunked(StatefulDelay(**_kw(D, taps, pp)), x, sz)
            assert y.shape == ref.shape and torch.equal(y, ref), (shape, off, sz[:4])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_non_finite_samples_land_where_the_one_shot_puts_them(dtype):
    from torchfx_amd import Delay
    from torchfx_amd.effect import PingPongDelayStrategy
    from torchfx_amd.realtime import StatefulDelay
    x = _signal((2, 30000), dtype, 3)
    x[0, 100] = float("nan")
    x[1, 7000] = float("inf")
    x[0, 20000] = float("-inf")
    for strat in (None, PingPongDelayStrategy()):
        ref = Delay(delay_samples=1200, taps=4, strategy=strat)(x)
        y = _chunked(StatefulDelay(delay_samples=1200, taps=4, strategy=strat), x, [512] * 40)
        assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.isnan(ref).any()
        fin = ~torch.isnan(ref)
        assert torch.equal(y[fin], ref[fin])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_reverb_stream_equals_one_shot_on_device(dtype):
    from torchfx_amd import Reverb
    from torchfx_amd.realtime import StatefulReverb
    for shape, off in (((2, 50000), 0), ((1, 2, 50000), 1), ((50000,), 1)):
        x = _signal(shape, dtype, 5, off)
        ref = Reverb(delay=4410, decay=0.6, mix=0.4)(x)
        for sizes in ([512] * 100, [8192] * 7, _random_sizes(50000, 9, 9000)):
            r = StatefulReverb(delay=4410, decay=0.6, mix=0.4)
            outs, o = [], 0
            for k in sizes:
                outs.append(r(x[..., o:o + k]))
                o += k
            assert torch.equal(torch.cat(outs, dim=-1)[..., :50000], ref), (shape, sizes[:3])
    short = _signal((2, 300), dtype, 6)
    assert torch.equal(StatefulReverb(delay=441)(short), Reverb(delay=441)(short))


def test_golden_cases_on_device(golden):
    from tests.test_gpu_delay import check
    from torchfx_amd.effect import PingPongDelayStrategy
    from torchfx_amd.realtime import StatefulDelay
    g = golden("delay_fx")
    for name in sorted({k.split("/")[0] for k in g.files}):
        p = g[f"{name}/params"]
        D, taps, fb, mix, pp, fs, bpm = float(p[0]), int(p[1]), float(p[2]), float(p[3]), bool(p[4]), int(p[5]), float(p[6])
        strat = PingPongDelayStrategy() if pp else None
        if bpm > 0:
            d = StatefulDelay(bpm=bpm, delay_time=str(g[f"{name}/delay_time"]), fs=fs, taps=taps, feedback=fb, mix=mix, strategy=strat)
        else:
            d = StatefulDelay(delay_samples=int(D), taps=taps, feedback=fb, mix=mix, strategy=strat)
        x, y = g[f"{name}/x"], g[f"{name}/y"]
        got = _chunked(d, torch.from_numpy(x).to(DEV), _random_sizes(x.shape[-1], 4, 300))
        check(got.cpu(), torch.from_numpy(y), name)


def _chain(taps=3):
    from torchfx_amd import filter as F
    from torchfx_amd.effect import Gain, PingPongDelayStrategy
    from torchfx_amd.realtime import StatefulDelay, StatefulReverb
    return [F.LoButterworth(3000, order=4, fs=48000), StatefulDelay(bpm=120, delay_time="1/16", taps=taps,
                                                                    strategy=PingPongDelayStrategy()),
            StatefulReverb(delay=4410), Gain(0.8)]


@pytest.mark.parametrize("taps", [3, 70])
@pytest.mark.parametrize("chunk", [512, 8192])
def test_graph_replay_equals_eager(taps, chunk):
    from torchfx_amd.realtime import StreamProcessor
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, chunk * 12)).astype(np.float32))
    eager = StreamProcessor(_chain(taps), chunk_size=chunk, device=DEV).process_tensor(x, 48000)
    sp = StreamProcessor(_chain(taps), chunk_size=chunk, device=DEV, use_graph=True)
    graph = sp.process_tensor(x, 48000)
    torch.cuda.synchronize()
    assert sp._graph is not None                       # the steps after the first were replayed
    assert graph.shape == x.shape and torch.equal(graph, eager)


@pytest.mark.parametrize("use_graph", [False, True])
def test_realtime_processor_on_device_gives_the_one_shot_signal(use_graph):
    from torchfx_amd import Delay, Reverb
    from torchfx_amd.realtime import RealtimeProcessor, StatefulDelay, StatefulReverb, StreamConfig
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 512 * 40)).astype(np.float32))
    be = _MemoryBackend()
    cfg = StreamConfig(sample_rate=48000, buffer_size=512, channels_in=2, channels_out=2)
    with RealtimeProcessor([StatefulDelay(bpm=120), StatefulReverb(delay=4410)], be, cfg, device=DEV, use_graph=use_graph):
        y = be.run(x, 512)
    xd = x.to(DEV)
    ref = Reverb(delay=4410)(Delay(delay_samples=12000)(xd)[:, :x.shape[-1]])
    assert torch.equal(y, ref.cpu())


def test_one_launch_per_chunk():
    from torchfx_amd import _lib
    from torchfx_amd.realtime import StatefulDelay, StatefulReverb, StreamProcessor
    lib = _lib.load()
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 512 * 20)).astype(np.float32))
    for eff, name in ((StatefulDelay(delay_samples=12000), "delay_stream_kernel"),
                      (StatefulDelay(delay_samples=5, taps=70), "delay_stream_kernel"),
                      (StatefulReverb(delay=4410), "delay_line_stream_kernel")):
        sp = StreamProcessor([eff], chunk_size=512, device=DEV)
        lib.tfx_prof_enable(1)
        lib.tfx_prof_collect()
        sp.process_tensor(x, 48000)
        torch.cuda.synchronize()
        prof = json.loads(lib.tfx_prof_collect().decode())
        lib.tfx_prof_enable(0)
        assert set(prof) == {name} and prof[name]["calls"] == 20, prof


def test_parameter_changes_between_chunks_keep_the_past():
    from torchfx_amd.realtime import StatefulDelay
    d = StatefulDelay(delay_samples=1000, taps=3)
    x = _signal((2, 4000), torch.float32, 8)
    d(x)
    d.taps, d.feedback, d.mix = 2, 0.7, 0.9
    d(x[:, :0])
    assert torch.equal(d._hist, x[:, -2000:])
    d.delay_samples = 1500
    y = d(torch.zeros(2, 1500, device=DEV))
    assert d._hist.shape == (2, 3000) and y[:, 1000:].abs().sum() > 0


def test_zero_delay_runs_without_history_on_device():
    from torchfx_amd import Delay
    from torchfx_amd.realtime import StatefulDelay
    kw = _kw(0, 3, True)
    x = _signal((2, 2, 3000), torch.float32, 12, 1)
    d = StatefulDelay(**kw)
    y = _chunked(d, x, [1, 7, 512], flush=False)
    assert d._hist.shape == (4, 0)
    assert torch.equal(torch.cat([y, d.flush()], dim=-1), Delay(**kw)(x))


def _schedule_run(use_graph):
    """A RealtimeProcessor on the device whose delay and reverb parameters change between blocks."""
    from torchfx_amd.realtime import RealtimeProcessor, StatefulDelay, StatefulReverb, StreamConfig
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 512 * 48)).astype(np.float32))
    be = _MemoryBackend()
    cfg = StreamConfig(sample_rate=48000, buffer_size=512, channels_in=2, channels_out=2)
    changes = {12: [("0.taps", 4), ("0.feedback", 0.6), ("1.mix", 0.7)], 24: [("0.delay_samples", 9000), ("1.delay", 2000)],
               36: [("0.bpm", 100), ("0.mix", 0.5)]}
    out = []
    with RealtimeProcessor([StatefulDelay(bpm=120), StatefulReverb(delay=4410)], be, cfg, device=DEV, use_graph=use_graph) as rp:
        for b in range(48):
            for k, v in changes.get(b, []):
                rp.set_parameter(k, v)
            out.append(be.run(x[:, b * 512:(b + 1) * 512], 512))
        effects = rp.effects
    return torch.cat(out, dim=-1), effects


def test_parameter_changes_under_graph_replay_equal_eager():
    eager, _ = _schedule_run(False)
    graph, fx = _schedule_run(True)
    assert fx[0].taps == 4 and fx[0].delay_samples == 14400 and fx[1].delay == 2000
    assert torch.equal(graph, eager)


def test_stream_processor_graph_recaptures_after_a_direct_parameter_change():
    from torchfx_amd.realtime import StreamProcessor
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 512 * 16)).astype(np.float32))

    def run(use_graph):
        chain = _chain()
        sp = StreamProcessor(chain, chunk_size=512, device=DEV, use_graph=use_graph)
        a = sp.process_tensor(x[:, :512 * 8], 48000)
        chain[1].taps, chain[1].feedback, chain[2].delay = 5, 0.8, 1000
        return torch.cat([a, sp.process_tensor(x[:, 512 * 8:], 48000)], dim=-1)

    assert torch.equal(run(True), run(False))
