"""StatefulWaveshaper / StatefulDistortion on the device (tfx_waveshaper_stream_forward, csrc/waveshaper.hip): chunk outputs plus
flush() are torch.equal to the one-shot device call for every oversampling factor, both dtypes and chunk sizes around the
latency, the history and the tile; the concatenated stream also meets the per-sample bound of tests/waveshaper_reference.py and,
for the hard clipper, has the bits of the device composition resample -> multiply -> clamp -> resample; one-sample chunks,
layouts, planted NaNs and Infs at chunk seams and in the history, batch independence, one launch per chunk, graph replay and the
real-time callback.  The tile, the latency and the history come from the plan query.

All of it at the default window (waveshaper_kernel<T, 24, true>).  The stream form of every other register bucket and of stages of
unequal length, whose dry sample sits elsewhere in the staged window, is section B of tests/test_gpu_waveshaper_edges.py."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import waveshaper_reference as R
from tests.gpu_common import DEV, ext
from torchfx_amd import resample_poly, waveshape
from torchfx_amd.realtime import RealtimeProcessor, StatefulDistortion, StatefulWaveshaper, StreamConfig, StreamProcessor
from torchfx_amd.resample import design_taps

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
WINDOW = ("kaiser", 5.0)
CURVE5 = np.array([-0.9, -0.2, 0.05, 0.4, 0.8])
KW = dict(drive_db=9.0, bias=0.15, mix=0.7)


def plan(T, L, dt):
    n = 20 * L + 1 if L > 1 else 0
    return ext().waveshaper_stream_plan_info(T, L, n, n, 0, DT[dt][0])


def signal(shape, seed, dt):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(DT[dt][1])


@functools.lru_cache(maxsize=None)
def taps(L, dt):
    return design_taps(L, 1, WINDOW, DT[dt][0]).numpy(), design_taps(1, L, WINDOW, DT[dt][0]).numpy()


def run(fx, x, sizes):
    """The chunks of `sizes`, then the rest of x in one chunk, then the tail."""
    outs, o, n = [], 0, x.shape[-1]
    for k in sizes:
        outs.append(fx(x[..., o:o + k]))
        o += k
    if o < n:
        outs.append(fx(x[..., o:]))
    return torch.cat(outs + [fx.flush()], dim=-1)


def chunk_lists(L, dt):
    """Two lists over a row of 3 * tile + 100 samples that between them hit 1, D - 1, D, D + 1, Hs, tile - 1, tile, tile + 1,
    2 * tile + 3 and a 0-length chunk in the middle."""
    q = plan(1, L, dt)
    D, Hs, N = q["latency"], q["history"], q["tile"]
    return 3 * N + 100, [[1, D - 1, D, D + 1, Hs, 0, N - 1, N + 1], [N, 0, 2 * N + 3]], D


def same_bits(a, b):
    """Equal NaN masks and equal bit patterns everywhere else."""
    ia = a.view(torch.int32 if a.dtype == torch.float32 else torch.int64)
    ib = b.view(ia.dtype)
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(ia[~na], ib[~nb]))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", [2, 4, 8])
@pytest.mark.parametrize("shape", ["hard", "tanh", "curve5"])
def test_chunks_plus_flush_equal_the_one_shot_call_and_stay_within_the_bound(shape, L, dt):
    T, lists, D = chunk_lists(L, dt)
    xh = signal((2, T), 7 * L + len(shape), dt)
    x = torch.from_numpy(xh).to(DEV)
    kw = dict(KW, oversample=L, **(dict(curve=CURVE5) if shape == "curve5" else dict(shape=shape)))
    ref = waveshape(x, **kw)
    fx = StatefulWaveshaper(**kw)
    assert fx.latency == D
    for sizes in lists:
        got = run(fx, x, sizes)
        assert got.shape == ref.shape and got.dtype == ref.dtype and got.device == ref.device
        assert torch.equal(got, ref), sizes
    # independent of the code under test: the wide reference and its per-sample bound
    hu, hd = taps(L, dt)
    q = ext().waveshaper_plan_info(T, L, hu.size, hd.size, 0, DT[dt][0])
    frac = R.check(got.cpu().numpy(), xh, L, hu, hd, q["taps_up"], q["taps_dn"], "curve" if shape == "curve5" else shape,
                   what=f"stream {shape} L={L} {dt}", curve=CURVE5 if shape == "curve5" else None, **KW)
    print(f"largest fraction of the bound, {shape} L={L} {dt}: {frac:.3f}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", [2, 4, 8])
def test_hard_stream_has_the_bits_of_the_device_composition(L, dt):
    T, lists, _ = chunk_lists(L, dt)
    x = torch.from_numpy(signal((2, T), 50 + L, dt)).to(DEV)
    drive = 10.0 ** (14.0 / 20.0)
    want = resample_poly(torch.clamp(resample_poly(x, L, 1) * drive, -1, 1), 1, L)
    for sizes in lists:
        assert torch.equal(run(StatefulWaveshaper("hard", drive_db=14.0, oversample=L), x, sizes), want), sizes


@pytest.mark.parametrize("L", [1, 4])
def test_one_sample_chunks(L):
    x = torch.from_numpy(signal((2, 200), 3, "f32")).to(DEV)
    fx = StatefulWaveshaper("cubic", oversample=L, **KW)
    assert torch.equal(run(fx, x, [1] * 200), waveshape(x, "cubic", oversample=L, **KW))
    short = x[:, :5].contiguous()                                   # a stream shorter than the latency: all of it is the tail
    assert torch.equal(run(fx, short, [1] * 5), waveshape(short, "cubic", oversample=L, **KW))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_layouts(dt):
    tdt = DT[dt][0]
    sizes = [100, 333, 1, 40]
    for shape in ((900,), (3, 900), (2, 2, 900)):
        x = torch.from_numpy(signal(shape, 11 + len(shape), dt)).to(DEV)
        ref = waveshape(x, "tanh", oversample=4, **KW)
        assert torch.equal(run(StatefulWaveshaper("tanh", oversample=4, **KW), x, sizes), ref), shape
        # every chunk in a buffer whose rows start one element past a 16-byte boundary
        fx, outs, o = StatefulWaveshaper("tanh", oversample=4, **KW), [], 0
        for k in sizes + [900 - sum(sizes)]:
            rows = int(np.prod(shape[:-1], dtype=np.int64))
            buf = torch.empty(rows * k + 4, dtype=tdt, device=DEV)
            off = next(i for i in range(1, 5) if (buf.data_ptr() + i * buf.element_size()) % 16 != 0)
            c = buf[off:off + rows * k].view(*shape[:-1], k)
            c.copy_(x[..., o:o + k])
            assert c.data_ptr() % 16 != 0 and c.is_contiguous()
            outs.append(fx(c))
            o += k
        assert torch.equal(torch.cat(outs + [fx.flush()], dim=-1), ref), shape
        # chunks that are strided views: every second sample of a signal twice as long
        wide = torch.zeros(*shape[:-1], 1800, dtype=tdt, device=DEV)
        wide[..., ::2] = x
        fx, outs, o = StatefulWaveshaper("tanh", oversample=4, **KW), [], 0
        for k in sizes + [900 - sum(sizes)]:
            c = wide[..., 2 * o:2 * (o + k):2]
            assert c.shape[-1] == k and (k == 1 or not c.is_contiguous())
            outs.append(fx(c))
            o += k
        assert torch.equal(torch.cat(outs + [fx.flush()], dim=-1), ref), shape


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_non_finite_input(bad, dt):
    """The sample as the last of a chunk, as the first of the next one, and in chunks so short that it sits in the history for
    more than two of them: the stream's NaNs are the one-shot call's, exactly the outputs within reach_after behind and
    reach_before ahead of the sample; every other sample has the clean bits; the other rows are untouched."""
    q = ext().waveshaper_plan_info(1, 4, 81, 81, 0, DT[dt][0])
    rb, ra = q["reach_before"], q["reach_after"]
    n = 640
    base = signal((3, n), 21, dt)
    for cs, p in ((100, 299), (100, 300), (16, 16 * 9 + 5), (16, 16 * 9 - 1), (16, 16 * 9)):
        xh = base.copy()
        xh[1, p] = bad
        x = torch.from_numpy(xh).to(DEV)
        ref = waveshape(x, "tanh", oversample=4, **KW)
        clean = waveshape(torch.from_numpy(base).to(DEV), "tanh", oversample=4, **KW)
        got = run(StatefulWaveshaper("tanh", oversample=4, **KW), x, [cs] * (n // cs))
        want = torch.zeros(3, n, dtype=torch.bool)
        want[1, p - rb:p + ra + 1] = True
        assert torch.equal(torch.isnan(got).cpu(), want), (cs, p)
        assert same_bits(got, ref), (cs, p)
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]), (cs, p)
    # a sample whose reach crosses the stream's start, and its end
    for p in (3, n - 2):
        xh = base.copy()
        xh[1, p] = bad
        x = torch.from_numpy(xh).to(DEV)
        got = run(StatefulWaveshaper("tanh", oversample=4, **KW), x, [50] * 12)
        assert same_bits(got, waveshape(x, "tanh", oversample=4, **KW)), p
        assert int(torch.isnan(got).sum()) == min(n, p + ra + 1) - max(0, p - rb)


def test_batch_independence():
    x = torch.from_numpy(signal((5, 2500), 31, "f32")).to(DEV)
    got = run(StatefulDistortion(), x, [700, 1, 1100])
    for k in range(5):
        assert torch.equal(run(StatefulDistortion(), x[k].clone(), [64, 900, 3]), got[k]), k


def test_one_launch_per_chunk():
    from torchfx_amd import _lib
    lib = _lib.load()
    for L, dt, tail in ((1, "f32", 0), (4, "f32", 1), (2, "f64", 1)):
        fx = StatefulWaveshaper("tanh", oversample=L, **KW)
        x = torch.from_numpy(signal((2, 512 * 20), 41, dt)).to(DEV)
        blocks = [x[:, 512 * i:512 * (i + 1)].contiguous() for i in range(20)]
        fx(blocks[0])                                        # the tap tables exist before the count starts
        fx.reset_state()
        lib.tfx_prof_enable(1)
        lib.tfx_prof_collect()
        for b in blocks:
            fx(b)
        fx.flush()
        torch.cuda.synchronize()
        prof = json.loads(lib.tfx_prof_collect().decode())
        lib.tfx_prof_enable(0)
        assert set(prof) == {"waveshaper_stream_kernel"} and prof["waveshaper_stream_kernel"]["calls"] == 20 + tail, prof


def test_stream_processor_graph_equals_eager():
    B, n = 64, 64 * 12 + 20
    x = torch.from_numpy(signal((2, n), 51, "f32"))
    ref = waveshape(x.to(DEV), "tanh", drive_db=12.0)
    got = {}
    for use_graph in (False, True):
        fx = StatefulDistortion()
        proc = StreamProcessor([fx], chunk_size=B, device=DEV, use_graph=use_graph)
        replays = []
        step = proc._graph_step
        proc._graph_step = lambda w, step=step, fx=fx: (replays.append(fx._pos), step(w))[1]
        got[use_graph] = proc.process_tensor(x, 48000)
        sat = fx.latency + fx.history_length
        if use_graph:                                        # eager until the position counter has saturated, replays from then on
            assert proc._graph is not None and len(replays) == 12 - -(-sat // B) and all(p == sat for p in replays)
        else:
            assert not replays
    assert got[True].shape == ref.shape and torch.equal(got[True], got[False])
    assert torch.equal(got[False], ref)


@pytest.mark.parametrize("use_graph", [False, True])
def test_realtime_processor_constant_latency(use_graph):
    class Backend:
        def open_stream(self, config, callback=None):
            self.config, self.callback = config, callback

        def start(self): pass

        def stop(self): pass

        def close(self): pass

        def fire(self, block):
            out = torch.zeros(self.config.channels_out, block.shape[-1])
            self.callback(block, out, block.shape[-1])
            return out

    B = 512
    x = torch.from_numpy(signal((2, B * 6), 61, "f32"))
    ref = waveshape(x.to(DEV), "tanh", drive_db=12.0).cpu()
    be, fx = Backend(), StatefulDistortion(aligned=False)
    cfg = StreamConfig(sample_rate=48000, buffer_size=B, channels_in=2, channels_out=2)
    with RealtimeProcessor([fx], be, cfg, device=DEV, use_graph=use_graph) as p:
        D = p.chain_latency_samples
        assert D == fx.latency == 21
        y = torch.cat([be.fire(x[:, i:i + B]) for i in range(0, x.shape[-1], B)], dim=-1)
        assert (p._runner._graph is not None) == use_graph
    assert torch.equal(y[:, :D], torch.zeros(2, D)) and torch.equal(y[:, D:], ref[:, :-D])
