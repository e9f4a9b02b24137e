"""StatefulLimiter on the device (csrc/limiter.hip, the stream form of limiter_kernel): all chunk outputs plus flush() are
torch.equal to limit() on the whole signal on the same device and dtype -- for the sample detector and the 2x / 4x detectors,
a halo longer than a tile, chunk sizes around the tile, one-sample chunks, misaligned rows and strided chunks; the gain curve;
one launch per chunk; what a NaN / Inf poisons and when the stream is clean again; batch independence; StreamProcessor (eager,
HIP graph, files) and RealtimeProcessor.  Every length comes from the plan info (tile = 8193 - 2A - H)."""
import json
import sys

import numpy as np
import pytest
import torch

from tests.gpu_common import DEV
from tests.test_stream_limiter_host import FS, kwargs, random_sizes, run, stateful

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
GEOMS = [(1, 1), (72, 480), (512, 4096)]                     # the last: A + H - 1 behind a tile is longer than the tile (3073)


def det(up):
    return dict(detector="sample") if up == 1 else dict(detector="true_peak", oversample=up)


def plan(n, A, H, up, dtype=torch.float32):
    from torchfx_amd import torchfx_ext
    return torchfx_ext.limiter_stream_plan_info(n, A, H, up, 0 if up == 1 else 20 * up + 1, dtype)


def signal(shape, dtype, seed, A, H, tile, offset=0):
    """Noise under the ceiling; peaks far over it in the first eighth and, where the gain recovers soon enough to leave the
    end transparent, around the first tile boundary too.  offset 1: rows that start off any 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    x = ((torch.rand(n + offset, generator=g, dtype=torch.float64) * 2 - 1) * 0.3)[offset:].view(*shape).clone()
    T = shape[-1]
    x[..., :T // 8:37] *= 8.0
    if tile + 60 + A + H + 200 < T:
        x[..., tile - 40:tile + 40:7] *= 8.0
    base = torch.zeros(n + offset, dtype=dtype, device=DEV)
    base[offset:] = x.reshape(-1).to(dtype)
    return base[offset:].view(*shape)


def one_shot(x, A, H, up, **kw):
    from torchfx_amd.limiter import limit
    return limit(x, FS, **kwargs(A, H, **det(up)), **kw)


@pytest.mark.parametrize("A,H", GEOMS)
@pytest.mark.parametrize("up", [1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_chunks_plus_flush_equal_the_one_shot_result(dtype, up, A, H):
    info = plan(512, A, H, up, dtype)
    tile, D = info["tile"], info["latency"]
    assert tile == 8193 - 2 * A - H
    n = 2 * tile + 3
    x = signal((2, n), dtype, 1, A, H, tile)
    ref, g = one_shot(x, A, H, up, return_gain=True)
    assert float(g.min()) < 0.9 and bool((g[:, -64:] == 1).all()) and torch.equal(ref[:, -64:], x[:, -64:])
    lim = stateful(A, H, **det(up))
    assert lim.latency == D and lim.history_length == info["history"]
    assert lim.route(x, 512).startswith("native (limiter_stream_kernel")
    for name, sizes in {"rt512": [512] * (n // 512 + 1), "random": random_sizes(n, 2, 9000),
                        "around_the_tile": [tile - 1, tile, tile + 1]}.items():
        outs, tail = run(lim, x, sizes)
        got = torch.cat(outs + [tail], dim=-1)
        assert got.shape == ref.shape and torch.equal(got, ref), name


@pytest.mark.parametrize("up", [1, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_one_sample_chunks(dtype, up):
    x = signal((2, 300), dtype, 3, 5, 7, 10 ** 6)
    ref = one_shot(x, 5, 7, up)
    assert not torch.equal(ref, x)
    lim = stateful(5, 7, **det(up))
    D = lim.latency
    outs, tail = run(lim, x, [1] * 300)
    assert [o.shape[-1] for o in outs] == [0] * D + [1] * (300 - D)
    assert torch.equal(torch.cat(outs + [tail], dim=-1), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_misaligned_rows_strided_chunks_and_shapes(dtype):
    A, H, up = 72, 480, 4
    tile = plan(512, A, H, up)["tile"]
    n = tile + 700
    x = signal((2, 2, n), dtype, 4, A, H, tile, offset=1)
    assert x.data_ptr() % 16 != 0
    ref = one_shot(x, A, H, up)
    outs, tail = run(stateful(A, H, **det(up)), x, random_sizes(n, 5, 3000))
    assert torch.equal(torch.cat(outs + [tail], dim=-1), ref)
    wide = torch.zeros(2, 2, 2 * n, dtype=dtype, device=DEV)
    wide[..., ::2] = x
    view = wide[..., ::2]                                     # every chunk is a strided view
    assert not view.is_contiguous()
    outs, tail = run(stateful(A, H, **det(up)), view, [512] * (n // 512 + 1))
    assert torch.equal(torch.cat(outs + [tail], dim=-1), ref)
    # unlinked rows, a [T] signal, and the constant-latency mode
    ref1 = one_shot(x[0, 0], A, H, up)
    outs, tail = run(stateful(A, H, **det(up)), x[0, 0], [1000] * (n // 1000 + 1))
    assert torch.equal(torch.cat(outs + [tail], dim=-1), ref1)
    refu = one_shot(x, A, H, up, link=False)
    assert not torch.equal(refu, ref)
    lim = stateful(A, H, link=False, aligned=False, **det(up))
    outs, tail = run(lim, x, [512] * (n // 512 + 1))
    assert all(o.shape[-1] == 512 for o in outs[:-1]) and tail.shape[-1] == lim.latency
    assert torch.equal(torch.cat(outs + [tail], dim=-1),
                       torch.cat([torch.zeros(2, 2, lim.latency, dtype=dtype, device=DEV), refu], dim=-1))


@pytest.mark.parametrize("up", [1, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_gain_curve_at_the_ext_level(dtype, up):
    from torchfx_amd import torchfx_ext
    from torchfx_amd.limiter import LimiterParams
    A, H = 72, 480
    info = plan(512, A, H, up, dtype)
    D, n = info["latency"], info["tile"] + 300
    x = signal((3, 2, n), dtype, 6, A, H, info["tile"])
    ref, g = one_shot(x, A, H, up, return_gain=True)
    P = LimiterParams(FS, dtype, **kwargs(A, H, **det(up)))
    w = torch.from_numpy(P.w)
    ys, gs, hist, N = [], [], None, 0
    for k in random_sizes(n, 7, 4000):
        c = x[..., N:N + k]
        y, gg, hist = torchfx_ext.limiter_stream_forward(c, hist, N, P.c, A, H, w, P.up, P.taps, 2, True)
        assert gg.shape == (3, c.shape[-1]) and hist.shape == (6, info["history"])
        ys.append(y)
        gs.append(gg)
        N += c.shape[-1]
    y, gg, _ = torchfx_ext.limiter_stream_forward(torch.zeros(3, 2, D, dtype=dtype, device=DEV), hist, N, P.c, A, H, w, P.up, P.taps,
                                                  2, True, n_in=0)
    got_y, got_g = torch.cat(ys + [y], dim=-1), torch.cat(gs + [gg], dim=-1)
    assert torch.equal(got_y[..., :D], torch.zeros_like(got_y[..., :D])) and torch.equal(got_g[:, :D], torch.ones_like(got_g[:, :D]))
    assert torch.equal(got_y[..., D:], ref) and torch.equal(got_g[:, D:], g)
    assert torchfx_ext.limiter_stream_forward(x[..., :100], None, 0, P.c, A, H, w, P.up, P.taps, 2)[1] is None


def test_one_launch_per_chunk():
    from torchfx_amd import _lib
    lib = _lib.load()
    for up, dtype in ((1, torch.float32), (4, torch.float32), (2, torch.float64)):
        lim = stateful(72, 480, **det(up))
        x = signal((2, 512 * 20), dtype, 8, 72, 480, 10 ** 6)
        blocks = [x[:, 512 * i:512 * (i + 1)].contiguous() for i in range(20)]
        lim(blocks[0])                                       # the tap table and the padded window exist before the count starts
        lim.reset_state()
        lib.tfx_prof_enable(1)
        lib.tfx_prof_collect()
        for b in blocks:
            lim(b)
        lim.flush()
        torch.cuda.synchronize()
        prof = json.loads(lib.tfx_prof_collect().decode())
        lib.tfx_prof_enable(0)
        assert set(prof) == {"limiter_stream_kernel"} and prof["limiter_stream_kernel"]["calls"] == 21, prof


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("up", [1, 4])
def test_non_finite_input(bad, up):
    A, H, B = 72, 480, 512
    info = plan(B, A, H, up)
    D, Hs = info["latency"], info["history"]
    n, p0 = B * 8, B + 100
    x = signal((2, 2, n), torch.float32, 9, A, H, 10 ** 6)
    x[..., n // 2::41] *= 8.0                                # the clean stream is limited after the sample too
    clean = one_shot(x, A, H, up)
    xb = x.clone()
    xb[0, 1, p0] = bad
    outs, tail = run(stateful(A, H, **det(up)), xb, [B] * 8)
    got = torch.cat(outs + [tail], dim=-1)
    assert torch.equal(got[1], clean[1])                     # the other group never sees it
    # every output whose dependence window [n - (Hs - D), n + D] holds the sample: NaN in both channels of the group
    assert bool(torch.isnan(got[0, :, p0 - D:p0 + Hs - D + 1]).all())
    # nothing else than the outputs of the chunks whose [history | chunk] holds the sample: chunks 1 .. k, k the last with
    # k * B - Hs <= p0; a chunk that starts at N writes positions [N - D, N + B - D)
    k = (p0 + Hs) // B
    lo, hi = B - D, (k + 1) * B - D
    nan = torch.isnan(got[0])
    assert not bool(nan[:, :lo].any()) and not bool(nan[:, hi:].any())
    assert torch.equal(got[0, :, :lo], clean[0, :, :lo])
    # ... and Hs + one chunk after the sample the stream is the clean stream's again, bit for bit
    assert hi <= p0 + Hs + B and torch.equal(got[0, :, p0 + Hs + B:], clean[0, :, p0 + Hs + B:])
    assert not torch.equal(clean[0, :, p0 + Hs + B:], x[0, :, p0 + Hs + B:])


def test_batch_independence():
    A, H, up = 72, 480, 4
    n = 3000
    x = signal((3, 2, n), torch.float32, 10, A, H, 10 ** 6)
    x[1] *= 0.5
    outs, tail = run(stateful(A, H, **det(up)), x, random_sizes(n, 11, 700))
    got = torch.cat(outs + [tail], dim=-1)
    for b in range(3):
        outs, tail = run(stateful(A, H, **det(up)), x[b], random_sizes(n, 12 + b, 900))
        assert torch.equal(torch.cat(outs + [tail], dim=-1), got[b])


def _hp():
    from torchfx_amd.filter import HiButterworth
    return HiButterworth(200, order=2)


def test_stream_processor_graph_equals_eager():
    from torchfx_amd.realtime import StatefulLimiter, StreamProcessor
    B, n = 512, 512 * 12 + 100
    x = signal((2, n), torch.float32, 13, 72, 480, 10 ** 6)
    x[:, n // 2::41] *= 8.0
    # the limiter's reference is the one-shot call on what the chain hands it: the chunked filter's output
    ref = one_shot(StreamProcessor([_hp()], chunk_size=B, device=DEV).process_tensor(x.cpu(), FS), 72, 480, 4)
    got = {}
    for use_graph in (False, True):
        lim = StatefulLimiter()                              # the defaults at 48 kHz: 72 / 480, 4x
        proc = StreamProcessor([_hp(), lim], chunk_size=B, device=DEV, use_graph=use_graph)
        replays = []
        step = proc._graph_step
        proc._graph_step = lambda w, step=step, lim=lim: (replays.append(lim._pos), step(w))[1]
        got[use_graph] = proc.process_tensor(x.cpu(), FS)
        sat = lim.latency + lim.history_length
        if use_graph:                                        # eager until the position counter has saturated, replays from then on
            assert proc._graph is not None and len(replays) == 12 - -(-sat // B) and all(p == sat for p in replays)
        else:
            assert not replays
    assert got[True].shape == ref.shape and torch.equal(got[True], got[False])
    assert torch.equal(got[False], ref)


def test_stream_processor_process_file(tmp_path, monkeypatch):
    from tests import _fake_soundfile as sf
    from torchfx_amd.realtime import StatefulLimiter, StreamProcessor
    monkeypatch.setitem(sys.modules, "soundfile", sf)
    frames = signal((2, 20_000), torch.float32, 14, 72, 480, 10 ** 6).cpu().numpy().T.copy()
    src = tmp_path / "in.wav"
    sf.make(src, frames, FS, subtype="FLOAT")
    ref = one_shot(torch.from_numpy(frames.T.copy()).to(DEV), 72, 480, 4).cpu().numpy()
    for use_graph in (False, True):
        StreamProcessor([StatefulLimiter()], chunk_size=4096, device=DEV, use_graph=use_graph).process_file(src, tmp_path / "o.wav")
        rec = sf.written[-1]
        assert rec["fs"] == FS and rec["data"].shape == frames.shape and np.array_equal(rec["data"].T, ref), use_graph


@pytest.mark.parametrize("use_graph", [False, True])
def test_realtime_processor_constant_latency(use_graph):
    from torchfx_amd.realtime import RealtimeProcessor, StatefulLimiter, StreamConfig

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
    x = signal((2, B * 10), torch.float32, 15, 72, 480, 10 ** 6)
    x[:, B * 5::41] *= 8.0
    ref = one_shot(x, 72, 480, 4).cpu()
    be, lim = Backend(), StatefulLimiter(aligned=False)
    cfg = StreamConfig(sample_rate=FS, buffer_size=B, channels_in=2, channels_out=2)
    xc = x.cpu()
    with RealtimeProcessor([lim], be, cfg, device=DEV, use_graph=use_graph) as p:
        D = p.chain_latency_samples
        assert D == 81
        y = torch.cat([be.fire(xc[:, i:i + B]) for i in range(0, xc.shape[-1], B)], dim=-1)
        assert (p._runner._graph is not None) == use_graph
    assert torch.equal(y[:, :D], torch.zeros(2, D)) and torch.equal(y[:, D:], ref[:, :-D])
