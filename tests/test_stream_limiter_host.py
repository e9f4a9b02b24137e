"""StatefulLimiter on the host: chunk outputs plus flush() are torch.equal to limit() on the whole signal for both dtypes, both
detectors, every input shape and chunking; the emission rule, the constant-latency mode, the two stream edges (the
interpolator rings in front of position 0 and past the end), restarts, StreamProcessor / RealtimeProcessor / Wave, and what the
C entry points refuse before they touch a device."""
import ctypes
import random
import sys

import numpy as np
import pytest
import torch

FS = 48000
DTYPES = [torch.float32, torch.float64]
GEOMS = [(1, 1), (5, 7), (72, 480)]


def signal(shape, dtype, seed):
    """Noise below the ceiling, in its first two fifths with peaks far over it: limited and transparent stretches both."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * 0.3
    T = shape[-1]
    x[..., :T * 2 // 5:53] *= 8.0
    return x.to(dtype)


def kwargs(A, H, detector="true_peak", **kw):
    return dict(lookahead=A / FS, hold=H / FS, detector=detector, **kw)


def stateful(A, H, detector="true_peak", **kw):
    from torchfx_amd.realtime import StatefulLimiter
    return StatefulLimiter(fs=FS, **kwargs(A, H, detector, **kw))


def one_shot(x, A, H, detector="true_peak", **kw):
    from torchfx_amd.limiter import limit
    return limit(x, FS, **kwargs(A, H, detector, **kw))


def run(lim, x, sizes):
    outs, o, n, sizes = [], 0, x.shape[-1], list(sizes)
    while o < n or sizes:
        k = sizes.pop(0) if sizes else n - o
        outs.append(lim(x[..., o:o + k]))
        o += k
    return outs, lim.flush()


def random_sizes(n, seed, hi):
    rng = random.Random(seed)
    out = []
    while sum(out) < n:
        out.append(rng.randint(1, hi))
    return out


def chunkings(n, D):
    small = max(1, D // 2)
    return {"one": [n], "ones": [1] * n, "random": random_sizes(n, 3, 200), "below_latency": [small] * (n // small + 1),
            "zero_in_the_middle": [n // 3, 0, n // 4, 0]}


@pytest.mark.parametrize("detector", ["true_peak", "sample"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("A,H", GEOMS)
def test_chunks_plus_flush_equal_the_one_shot_result(A, H, dtype, detector):
    from torchfx_amd.limiter import limit
    n = 1300 if A > 5 else 300
    x = signal((2, n), dtype, 1)
    ref, g = limit(x, FS, return_gain=True, **kwargs(A, H, detector))
    assert float(g.min()) < 0.9 and bool((g[:, -20:] == 1).all()) and torch.equal(ref[:, -20:], x[:, -20:])
    lim = stateful(A, H, detector)
    D = lim.latency
    for name, sizes in chunkings(n, D).items():
        outs, tail = run(lim, x, sizes)
        # the emission rule: after N inputs the stream has returned max(0, N - D) samples
        N = 0
        for k, o in zip(sizes + [n - sum(sizes)] * (sum(sizes) < n), outs):
            k = min(k, n - N)
            assert o.shape[-1] == max(0, N + k - D) - max(0, N - D), (name, N, k)
            N += k
        assert tail.shape[-1] == min(n, D)
        got = torch.cat(outs + [tail], dim=-1)
        assert got.dtype == dtype and torch.equal(got, ref), name


@pytest.mark.parametrize("link", [True, False])
@pytest.mark.parametrize("shape", [(400,), (2, 400), (2, 2, 400)])
def test_shapes_and_link(shape, link):
    x = signal(shape, torch.float32, 2)
    if len(shape) > 1:
        x[..., 1, :] *= 0.5                                   # the channels differ: linked and unlinked gains differ
    ref = one_shot(x, 5, 7, link=link)
    lim = stateful(5, 7, link=link)
    outs, tail = run(lim, x, random_sizes(400, 5, 60))
    assert torch.equal(torch.cat(outs + [tail], dim=-1), ref)
    if len(shape) > 1:
        assert not torch.equal(ref, one_shot(x, 5, 7, link=not link))


@pytest.mark.parametrize("detector", ["true_peak", "sample"])
def test_constant_latency_mode(detector):
    x = signal((2, 500), torch.float64, 3)
    ref = one_shot(x, 5, 7, detector)
    lim = stateful(5, 7, detector, aligned=False)
    D = lim.latency
    outs, tail = run(lim, x, random_sizes(500, 7, 40))
    assert all(o.shape[-1] > 0 for o in outs) and sum(o.shape[-1] for o in outs) == 500
    assert tail.shape[-1] == D
    assert torch.equal(torch.cat(outs + [tail], dim=-1), torch.cat([torch.zeros(2, D, dtype=x.dtype), ref], dim=-1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_interpolator_ringing_in_front_of_the_stream_does_not_reduce_the_gain(dtype):
    """x[0] far over the ceiling: the interpolated signal rings into negative time, where the one-shot call has r = 1 and
    q[-1] = 0.  Zeros for history without that mask would start the gain reduction at the wrong level."""
    x = torch.zeros(1, 300, dtype=dtype)
    x[0, 0] = 8.0
    x[0, 1:] = 0.2
    ref = one_shot(x, 5, 7)
    for sizes in ([1] * 300, [3] * 100, [300]):
        outs, tail = run(stateful(5, 7), x, sizes)
        assert torch.equal(torch.cat(outs + [tail], dim=-1), ref), sizes[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_interpolator_ringing_past_the_end_does_not_reduce_the_gain(dtype):
    x = torch.full((1, 300), 0.2, dtype=dtype)
    x[0, -1] = 8.0
    ref = one_shot(x, 5, 7)
    for sizes in ([1] * 300, [7] * 43, [300]):
        outs, tail = run(stateful(5, 7), x, sizes)
        assert torch.equal(torch.cat(outs + [tail], dim=-1), ref), sizes[0]


def test_latency_and_history_are_the_geometry():
    from torchfx_amd import torchfx_ext
    from torchfx_amd.limiter import LimiterParams
    for A, H in GEOMS + [(512, 4096)]:
        s = stateful(A, H, "sample")
        assert (s.latency, s.history_length) == (A - 1, 2 * A + H - 3)
        t = stateful(A, H)                                   # the default 4x filter: 81 taps, n_pre_remove 41
        P = LimiterParams(FS, torch.float32, **kwargs(A, H))
        assert (P.up, P.taps.numel()) == (4, 81)
        assert t.latency == A - 1 + 10
        one = torchfx_ext.limiter_plan_info(1000, A, H, 4, 81)
        assert t.latency == one["halo_right"] - 1
        # behind: A + H - 2 of the minimum and the smoothing, then the interpolator's taps per phase behind position i - 1
        assert t.history_length == t.latency + A + H - 2 + (one["Lp"] - 10) <= t.latency + one["halo_left"]
        info = torchfx_ext.limiter_stream_plan_info(512, A, H, 4, 81, torch.float64, groups=3, channels=2)
        assert (info["latency"], info["history"], info["tile"]) == (t.latency, t.history_length, 8193 - 2 * A - H)
        assert info["positions"] == min(512, info["tile"]) + 2 * A + H - 2 and info["tiles"] == -(-512 // info["tile"])
        assert info["lds_bytes"] == one["lds_bytes"] * 2
    # a filter whose n_pre_remove leaves two phases to the sample before: one more sample of forward reach
    even = torchfx_ext.limiter_stream_plan_info(512, 5, 7, 4, 83)    # half_len 41, n_pre_remove 42 = 10 * 4 + 2
    assert even["latency"] == 5 - 1 + 10 + 1


def test_custom_taps_with_two_phases_of_the_previous_sample():
    """83 taps at 4x: n_pre_remove mod up = 2, so a position's peak reads one input more ahead than n_pre_remove // up."""
    from torchfx_amd.resample import design_taps
    taps = torch.cat([torch.tensor([0.01]), design_taps(4, 1, ("kaiser", 5.0), torch.float64), torch.tensor([0.01])])
    x = signal((2, 300), torch.float64, 8)
    ref = one_shot(x, 5, 7, oversample=4, taps=taps)
    lim = stateful(5, 7, oversample=4, taps=taps)
    assert lim.latency == 5 - 1 + 10 + 1
    for sizes in ([1] * 300, random_sizes(300, 9, 30)):
        outs, tail = run(lim, x, sizes)
        assert torch.equal(torch.cat(outs + [tail], dim=-1), ref)


def test_restarts_and_live_parameters():
    x = signal((2, 600), torch.float64, 4)
    lim = stateful(5, 7)
    D = lim.latency
    lim(x[:, :300])
    # another row count, dtype or grouping: a new stream from silence, what was held back is dropped
    for other in (x[:1, 300:], x[:, 300:].float()):
        got = lim(other)
        fresh = stateful(5, 7)
        assert torch.equal(got, fresh(other)) and got.shape[-1] == 300 - D
        lim(x[:, :300])
    lim.link = False
    assert torch.equal(lim(x[:, 300:]), stateful(5, 7, link=False)(x[:, 300:]))
    lim.link = True
    # whatever changes D or Hs restarts too
    for name, value in (("lookahead", 9 / FS), ("hold", 11 / FS), ("detector", "sample"), ("oversample", 2), ("fs", 44100)):
        lim = stateful(5, 7)
        lim(x[:, :300])
        setattr(lim, name, value)
        fresh = stateful(5, 7)
        setattr(fresh, name, value)
        assert torch.equal(lim(x[:, 300:]), fresh(x[:, 300:])), name
        assert torch.equal(lim.flush(), fresh.flush())
    lim = stateful(5, 7)
    lim(x[:, :300])
    lim.hold = 20 / FS
    assert lim.flush().shape[-1] == 0                        # the stream the tail belonged to is gone
    # the ceiling and a window of the same length apply from the next chunk on, the stream goes on
    lim, ref = stateful(5, 7), stateful(5, 7)
    a = lim(x[:, :300])
    assert torch.equal(a, ref(x[:, :300]))
    lim.ceiling_db = -12.0
    b = lim(x[:, 300:])
    assert b.shape[-1] == 300 and not torch.equal(b, ref(x[:, 300:]))
    assert float(b[:, 40:].abs().max()) <= 10 ** (-12 / 20) * (1 + 1e-12)
    lim.window = torch.ones(5)
    assert lim(x[:, :100]).shape[-1] == 100 and lim.flush().shape[-1] == D
    # reset_state by hand
    lim.reset_state()
    assert torch.equal(lim(x[:, :200]), stateful(5, 7, ceiling_db=-12.0, window=torch.ones(5))(x[:, :200]))


def test_empty_stream_and_zero_length_chunks():
    lim = stateful(5, 7)
    assert lim.flush().numel() == 0                          # as StatefulResample.flush without a chunk
    assert lim(torch.zeros(2, 0)).shape == (2, 0)
    assert lim.flush().shape == (2, 0)
    x = signal((2, 3), torch.float32, 5)                     # a stream shorter than the latency
    lim = stateful(5, 7)
    assert lim(x).shape == (2, 0)
    assert torch.equal(lim.flush(), one_shot(x, 5, 7))


def test_bad_dtype():
    with pytest.raises(TypeError, match="float32 or float64"):
        stateful(5, 7)(torch.zeros(2, 10, dtype=torch.float16))


def _hp():
    from torchfx_amd.filter import HiButterworth
    return HiButterworth(200, order=2, fs=FS)


def test_stream_processor_on_the_cpu_equals_the_one_piece_composition(oracle_backend):
    from torchfx_amd.realtime import StatefulLimiter, StatefulResample, StreamProcessor
    from torchfx_amd.resample import resample_poly
    x = signal((2, 5000), torch.float32, 6)
    ref = one_shot(_hp()(x), 72, 480)
    for chunk in (64, 1000, 5000):
        proc = StreamProcessor([_hp(), StatefulLimiter(**kwargs(72, 480))], chunk_size=chunk, device="cpu")
        got = proc.process_tensor(x, FS)
        assert got.shape == ref.shape and torch.equal(got, ref), chunk
    # a resampler in front: its tail goes through the limiter before the limiter hands out its own; and behind
    up = resample_poly(x, 2, 1)
    ref2 = one_shot(up, 144, 960, oversample=2)
    proc = StreamProcessor([StatefulResample(2 * FS), StatefulLimiter(lookahead=1.5e-3, hold=10e-3, oversample=2)], chunk_size=700,
                           device="cpu")
    got = proc.process_tensor(x, FS)
    assert proc.output_rate(FS) == 2 * FS and got.shape == ref2.shape and torch.equal(got, ref2)
    ref3 = resample_poly(one_shot(x, 72, 480), 2, 1)
    proc = StreamProcessor([StatefulLimiter(**kwargs(72, 480)), StatefulResample(2 * FS)], chunk_size=700, device="cpu")
    got = proc.process_tensor(x, FS)
    assert got.shape == ref3.shape and torch.equal(got, ref3)


def test_process_file_writes_every_frame(tmp_path, monkeypatch):
    from tests import _fake_soundfile as sf
    from torchfx_amd.realtime import StatefulLimiter, StreamProcessor
    monkeypatch.setitem(sys.modules, "soundfile", sf)
    frames = signal((2, 3000), torch.float32, 7).numpy().T.copy()
    src = tmp_path / "in.wav"
    sf.make(src, frames, FS, subtype="FLOAT")
    StreamProcessor([StatefulLimiter(**kwargs(5, 7))], chunk_size=512, device="cpu").process_file(src, tmp_path / "out.wav")
    rec = sf.written[-1]
    assert rec["data"].shape == frames.shape
    assert np.array_equal(rec["data"].T, one_shot(torch.from_numpy(frames.T.copy()), 5, 7).numpy())


def test_processor_and_wave_refusals():
    from torch import nn

    from torchfx_amd import Wave
    from torchfx_amd.effect import FX, Gain, Limiter
    from torchfx_amd.realtime import AudioBackend, RealtimeProcessor, StatefulLimiter, StreamConfig, StreamProcessor

    class Wrap(FX):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x)

    class Null(AudioBackend):
        def open_stream(self, config, callback=None): ...
        def start(self): ...
        def stop(self): ...
        def close(self): ...

    with pytest.raises(ValueError, match="StatefulLimiter needs overlap = 0"):
        StreamProcessor([StatefulLimiter()], chunk_size=1000, overlap=10, device="cpu")
    with pytest.raises(TypeError, match=r"looks A - 1 samples ahead.*streaming limiter.*not provided.*StatefulLimiter"):
        StreamProcessor([Gain(0.5), Limiter()], device="cpu")
    with pytest.raises(TypeError, match="top-level effect"):
        StreamProcessor([Gain(0.5), Wrap(StatefulLimiter())], device="cpu")
    with pytest.raises(TypeError, match="aligned=False"):
        RealtimeProcessor([StatefulLimiter()], Null(), StreamConfig(), device="cpu")
    with pytest.raises(TypeError, match="StatefulLimiter"):
        RealtimeProcessor([Limiter()], Null(), StreamConfig(), device="cpu")
    with pytest.raises(TypeError, match="StatefulLimiter is for chunked streams"):
        Wave(torch.zeros(2, 100), FS, device="cpu") | StatefulLimiter()
    with pytest.raises(TypeError, match="StatefulLimiter is for chunked streams"):
        Wave(torch.zeros(2, 100), FS, device="cpu") | nn.Sequential(Gain(0.5), StatefulLimiter())


def test_realtime_processor_runs_the_constant_latency_mode(oracle_backend):
    from tests.test_host_logic import _MockBackend
    from torchfx_amd.realtime import RealtimeProcessor, StatefulLimiter, StreamConfig
    x = signal((2, 512 * 6), torch.float32, 9)
    be = _MockBackend()
    cfg = StreamConfig(sample_rate=FS, buffer_size=512, channels_in=2, channels_out=2)
    lim = StatefulLimiter(aligned=False, **kwargs(72, 480))
    with RealtimeProcessor([_hp(), lim], be, cfg, device="cpu") as p:
        D = p.chain_latency_samples
        assert D == lim.latency == 72 - 1 + 10 and abs(p.latency_ms - cfg.latency_ms) < 1e-12
        outs = [be.simulate_callback(x[:, i:i + 512]) for i in range(0, x.shape[-1], 512)]
    assert all(o.shape == (2, 512) for o in outs)
    ref = one_shot(_hp()(x), 72, 480)
    got = torch.cat(outs, dim=-1)
    assert torch.equal(got[:, :D], torch.zeros(2, D)) and torch.equal(got[:, D:], ref[:, :x.shape[-1] - D])


def test_meta_free_entry_points_and_names():
    from torchfx_amd import native, torchfx_ext
    from torchfx_amd.effect import Limiter
    from torchfx_amd.realtime import StatefulLimiter
    native.load()
    assert issubclass(StatefulLimiter, Limiter)
    assert "limiter_stream_forward" in torchfx_ext.__all__ and "limiter_stream_plan_info" in torchfx_ext.__all__
    assert StatefulLimiter(fs=FS).route(torch.zeros(2, 10)).startswith("numpy on host")
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.torchfx_hip.limiter_stream_forward(torch.zeros(2, 100), None, 0, 0.9, 1, 1, torch.ones(1), 1, None, 1, False, -1)


def test_capi_checks_arguments_before_the_device():
    from torchfx_amd import _lib
    lib = _lib.load()
    w = (ctypes.c_float * 5)(*([0.2] * 5))
    wneg = (ctypes.c_float * 5)(0.2, -0.1, 0.2, 0.2, 0.5)
    h = (ctypes.c_float * 81)()
    x, y, g, hin, hout = [ctypes.c_void_p(16 + (1 << 20) * i) for i in range(5)]

    def call(*a):
        rc = lib.tfx_limiter_stream_forward(*a, None)
        return rc, lib.tfx_last_error().decode()

    #        x  y  gain dtype groups channels T  n_in consumed c  A  H  window up taps nh hist_in hist_out
    good = (x, y, g, 0, 1, 2, 100, 100, 0, 0.9, 5, 7, w, 4, h, 81, hin, hout)
    bad = {
        "bad dtype": {3: 7}, "up must be": {13: 3}, "look-ahead of 513": {10: 513}, "hold of 0": {11: 0},
        "channels must be": {5: 0}, "negative size": {6: -1}, "n_in = 101": {7: 101}, "n_in = -1": {7: -1},
        "negative stream position": {8: -1}, "ceiling must be": {9: 0.0}, "no window": {12: None}, "no taps": {14: None},
        "is negative or not finite": {12: wneg}, "null pointer": {1: None},
        "the new history needs its own buffer": {17: hin},
        "y and hist_out may not overlap x, hist_in or each other": {1: x},
    }
    for msg, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        rc, err = call(*args)
        assert rc != 0 and err.startswith("limiter_stream_forward: ") and msg in err, (msg, rc, err)
    for k, v in ((17, x), (2, x), (2, y), (2, hin), (2, hout), (1, hin), (1, hout)):       # every other overlap
        args = list(good)
        args[k] = v
        rc, err = call(*args)
        assert rc != 0 and "may not overlap" in err, (k, err)
    o = [ctypes.c_int64() for _ in range(6)]
    refs = [ctypes.byref(v) for v in o]
    assert lib.tfx_limiter_stream_plan_info(1, 2, 512, 72, 480, 4, 81, 0, *refs) == 0
    assert [v.value for v in o[:5]] == [81, 81 + 72 + 480 - 2 + 11, 8193 - 144 - 480, 1, 512 + 144 + 480 - 2]
    assert lib.tfx_limiter_stream_plan_info(1, 2, 512, 72, 480, 3, 81, 0, *refs) != 0
    assert lib.tfx_limiter_stream_plan_info(1, 2, 512, 72, 480, 4, 81, 0, *refs[:5], None) != 0
    assert "null output" in lib.tfx_last_error().decode()
