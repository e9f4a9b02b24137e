"""StatefulWaveshaper / StatefulDistortion on the host: chunk outputs plus flush() are torch.equal to waveshape() on the whole
signal for every oversampling factor, shape, dtype, window and chunking; the geometry is the plan query's and does not depend
on the chunk length; the constant-latency form, restarts, the two processors and Wave, the op's namespace, and what the C
entry points refuse before they touch a device.  Both stages have one length here; the stream plan at stages of unequal length, and
the refusal of gains that are not finite in the signal's dtype, are tests/test_waveshaper_cases_host.py."""
import ctypes

import numpy as np
import pytest
import torch

from torchfx_amd import Distortion, Wave, Waveshaper, waveshape
from torchfx_amd import torchfx_ext as E
from torchfx_amd.realtime import RealtimeProcessor, StatefulDistortion, StatefulWaveshaper, StreamConfig, StreamProcessor

DTYPES = {"f32": torch.float32, "f64": torch.float64}
CURVE = np.array([-0.9, -0.2, 0.05, 0.4, 0.8])
KW = dict(drive_db=9.0, bias=0.15, mix=0.7, output_db=-3.0)


def windows(L):
    """The default window spec, a 3L-tap even-length array and a 64L-tap array (none for L = 1: no filters)."""
    if L == 1:
        return {"default": ("kaiser", 5.0)}
    return {"default": ("kaiser", 5.0), "3L": np.hanning(3 * L + 2)[1:-1] / 1.5, "64L": np.hanning(64 * L + 2)[1:-1] / 32.0}


def signal(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * 1.2).to(dtype)


def run(fx, x, sizes):
    outs, o, n = [], 0, x.shape[-1]
    for k in sizes:
        outs.append(fx(x[..., o:o + k]))
        o += k
    if o < n:
        outs.append(fx(x[..., o:]))
    return outs, fx.flush()


def taps_of(L, window, dtype=torch.float32):
    return Waveshaper(oversample=L, window=window).params().taps(dtype)


def test_latency_and_history_are_the_plans_reaches_for_every_chunk_length():
    for L in (1, 2, 4, 8):
        for name, window in windows(L).items():
            up, dn = taps_of(L, window)
            n = 0 if up is None else up.numel()
            fx = StatefulWaveshaper(oversample=L, window=window)
            one = E.waveshaper_plan_info(1000, L, n, n)
            assert (fx.latency, fx.history_length) == (one["reach_before"], one["reach_before"] + one["reach_after"]), (L, name)
            for T in (1, 2, 100, 10 ** 7):
                q = E.waveshaper_plan_info(T, L, n, n)
                assert (q["reach_before"], q["reach_after"]) == (one["reach_before"], one["reach_after"]), (L, name, T)
                s = E.waveshaper_stream_plan_info(T, L, n, n, 0, torch.float64, rows=3)
                assert (s["latency"], s["history"]) == (fx.latency, fx.history_length)
                assert s["tile"] == E.waveshaper_plan_info(T, L, n, n, 0, torch.float64)["tile"] and s["tiles"] == -(-T // s["tile"])
    assert (StatefulDistortion().latency, StatefulDistortion().history_length) == (21, 41)
    assert (StatefulDistortion(oversample=1).latency, StatefulDistortion(oversample=1).history_length) == (0, 0)


def test_positions_count_whole_waves_of_the_first_tile():
    for dtype, PT, wave in ((torch.float32, 2048, 512), (torch.float64, 1024, 256)):
        for T in (1, 64, 512, 1000, 5000):
            q = E.waveshaper_stream_plan_info(T, 4, 81, 81, 0, dtype)
            need = min(T, q["tile"]) + q["latency"]                # positions 0 .. n + D - 1 of the tile (I0 = 0 here)
            assert q["positions"] == min(PT, -(-need // wave) * wave), (dtype, T, q)
        assert E.waveshaper_stream_plan_info(0, 4, 81, 81, 0, dtype)["positions"] == 0
    assert E.waveshaper_stream_plan_info(512, 4, 81, 81)["positions"] == 1024          # a real-time block: half a tile's up-sampler
    assert E.waveshaper_stream_plan_info(300, 1)["positions"] == 300


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L,win", [(L, w) for L in (1, 2, 4, 8) for w in windows(L)])
def test_chunks_plus_flush_equal_the_one_shot_result(L, win, dt):
    window, dtype = windows(L)[win], DTYPES[dt]
    D, Hs = StatefulWaveshaper(oversample=L, window=window).latency, StatefulWaveshaper(oversample=L, window=window).history_length
    n = 3 * Hs + 57
    x = signal((2, n), 10 * L + len(win), dtype)
    lists = {"edges": [0, 1, max(D - 1, 0), D, D + 1, Hs + 1, 0], "one": [n], "ones": [1] * 50, "zero_in_the_middle": [n // 3, 0, n // 4, 0]}
    for shape in ("hard", "cubic", "tanh", "curve"):
        kw = dict(KW, oversample=L, window=window, **(dict(curve=CURVE) if shape == "curve" else dict(shape=shape)))
        ref = waveshape(x, **kw)
        fx = StatefulWaveshaper(**kw)
        for name, sizes in lists.items():
            outs, tail = run(fx, x, sizes)
            N = 0
            for k, o in zip(list(sizes) + [n - sum(sizes)] * (sum(sizes) < n), outs):     # the emission rule
                assert o.shape[-1] == max(0, N + k - D) - max(0, N - D), (name, N, k)
                N += k
            assert tail.shape[-1] == min(n, D)
            got = torch.cat(outs + [tail], dim=-1)
            assert got.dtype == dtype and torch.equal(got, ref), (shape, name)
        short = x[:, :max(D - 2, 1)]                                # a stream shorter than the latency
        outs, tail = run(fx, short, [1])
        assert all(o.shape[-1] == (0 if D else k) for o, k in zip(outs, (1, short.shape[-1] - 1)))
        assert torch.equal(torch.cat(outs + [tail], dim=-1), waveshape(short, **kw)), shape


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_positions_on_the_host(bad):
    x = signal((2, 300), 3, torch.float64)
    x[0, 150] = bad
    ref = waveshape(x, "tanh", **KW)
    outs, tail = run(StatefulWaveshaper("tanh", **KW), x, [7] * 30)
    got = torch.cat(outs + [tail], dim=-1)
    mask = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), mask) and bool(mask[0, 150 - 21:150 + 21].all()) and int(mask.sum()) == 42
    assert torch.equal(got[~mask].view(torch.int64), ref[~mask].view(torch.int64))


@pytest.mark.parametrize("shape", [(400,), (2, 400), (2, 3, 400)])
def test_shapes_and_the_constant_latency_form(shape):
    x = signal(shape, 4, torch.float32)
    ref = waveshape(x, "tanh", drive_db=12.0)
    outs, tail = run(StatefulDistortion(), x, [33] * 5 + [1, 0, 90])
    assert torch.equal(torch.cat(outs + [tail], dim=-1), ref)
    fx = StatefulDistortion(aligned=False)
    D = fx.latency
    outs, tail = run(fx, x, [33] * 5 + [1, 90])
    assert all(o.shape[-1] == k for o, k in zip(outs, [33] * 5 + [1, 90, 400 - 256])) and tail.shape[-1] == D
    assert torch.equal(torch.cat(outs + [tail], dim=-1), torch.cat([torch.zeros(*shape[:-1], D), ref], dim=-1))
    one = StatefulDistortion(oversample=1, aligned=False)
    outs, tail = run(one, x, [100, 7])
    assert tail.shape[-1] == 0 and torch.equal(torch.cat(outs, dim=-1), waveshape(x, "tanh", drive_db=12.0, oversample=1))


def test_restarts_and_live_parameters():
    x = signal((2, 600), 5, torch.float64)
    kw = dict(shape="cubic", oversample=4, **KW)
    fresh = lambda **over: StatefulWaveshaper(**dict(kw, **over))     # noqa: E731
    fx = fresh()
    D = fx.latency
    fx(x[:, :300])
    # another row count, dtype: a new stream from silence, what was held back is dropped
    for other in (x[:1, 300:], x[:, 300:].float()):
        got = fx(other)
        assert torch.equal(got, fresh()(other)) and got.shape[-1] == 300 - D
        fx(x[:, :300])
    # the oversampling factor and the window's taps restart too
    for name, value in (("oversample", 2), ("oversample", 1), ("window", ("kaiser", 8.0)), ("window", np.hanning(40) / 5.0)):
        fx = fresh()
        fx(x[:, :300])
        setattr(fx, name, value)
        other = fresh(**{name: value})
        assert torch.equal(fx(x[:, 300:]), other(x[:, 300:])), name
        assert torch.equal(fx.flush(), other.flush())
    fx = fresh()
    fx(x[:, :300])
    fx.oversample = 8
    assert fx.flush().shape[-1] == 0                         # the stream the tail belonged to is gone
    # drive, bias, mix, output level, shape and curve apply from the next chunk on: the stream goes on
    for name, value in (("drive_db", 20.0), ("bias", -0.2), ("mix", 0.2), ("output_db", 3.0), ("shape", "hard")):
        fx, ref = fresh(), fresh()
        assert torch.equal(fx(x[:, :300]), ref(x[:, :300]))
        setattr(fx, name, value)
        b = fx(x[:, 300:])
        assert b.shape[-1] == 300 and not torch.equal(b, ref(x[:, 300:])), name
        # from `reach_after` behind the change on, the outputs are the changed effect's on the whole signal
        assert torch.equal(b[:, D:], waveshape(x, **dict(kw, **{name: value}))[:, 300:600 - D]), name
        assert fx.flush().shape[-1] == D
    fx = StatefulWaveshaper(curve=CURVE)
    a = fx(x[:, :300])
    fx.curve = CURVE[::-1].copy()
    assert fx(x[:, 300:]).shape[-1] == 300 and a.shape[-1] == 300 - D
    fx.reset_state()                                         # by hand
    assert torch.equal(fx(x[:, :200]), StatefulWaveshaper(curve=CURVE[::-1].copy())(x[:, :200]))


def test_empty_stream_and_bad_dtype():
    fx = StatefulDistortion()
    assert fx.flush().numel() == 0
    assert fx(torch.zeros(2, 0)).shape == (2, 0) and fx.flush().shape == (2, 0)
    with pytest.raises(TypeError, match="float32 or float64"):
        StatefulDistortion()(torch.zeros(2, 10, dtype=torch.float16))
    assert isinstance(StatefulDistortion(), Distortion) and isinstance(StatefulWaveshaper(), Waveshaper)
    assert (StatefulDistortion().drive_db, StatefulDistortion().aligned, StatefulDistortion(aligned=False).aligned) == (12.0, True, False)
    assert StatefulDistortion().route(torch.zeros(2, 10)).startswith("scipy on host")


def test_route_names_the_stream_kernel_for_a_device_tensor():
    class OnDevice:                       # what route() reads of a device tensor
        is_cuda, dtype, shape, device = True, torch.float32, (2, 512), torch.device("meta")

    assert StatefulDistortion().route(OnDevice()) == (
        "native (waveshaper_stream_kernel, L = 4, tanh, latency 21, history 41, 1 tile(s) of 2027, 1024 positions up-sampled and "
        "shaped; one launch)")
    assert "waveshaper_stream_kernel, L = 1, hard, latency 0, history 0" in StatefulWaveshaper("hard", oversample=1).route(OnDevice())


def test_processors_take_the_stateful_class_and_refuse_the_plain_one():
    from torch import nn

    from torchfx_amd.effect import FX, Gain

    class Wrap(FX):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x)

    for who in (Distortion(), Waveshaper("hard", oversample=2)):
        with pytest.raises(TypeError, match=r"cannot run in StreamProcessor: every call zero-pads.*Stateful" + type(who).__name__):
            StreamProcessor([who], chunk_size=64, device="cpu")
    with pytest.raises(TypeError, match=r"cannot run in RealtimeProcessor: every call zero-pads.*StatefulDistortion"):
        RealtimeProcessor([Distortion()], object(), StreamConfig(), device="cpu")
    with pytest.raises(TypeError, match="top-level effect"):
        StreamProcessor([Gain(0.5), Wrap(StatefulDistortion())], device="cpu")
    with pytest.raises(ValueError, match="StatefulDistortion needs overlap = 0"):
        StreamProcessor([StatefulDistortion()], chunk_size=1000, overlap=10, device="cpu")
    with pytest.raises(TypeError, match="aligned=False"):
        RealtimeProcessor([StatefulDistortion()], object(), StreamConfig(), device="cpu")
    with pytest.raises(TypeError, match="are for chunked streams"):
        Wave(torch.zeros(2, 100), 48000, device="cpu") | StatefulWaveshaper()
    with pytest.raises(TypeError, match="are for chunked streams"):
        Wave(torch.zeros(2, 100), 48000, device="cpu") | nn.Sequential(Gain(0.5), StatefulDistortion())
    StreamProcessor([StatefulDistortion(), StatefulWaveshaper("hard", oversample=8)], chunk_size=64, device="cpu")
    p = RealtimeProcessor([Gain(0.5), StatefulDistortion(aligned=False)], object(), StreamConfig(), device="cpu")
    assert p.chain_latency_samples == 21


def test_stream_processor_equals_the_one_shot_call(oracle_backend):
    from torchfx_amd.effect import Gain
    x = signal((2, 3000), 6, torch.float32)
    ref = waveshape(Gain(0.5)(x), "tanh", drive_db=12.0)
    for chunk in (16, 64, 1000, 3000):
        proc = StreamProcessor([Gain(0.5), StatefulDistortion()], chunk_size=chunk, device="cpu")
        got = proc.process_tensor(x, 48000)
        assert got.shape == ref.shape and torch.equal(got, ref), chunk
    # two of them in a row: the first one's tail goes through the second before the second hands out its own
    ref2 = waveshape(ref, "hard", oversample=2, drive_db=3.0)
    proc = StreamProcessor([Gain(0.5), StatefulDistortion(), StatefulWaveshaper("hard", oversample=2, drive_db=3.0)], chunk_size=100,
                           device="cpu")
    assert torch.equal(proc.process_tensor(x, 48000), ref2)


def test_realtime_processor_runs_the_constant_latency_form(oracle_backend):
    from tests.test_host_logic import _MockBackend
    x = signal((2, 512 * 5), 7, torch.float32)
    be = _MockBackend()
    cfg = StreamConfig(sample_rate=48000, buffer_size=512, channels_in=2, channels_out=2)
    fx = StatefulDistortion(aligned=False)
    with RealtimeProcessor([fx], be, cfg, device="cpu") as p:
        D = p.chain_latency_samples
        assert D == fx.latency == 21
        outs = [be.simulate_callback(x[:, i:i + 512]) for i in range(0, x.shape[-1], 512)]
    assert all(o.shape == (2, 512) for o in outs)
    got = torch.cat(outs, dim=-1)
    assert torch.equal(got[:, :D], torch.zeros(2, D)) and torch.equal(got[:, D:], waveshape(x, "tanh", drive_db=12.0)[:, :-D])


def test_namespace_holds_exactly_its_op():
    from torchfx_amd import native

    ops = native.shaper_stream_ops()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_shaper_stream::")}
    op = "torchfx_shaper_stream::waveshaper_stream_forward"
    assert names == {op}
    for key in ("CUDA", "CPU", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op, key), key
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.waveshaper_stream_forward(torch.zeros(2, 8), None, 0, 1, 2, None, 1.0, 0.0, 0.0, 1.0, None, None, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.waveshaper_stream_forward(torch.zeros(2, 8), None, 0, 1, "tanh", None, 1.0, 0.0, 0.0, 1.0)
    y, h = ops.waveshaper_stream_forward(torch.empty(2, 3, 77, device="meta"), None, 0, 4, 0, None, 1.0, 0.0, 0.0, 1.0,
                                         torch.empty(81), torch.empty(81), -1)
    assert y.shape == (2, 3, 77) and h.shape == (6, 41) and y.device.type == h.device.type == "meta"
    y, h = ops.waveshaper_stream_forward(torch.empty(5, 9, device="meta", dtype=torch.float64), None, 0, 1, 2, None, 1.0, 0.0, 0.0, 1.0,
                                         None, None, -1)
    assert y.shape == (5, 9) and h.shape == (5, 0) and h.dtype == torch.float64
    assert "waveshaper_stream_forward" in E.__all__ and "waveshaper_stream_plan_info" in E.__all__


def test_capi_checks_arguments_before_the_device():
    from torchfx_amd import _lib
    lib = _lib.load()
    h = (ctypes.c_float * 81)()
    c = (ctypes.c_float * 5)(*CURVE)
    x, y, hin, hout = [ctypes.c_void_p(16 + (1 << 20) * i) for i in range(4)]

    def call(*a):
        rc = lib.tfx_waveshaper_stream_forward(*a, None)
        return rc, lib.tfx_last_error().decode()

    #       x  y  dtype rows T  n_in consumed L shape curve n drive bias dry wet taps_up nh taps_dn nh hist_in hist_out
    good = (x, y, 0, 2, 100, 100, 0, 4, 2, None, 0, 2.0, 0.1, 0.3, 0.7, h, 81, h, 81, hin, hout)
    bad = {
        "bad dtype": {2: 7}, "oversample must be 1, 2, 4 or 8": {7: 3}, "negative size": {4: -1}, "n_in = 101": {5: 101},
        "n_in = -1": {5: -1}, "negative stream position": {6: -1}, "bad shape": {8: 4}, "no curve": {8: 3, 10: 5},
        "2 to 4096 points": {8: 3, 9: c, 10: 1}, "curve points with a shape that is no curve": {10: 5},
        "must be finite": {11: float("inf")}, "no taps": {15: None}, "at most 64": {16: 257}, "null pointer": {1: None},
        "the new history needs its own buffer": {20: hin},
        "y and hist_out may not overlap x, hist_in or each other": {1: x},
    }
    for msg, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        rc, err = call(*args)
        assert rc != 0 and err.startswith("waveshaper_stream_forward: ") and msg in err, (msg, rc, err)
    for k, v in ((20, x), (20, y), (1, hin), (1, hout), (19, y)):        # every other overlap
        args = list(good)
        args[k] = v
        rc, err = call(*args)
        assert rc != 0 and "may not overlap" in err, (k, err)
    # a partial overlap: y starts inside x's last row
    args = list(good)
    args[1] = ctypes.c_void_p(16 + 4 * 150)
    rc, err = call(*args)
    assert rc != 0 and "may not overlap" in err
    o = [ctypes.c_int64() for _ in range(6)]
    refs = [ctypes.byref(v) for v in o]
    assert lib.tfx_waveshaper_stream_plan_info(2, 512, 4, 81, 81, 0, 0, *refs) == 0
    assert [v.value for v in o[:5]] == [21, 41, 2027, 1, 1024]
    assert lib.tfx_waveshaper_stream_plan_info(2, 512, 3, 81, 81, 0, 0, *refs) != 0
    assert lib.tfx_waveshaper_stream_plan_info(2, 512, 4, 81, 81, 0, 0, *refs[:5], None) != 0
    assert "null output" in lib.tfx_last_error().decode()
    # empty work touches nothing
    assert lib.tfx_waveshaper_stream_forward(None, None, 0, 0, 100, 100, 0, 4, 2, None, 0, 2.0, 0.1, 0.3, 0.7, h, 81, h, 81, None, None,
                                             None) == 0
