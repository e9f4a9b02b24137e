"""StatefulResample without a GPU: chunked output plus flush() against scipy.signal.resample_poly on the whole signal (CPU
routing: scipy.signal.upfirdn over [history | chunk]), the emission rule per chunk, the restart rules, StreamProcessor and
process_file with a resampler in the chain, the refusals, the new op's Meta shape and the C ABI's argument checks."""
import ctypes
import math
import random
import sys

import numpy as np
import pytest
import scipy.signal as ss
import torch

# the ratios of tests/test_gpu_resample.py (TABLE + EXTRA)
RATIOS = [(160, 147), (147, 160), (1, 3), (3, 1), (1, 6), (441, 80), (160, 441), (997, 1000), (1, 480), (480, 1), (3, 7)]
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}            # TOL_CONV_F32 / TOL_CONV_F64 of tests/gpu_common.py
NP = {torch.float32: np.float32, torch.float64: np.float64}


def rnd(shape, seed, dtype=torch.float32):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, shape)).to(dtype)


def stateful(up, down, **kw):
    from torchfx_amd.realtime import StatefulResample
    return StatefulResample(up * 100, down * 100, **kw)


def emitted(n, up, down, pre):
    return max(0, math.ceil(n * up / down) - pre)


def chunked(r, x, sizes):
    """Feed x in chunks of `sizes` (the rest in one chunk), then flush; returns the chunk outputs and the flush."""
    outs, o, n = [], 0, x.shape[-1]
    sizes = list(sizes)
    while o < n:
        k = sizes.pop(0) if sizes else n - o
        outs.append(r(x[..., o:o + k]))
        o += k
    return outs, r.flush()


def random_sizes(n, seed, hi):
    rng = random.Random(seed)
    out = []
    while sum(out) < n:
        out.append(rng.randint(1, hi))
    return out


def check_against_scipy(x, up, down, outs, tail, what):
    got = torch.cat([*outs, tail], dim=-1)
    ref = ss.resample_poly(x.numpy(), up, down, axis=-1)
    assert got.shape == ref.shape and got.dtype == x.dtype, (what, got.shape, ref.shape)
    err = np.abs(got.numpy() - ref).max() / max(1.0, np.abs(ref).max()) if ref.size else 0.0
    assert err <= TOL[x.dtype], (what, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("up,down", RATIOS)
def test_chunkings_match_scipy(up, down, dtype):
    T = 5003
    x = rnd((2, T), up * 7 + down, dtype)
    hl = stateful(up, down).history_length
    for name, sizes in [("random", random_sizes(T, up + down, 700)), ("shorter than the history", [max(1, hl // 3)] * 40),
                        ("single", [T]), ("with empty chunks", [0, 100, 0, 1, 0])]:
        outs, tail = chunked(stateful(up, down), x, sizes)
        check_against_scipy(x, up, down, outs, tail, f"{up}/{down} {name}")


@pytest.mark.parametrize("up,down", [(160, 147), (1, 6), (3, 1)])
def test_one_sample_chunks(up, down):
    x = rnd((2, 600), 3, torch.float64)
    outs, tail = chunked(stateful(up, down), x, [1] * 600)
    check_against_scipy(x, up, down, outs, tail, "1-sample chunks")


@pytest.mark.parametrize("shape", [(3001,), (3, 3001), (2, 2, 3001)])
def test_shapes(shape):
    x = rnd(shape, 4, torch.float32)
    outs, tail = chunked(stateful(160, 147), x, [512] * 10)
    assert all(o.shape[:-1] == shape[:-1] for o in outs) and tail.shape[:-1] == shape[:-1]
    check_against_scipy(x, 160, 147, outs, tail, str(shape))


@pytest.mark.parametrize("up,down", RATIOS)
def test_emission_rule(up, down):
    r = stateful(up, down)
    pre = r.latency
    n = 0
    for T in random_sizes(4000, up * down, 300) + [0, 1, 0]:
        y = r(rnd((2, T), T))
        assert y.shape == (2, emitted(n + T, up, down, pre) - emitted(n, up, down, pre)), (n, T)
        n += T
    total = math.ceil(n * up / down)
    assert r._emitted == emitted(n, up, down, pre) and r._consumed == n
    tail = r.flush()
    assert tail.shape == (2, total - emitted(n, up, down, pre)) and tail.shape[-1] <= pre


def test_geometry_matches_the_c_side_and_the_issue_numbers():
    from torchfx_amd import torchfx_ext
    for up, down in RATIOS:
        r = stateful(up, down)
        info = torchfx_ext.resample_stream_plan_info(0, 1000, up, down, 2 * 10 * max(up, down) + 1)
        assert (r.latency, r.history_length) == (info["n_pre_remove"], info["hist_len"])
        assert (info["out_begin"], info["out_end"]) == (0, emitted(1000, up, down, r.latency))
    r = stateful(480, 441)                                      # 44.1k -> 48k
    assert (r.up, r.down, r.history_length, r.latency) == (160, 147, 20, 11)
    r = stateful(8, 48)                                         # 48k -> 8k
    assert (r.history_length, r.latency) == (126, 11)
    assert torchfx_ext.resample_stream_plan_info(10, 5, 7, 7, 1)["kernel"] == "copy"
    assert torchfx_ext.resample_stream_plan_info(0, 512, 160, 147, 3201)["kernel"] == "resample_stream_reg_kernel"
    assert torchfx_ext.resample_stream_plan_info(0, 512, 1, 6, 121)["kernel"] == "resample_stream_lds_kernel"
    assert torchfx_ext.resample_stream_plan_info(0, 512, 1, 480, 9601, torch.float64)["kernel"] == "resample_stream_gather_kernel"


def test_empty_stream_and_zero_length_chunk():
    r = stateful(160, 147)
    assert r.flush().numel() == 0
    y = r(torch.zeros(2, 0))
    assert y.shape == (2, 0)
    assert r.flush().shape == (2, 0)


def test_equal_rates_pass_through():
    r = stateful(3, 3)
    x = rnd((2, 100), 5)
    assert torch.equal(r(x), x) and r.latency == 0 and r.history_length == 0
    assert r.flush().shape == (2, 0)


def test_restarts():
    x = rnd((2, 3000), 6, torch.float64)
    ref = ss.resample_poly(x[:, 1000:].numpy(), 160, 147, axis=-1)
    for change in ("rows", "dtype", "param"):
        r = stateful(160, 147)
        if change == "rows":
            r(rnd((3, 1000), 7, torch.float64))
        elif change == "dtype":
            r(x[:, :1000].float())
        else:
            r.window = ("kaiser", 6.0)
            r(x[:, :1000])
            r.window = ("kaiser", 5.0)
        outs, tail = chunked(r, x[:, 1000:], [700] * 3)
        got = torch.cat([*outs, tail], dim=-1).numpy()
        assert got.shape == ref.shape, change
        assert np.abs(got - ref).max() <= 1e-11, change
    r = stateful(160, 147)
    r(x[:, :1000])
    r.new_fs, r.fs = 48000, 44100                               # the same ratio, new rates: a new stream, held-back outputs dropped
    assert r(x[:, :10]).shape[-1] == 0 and r._consumed == 10


def test_bad_dtype():
    with pytest.raises(TypeError, match="float32 or float64"):
        stateful(160, 147)(torch.zeros(2, 10, dtype=torch.float16))
    with pytest.raises(ValueError, match="shape"):
        stateful(160, 147)(torch.zeros(2, 2, 2, 10))


def _scale(k):
    """A gain that also runs on the host (the library's Gain is device-only)."""
    from torchfx_amd import FX

    class Scale(FX):
        def forward(self, x):
            return x * k
    return Scale()


def _gain_chain(up, down):
    from torchfx_amd.realtime import StatefulResample
    return [_scale(0.5), StatefulResample(up * 100), _scale(2.0)]


def test_stream_processor_on_cpu_equals_the_one_shot_chain():
    from torchfx_amd.realtime import StreamProcessor
    x = rnd((2, 10_000), 8)
    ref = ss.resample_poly((x * 0.5).numpy(), 160, 147, axis=-1) * 2.0
    for chunk in (512, 3000, 65536):
        proc = StreamProcessor(_gain_chain(160, 147), chunk_size=chunk, device="cpu")
        chunks = list(proc.process_chunks(x, 14700))
        assert all(c.shape[-1] > 0 for c in chunks)
        got = torch.cat(chunks, dim=-1)
        assert got.shape == (2, math.ceil(10_000 * 160 / 147)) and proc.output_rate(14700) == 16000
        assert np.abs(got.numpy() - ref).max() <= 1e-5, chunk
        assert torch.equal(proc.process_tensor(x, 14700), got)       # flush() reset the stream: a second run is the same


def test_stream_processor_skips_chunks_with_no_output():
    from torchfx_amd import FX
    from torchfx_amd.realtime import StatefulResample, StreamProcessor
    calls = []

    class Spy(FX):
        def forward(self, x):
            calls.append(x.shape[-1])
            return x
    proc = StreamProcessor([StatefulResample(1), Spy()], chunk_size=3, device="cpu")     # 6 -> 1: 11 outputs held
    chunks = list(proc.process_chunks(rnd((1, 90), 9), 6))
    assert 0 not in calls and sum(calls) == 15 and sum(c.shape[-1] for c in chunks) == 15


def test_two_resamplers_and_rates():
    from torchfx_amd.filter import LoButterworth
    from torchfx_amd.realtime import StatefulResample, StreamProcessor
    lo = LoButterworth(20000)
    a, b = StatefulResample(48000), StatefulResample(16000)
    proc = StreamProcessor([_scale(1.0), a, lo, b, _scale(1.0)], chunk_size=1000, device="cpu")
    proc._configure_effects(44100)
    assert (a.fs, lo.fs, b.fs) == (44100, 48000, 48000) and proc.output_rate(44100) == 16000
    assert lo._has_computed_coeff
    with pytest.raises(ValueError, match="Nyquist"):
        StreamProcessor([StatefulResample(16000), LoButterworth(10000)], device="cpu")._configure_effects(44100)
    x = rnd((2, 7000), 10)
    proc2 = StreamProcessor([StatefulResample(48000), StatefulResample(16000)], chunk_size=999, device="cpu")
    got = proc2.process_tensor(x, 44100)
    ref = ss.resample_poly(ss.resample_poly(x.numpy(), 160, 147, axis=-1), 1, 3, axis=-1)
    assert got.shape == ref.shape and np.abs(got.numpy() - ref).max() <= 1e-5


def test_stream_processor_refusals():
    from torchfx_amd import FX, Gain, Resample
    from torchfx_amd.realtime import StatefulResample, StreamProcessor

    class Wrap(FX):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x)
    with pytest.raises(ValueError, match="overlap"):
        StreamProcessor([StatefulResample(16000)], chunk_size=1000, overlap=10, device="cpu")
    with pytest.raises(TypeError, match="Resample.*StatefulResample"):
        StreamProcessor([Gain(0.5), Resample(16000)], device="cpu")
    with pytest.raises(TypeError, match="Resample.*StatefulResample"):
        StreamProcessor([Gain(0.5), Wrap(StatefulResample(16000))], device="cpu")
    StreamProcessor([Gain(0.5), StatefulResample(16000)], chunk_size=1000, device="cpu")


def test_process_file_writes_the_new_rate(tmp_path, monkeypatch):
    from tests import _fake_soundfile as sf
    from torchfx_amd.realtime import StreamProcessor
    monkeypatch.setitem(sys.modules, "soundfile", sf)
    frames = (np.random.default_rng(11).standard_normal((20_000, 2)) * 0.3).astype(np.float32)
    src = tmp_path / "in.wav"
    sf.make(src, frames, 44100, subtype="FLOAT")
    proc = StreamProcessor(_gain_chain(480, 441), chunk_size=4096, device="cpu")
    proc.process_file(src, tmp_path / "out.wav")
    rec = sf.written[-1]
    assert rec["fs"] == 48000 and rec["data"].shape == (math.ceil(20_000 * 160 / 147), 2)
    ref = ss.resample_poly(frames.T * np.float32(0.5), 160, 147, axis=-1) * 2.0
    assert np.abs(rec["data"].T - ref).max() <= 1e-5


def test_realtime_processor_and_wave_refuse_it():
    from torchfx_amd import Gain, Wave
    from torchfx_amd.realtime import AudioBackend, RealtimeProcessor, StatefulResample, StreamConfig

    class Null(AudioBackend):
        def open_stream(self, config, callback=None): ...
        def start(self): ...
        def stop(self): ...
        def close(self): ...
    with pytest.raises(TypeError, match="StatefulResample cannot run in RealtimeProcessor"):
        RealtimeProcessor([Gain(1.0), StatefulResample(16000)], Null(), StreamConfig(), device="cpu")
    w = Wave(rnd((2, 1000), 12), 44100)
    with pytest.raises(TypeError, match="Resample"):
        w | StatefulResample(48000)


def test_meta_shape_and_no_cpu_path():
    from torchfx_amd import native
    from torchfx_amd.resample import design_taps
    native.load()
    h = design_taps(160, 147)
    y, hist = torch.ops.torchfx_hip.resample_stream_forward(torch.empty(2, 3, 512, device="meta"), h, None, 160, 147, 1000)
    assert tuple(y.shape) == (2, 3, emitted(1512, 160, 147, 11) - emitted(1000, 160, 147, 11)) and y.device.type == "meta"
    assert tuple(hist.shape) == (6, 20)
    y, hist = torch.ops.torchfx_hip.resample_stream_forward(torch.empty(4, 0, device="meta"), h, None, 160, 147, 0)
    assert tuple(y.shape) == (4, 0) and tuple(hist.shape) == (4, 20)
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.torchfx_hip.resample_stream_forward(torch.zeros(2, 100), h, None, 160, 147, 0)


def test_capi_checks_arguments_before_the_device():
    from torchfx_amd import _lib
    lib = _lib.load()
    h = (ctypes.c_float * 5)()
    d = [ctypes.c_void_p(16 + 4096 * i) for i in range(4)]
    x, y, hin, hout = d
    bad = [
        (x, y, 7, 1, 10, 2, 3, h, 5, 0, None, hout),                 # dtype
        (x, y, 0, 1, 10, 0, 3, h, 5, 0, None, hout),                 # up
        (x, y, 0, 1, 10, 2, 3, None, 5, 0, None, hout),              # taps
        (x, y, 0, 1, 10, 2, 3, h, 0, 0, None, hout),                 # nh
        (x, y, 0, 1, 10, 2, 3, h, 5, -1, None, hout),                # consumed
        (x, y, 0, 1, -1, 2, 3, h, 5, 0, None, hout),                 # T
        (None, y, 0, 1, 10, 2, 3, h, 5, 0, None, hout),              # null x
        (x, y, 0, 1, 10, 3, 2, h, 5, 0, None, None),                 # null hist_out
        (x, y, 0, 1, 10, 2, 3, h, 5, (1 << 62) // 6, None, hout),    # (consumed + T) * up * down overflows
        (x, x, 0, 1, 10, 3, 2, h, 5, 0, None, hout),                 # y overlaps x
        (x, y, 0, 1, 10, 3, 2, h, 5, 0, hin, hin),                   # history in place
        (x, y, 0, 1, 10, 3, 2, h, 5, 0, None, x),                    # hist_out overlaps x
    ]
    for args in bad:
        assert lib.tfx_resample_stream_forward(*args, None) != 0, args
    o = ctypes.c_int64()
    assert lib.tfx_resample_stream_plan_info(0, 10, 0, 3, 5, 0, *[ctypes.byref(o)] * 5, ctypes.byref(ctypes.c_int()),
                                             ctypes.byref(o)) != 0
    assert lib.tfx_resample_stream_plan_info(0, 10, 2, 3, 5, 0, *[ctypes.byref(o)] * 5, None, ctypes.byref(o)) != 0


def test_top_level_names():
    from torchfx_amd import torchfx_ext
    from torchfx_amd.realtime import StatefulResample
    from torchfx_amd.resample import Resample
    assert issubclass(StatefulResample, Resample)
    assert "resample_stream_forward" in torchfx_ext.__all__ and "resample_stream_plan_info" in torchfx_ext.__all__
    r = StatefulResample(48000, 44100)
    assert r.route(torch.zeros(2, 10)).startswith("scipy on host")
