"""The waveshaper without a GPU: the CPU path of torchfx_amd.waveshaper against the float64 definition of
tests/waveshaper_reference.py within its bound (hard: exact against numpy's clip of the SciPy composition), argument refusals,
the effects in a Wave and in the stream processors, the op namespace, the host-only plan query against a NaN probe of the CPU
path, the transfer functions' measured error (tools/shape_sweep.cpp, compiled here) and the alias figures of the design note.
The plan at every register bucket and at stages of unequal length, the exact tap probes' own checks and the refusal of gains that
are not finite in the signal's dtype are tests/test_waveshaper_cases_host.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import waveshaper_reference as R
from torchfx_amd import Distortion, Wave, Waveshaper, waveshape
from torchfx_amd import torchfx_ext as E
from torchfx_amd.resample import design_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
CURVES = {
    "curve2": np.array([-1.0, 1.0]),
    "curve3": np.array([-0.5, 0.1, 0.8]),
    "curve4096": np.tanh(3.0 * np.linspace(-1.0, 1.0, 4096)),
}


def signal(shape, seed, dt):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(dt)


def plan(T, L, tdt, curve=0):
    n = 20 * L + 1 if L > 1 else 0
    return E.waveshaper_plan_info(T, L, n, n, curve, tdt)


def taps(L, tdt):
    if L == 1:
        return None, None
    return design_taps(L, 1, ("kaiser", 5.0), tdt).numpy(), design_taps(1, L, ("kaiser", 5.0), tdt).numpy()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", ["tanh", "cubic", "curve2", "curve3", "curve4096"])
def test_cpu_path_is_within_the_bound(shape, L, dt):
    tdt, ndt = DT[dt]
    x = signal((2, 700), 7, ndt)
    kw = dict(drive_db=9.0, bias=0.15, mix=0.3, output_db=-6.0)
    curve = CURVES.get(shape)
    y = waveshape(torch.from_numpy(x), None if curve is not None else shape, oversample=L, curve=curve, **kw)
    assert y.dtype == tdt and y.shape == x.shape
    hu, hd = taps(L, tdt)
    info = plan(700, L, tdt)
    R.check(y.numpy(), x, L, hu, hd, info["taps_up"], info["taps_dn"], "curve" if curve is not None else shape,
            what=f"cpu {shape} L={L} {dt}", curve=curve, **kw)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("L", [1, 2, 4, 8])
def test_cpu_hard_is_the_clipped_scipy_composition(L, dt):
    from scipy.signal import resample_poly

    tdt, ndt = DT[dt]
    x = signal((3, 500), 11, ndt)
    drive = ndt(10.0 ** (6.0 / 20.0))
    u = resample_poly(x, L, 1, axis=-1).astype(ndt) if L > 1 else x
    w = np.clip(u * drive, ndt(-1), ndt(1))
    want = resample_poly(w, 1, L, axis=-1).astype(ndt) if L > 1 else w
    got = waveshape(torch.from_numpy(x), "hard", drive_db=6.0, oversample=L).numpy()
    assert np.array_equal(got, ndt(0) * x + ndt(1) * want)
    assert torch.equal(waveshape(torch.from_numpy(x), "tanh", drive_db=20.0, oversample=L, mix=0.0), torch.from_numpy(x))


def test_shapes_and_empty_signals():
    for shape in ((9,), (2, 9), (2, 2, 9), (0,), (2, 0)):
        x = torch.zeros(shape)
        assert waveshape(x, "cubic", bias=0.3).shape == x.shape
    assert float(waveshape(torch.zeros(50), "tanh", bias=0.4, drive_db=12).abs().max()) == 0.0      # c0 keeps silence silent


@pytest.mark.parametrize("kw, err, msg", [
    (dict(oversample=3), ValueError, "oversample must be one of"),
    (dict(oversample=True), ValueError, "oversample must be one of"),
    (dict(shape="soft"), ValueError, "shape must be one of"),
    (dict(shape="tanh", curve=[-1.0, 1.0]), ValueError, "a shape or a curve, not both"),
    (dict(curve=[0.5]), ValueError, "2 to 4096 points"),
    (dict(curve=np.zeros(4097)), ValueError, "2 to 4096 points"),
    (dict(curve=np.zeros((2, 2))), TypeError, "1-D array"),
    (dict(curve=[0.0, float("nan")]), ValueError, "curve must be finite"),
    (dict(drive_db=float("inf")), ValueError, "drive_db must be a finite number"),
    (dict(bias=float("nan")), ValueError, "bias must be a finite number"),
    (dict(mix="1"), ValueError, "mix must be a finite number"),
    (dict(output_db=float("-inf")), ValueError, "output_db must be a finite number"),
    (dict(drive_db=1e6), ValueError, "finite gains"),
    (dict(oversample=2, window=np.ones(129)), ValueError, "at most 64 \\* oversample = 128"),
])
def test_argument_refusals(kw, err, msg):
    with pytest.raises(err, match=msg):
        waveshape(torch.zeros(2, 64), **kw)
    if "window" not in kw:
        with pytest.raises(err, match=msg):
            Waveshaper(**kw)


def test_signal_refusals():
    with pytest.raises(TypeError, match="torch.Tensor"):
        waveshape(np.zeros(8))
    with pytest.raises(TypeError, match="float32 or float64"):
        waveshape(torch.zeros(8, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"\[T\], \[C, T\], or \[B, C, T\]"):
        waveshape(torch.zeros(1, 1, 1, 8))
    assert waveshape(torch.ones(40), window=np.ones(128) / 128, oversample=2).shape == (40,)      # a tap array at the cap


def test_effects_in_a_wave(oracle_backend):
    x = torch.from_numpy(signal((2, 900), 3, np.float32))
    d = Distortion()
    assert (d.drive_db, d.shape, d.oversample, d.mix) == (12.0, "tanh", 4, 1.0) and isinstance(d, Waveshaper)
    w = Wave(x, 48000) | Distortion()
    assert [type(m).__name__ for m in w.plan()] == ["Distortion"]
    assert w.explain() == ["Distortion: scipy on host -- cpu tensor"]
    assert torch.equal(w.ys, waveshape(x, "tanh", drive_db=12.0))
    from torchfx_amd import Gain

    w2 = Wave(x, 48000) | Gain(0.5) | Waveshaper(curve=CURVES["curve3"], oversample=2, mix=0.5) | Gain(2.0)
    assert [type(m).__name__ for m in w2.plan()] == ["Gain", "Waveshaper", "Gain"]          # a step of its own
    assert torch.equal(w2.ys, Gain(2.0)(waveshape(Gain(0.5)(x), curve=CURVES["curve3"], oversample=2, mix=0.5)))
    assert "curve=3 points" in repr(Waveshaper(curve=CURVES["curve3"])) and "shape='tanh'" in repr(Waveshaper())


def test_route_names_the_kernel_for_a_device_tensor():
    x = torch.empty(2, 5000, device="meta")

    class OnDevice:                       # what route() reads of a device tensor
        is_cuda, dtype, shape, device = True, torch.float32, x.shape, x.device

    info = plan(5000, 4, torch.float32)
    assert Waveshaper("hard", oversample=4).route(OnDevice()) == (
        f"native (waveshaper_kernel, L = 4, hard, {info['taps_up']} taps per phase up and {info['taps_dn']} taps down, "
        f"{info['tiles']} tile(s) of {info['tile']} per row, {info['lds_bytes']} B of LDS; one launch)")
    assert "waveshaper_plain_kernel, L = 1" in Waveshaper(oversample=1).route(OnDevice())
    assert Waveshaper(oversample=2, window=np.ones(200)).route(OnDevice()).startswith("refused -- waveshape: 200 taps")


def test_stream_processors_take_oversample_one_only():
    from torchfx_amd.realtime import RealtimeProcessor, StreamConfig, StreamProcessor

    for who in (Distortion(), Waveshaper("hard", oversample=2)):
        with pytest.raises(TypeError, match="cannot run in StreamProcessor: every call zero-pads"):
            StreamProcessor([who], chunk_size=64)
    with pytest.raises(TypeError, match="cannot run in RealtimeProcessor"):
        RealtimeProcessor([Distortion()], object(), StreamConfig(), device="cpu")       # refused before the backend is touched
    fx = Distortion(oversample=1, bias=0.1)
    StreamProcessor([fx], chunk_size=64)
    x = torch.from_numpy(signal((2, 300), 5, np.float32))
    chunks = [fx(x[:, a:a + 64]) for a in range(0, 300, 64)]
    assert torch.equal(torch.cat(chunks, dim=-1), fx(x))


def test_namespace_holds_exactly_its_op():
    from torchfx_amd import native

    ops = native.shaper_ops()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_shaper::")}
    assert names == {"torchfx_shaper::waveshaper_forward"}
    assert torch._C._dispatch_has_kernel_for_dispatch_key("torchfx_shaper::waveshaper_forward", "CUDA")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("torchfx_shaper::waveshaper_forward", "CPU")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.waveshaper_forward(torch.zeros(2, 8), 1, 2, None, 1.0, 0.0, 0.0, 1.0, None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.waveshaper_forward(torch.zeros(2, 8), 1, "tanh", None, 1.0, 0.0, 0.0, 1.0)
    y = ops.waveshaper_forward(torch.empty(2, 3, 77, device="meta"), 4, 0, None, 1.0, 0.0, 0.0, 1.0, None, None)
    assert y.shape == (2, 3, 77) and y.device.type == "meta"


@pytest.mark.parametrize("L", [2, 4, 8])
def test_plan_info_reach_is_the_cpu_paths(L):
    info = plan(3000, L, torch.float64)
    assert (info["reach_before"], info["reach_after"]) == (21, 20)
    first, last = R.reach_probe(lambda a: waveshape(torch.from_numpy(a), "tanh", oversample=L).numpy(), 400, 200)
    assert (200 - first, last - 200) == (info["reach_before"], info["reach_after"])
    h = np.hanning(37 * L)                                           # a tap array: another geometry
    q = E.waveshaper_plan_info(3000, L, h.size, h.size, 0, torch.float64)
    first, last = R.reach_probe(lambda a: waveshape(torch.from_numpy(a), "hard", oversample=L, window=h).numpy(), 400, 200)
    assert (200 - first, last - 200) == (q["reach_before"], q["reach_after"])


def test_plan_info_without_a_device():
    q = plan(5000, 8, torch.float32)
    assert q["tiles"] == -(-5000 // q["tile"]) and 1500 < q["tile"] <= 2048 and 2 * q["lds_bytes"] <= 160 * 1024
    q64 = plan(5000, 8, torch.float64, curve=0)
    assert 750 < q64["tile"] <= 1024 and 2 * q64["lds_bytes"] <= 160 * 1024
    assert plan(5000, 1, torch.float32) == dict(tile=1024, tiles=5, reach_before=0, reach_after=0, lds_bytes=0, taps_up=0, taps_dn=0)
    assert plan(0, 4, torch.float32)["tiles"] == 0
    assert E.waveshaper_plan_info(100, 4, 81, 81, 4096, torch.float32)["lds_bytes"] == plan(100, 4, torch.float32)["lds_bytes"] + 4 * 4096
    for args, msg in [((1, -1, 4, 81, 81, 0, 0), "negative size"), ((1, 10, 3, 81, 81, 0, 0), "oversample must be 1, 2, 4 or 8"),
                      ((1, 10, 4, 0, 81, 0, 0), "no taps"), ((1, 10, 4, 257, 257, 0, 0), "at most 64"),
                      ((1, 10, 4, 81, 81, 1, 0), "2 to 4096 points"), ((1, 10, 4, 81, 81, 0, 7), "bad dtype")]:
        with pytest.raises(RuntimeError, match=msg):
            E._query(E.L.load().tfx_waveshaper_plan_info, args, "tile tiles reach_before reach_after lds_bytes taps_up taps_dn")
    lib = E.L.load()
    out = [ctypes.c_int64() for _ in range(7)]
    ptrs = [ctypes.byref(o) for o in out]
    assert lib.tfx_waveshaper_plan_info(1, 10, 4, 81, 81, 0, 0, *ptrs) == 0
    assert lib.tfx_waveshaper_plan_info(1, 10, 4, 81, 81, 0, 0, None, *ptrs[1:]) != 0
    assert b"null output" in lib.tfx_last_error()
    assert lib.tfx_waveshaper_forward(None, None, 0, 1, 10, 4, 2, None, 0, 1.0, 0.0, 0.0, 1.0, None, 81, None, 81, None) != 0
    assert b"waveshaper_forward" in lib.tfx_last_error()


def test_sampled_shape_sweep_stays_under_the_recorded_error(tmp_path):
    exe = str(tmp_path / "shape_sweep")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", os.path.join(ROOT, "tools", "shape_sweep.cpp"),
                           "-o", exe])
    out = subprocess.run([exe, "4099"], capture_output=True, text=True, check=True).stdout
    got = {m[0]: (float(m[1]), float(m[2])) for m in re.findall(r"(\w+) max_ulp=([\d.]+) at=\S+ max_rel_u=([\d.]+)", out)}
    assert set(got) == {"tanh", "cubic"}, out
    for name, (ulp, rel) in got.items():
        assert 0 < ulp <= rel <= R.E_SHAPE_F32[name], (name, ulp, rel)


def test_each_doubling_of_the_oversampling_lowers_the_alias_share_by_8_db():
    T = 32768
    x = 0.9 * np.sin(2 * np.pi * 4004 * np.arange(T) / T)
    win = np.blackman(T)
    keep = np.ones(T // 2 + 1, bool)
    for k in range(5):                                               # DC and the harmonics below Nyquist, +- 4 bins
        keep[max(0, k * 4004 - 4):k * 4004 + 5] = False
    share = []
    for L in (1, 2, 4, 8):
        y = waveshape(torch.from_numpy(x), "tanh", drive_db=24.0, oversample=L).numpy()
        p = np.abs(np.fft.rfft(y * win)) ** 2
        share.append(10 * np.log10(p[keep].sum() / p.sum()))
    print("alias share in dB at 1x, 2x, 4x, 8x:", [round(s, 1) for s in share])
    assert all(a - b >= 8.0 for a, b in zip(share, share[1:])), share
    assert share[0] < -10.0 and share[3] < -60.0
