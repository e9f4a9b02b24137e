"""Polyphase resampling without a GPU: resample_poly on CPU tensors against scipy.signal.resample_poly, the C side's
geometry (tfx_resample_plan_info) against SciPy's arithmetic, the op's Meta shape and CPU refusal, argument checks, and the
Wave / planner / streaming treatment of a Resample."""
import ctypes
import math

import numpy as np
import pytest
import scipy.signal as ss
import torch

# (up, down) of the typical geometries: 44.1k<->48k, 48k->16k, 16k->48k, 48k->8k, 8k->44.1k, 44.1k->16k, 1000->997
TABLE = [(160, 147), (147, 160), (1, 3), (3, 1), (1, 6), (441, 80), (160, 441), (997, 1000)]
NP = {torch.float32: np.float32, torch.float64: np.float64}


def rnd(shape, seed, dtype):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape)).to(dtype)


def scipy_ref(x, up, down, **kw):
    return ss.resample_poly(x.numpy(), up, down, axis=-1, **kw).astype(NP[x.dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(1000,), (3, 1000), (2, 2, 777)])
@pytest.mark.parametrize("up,down", [(160, 147), (1, 3), (3, 1), (3, 7)])
def test_cpu_matches_scipy_bit_for_bit(dtype, shape, up, down):
    from torchfx_amd import resample_poly
    x = rnd(shape, 1, dtype)
    y = resample_poly(x, up, down)
    ref = scipy_ref(x, up, down)
    assert y.dtype == dtype and tuple(y.shape) == ref.shape
    assert np.array_equal(y.numpy(), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [31, 40, 1])
def test_cpu_custom_window_arrays(dtype, n):
    from torchfx_amd import resample_poly
    w = np.random.default_rng(n).standard_normal(n)
    x = rnd((2, 500), 2, dtype)
    y = resample_poly(x, 3, 2, window=w)
    assert y.dtype == dtype
    assert np.array_equal(y.numpy(), scipy_ref(x, 3, 2, window=w))
    assert np.array_equal(resample_poly(x, 3, 2, window=list(w)).numpy(), y.numpy())


def test_cpu_window_spec():
    from torchfx_amd import resample_poly
    x = rnd((2, 900), 3, torch.float32)
    assert np.array_equal(resample_poly(x, 2, 3, window="hann").numpy(), scipy_ref(x, 2, 3, window="hann"))
    assert np.array_equal(resample_poly(x, 2, 3, window=("kaiser", 8.0)).numpy(), scipy_ref(x, 2, 3, window=("kaiser", 8.0)))


@pytest.mark.parametrize("up,down", [(1, 1), (5, 5), (44100, 44100)])
def test_equal_rates_copy(up, down):
    from torchfx_amd import resample_poly
    x = rnd((2, 300), 4, torch.float32)
    y = resample_poly(x, up, down)
    assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()


def test_gcd_reduction():
    from torchfx_amd import resample_poly
    x = rnd((1, 600), 5, torch.float64)
    assert torch.equal(resample_poly(x, 320, 294), resample_poly(x, 160, 147))


@pytest.mark.parametrize("up,down", [(160, 147), (1, 3), (3, 1), (1, 6)])
def test_n_out_for_short_rows(up, down):
    from torchfx_amd import resample_poly, torchfx_ext
    nh = 2 * 10 * max(up, down) + 1
    Lp = torchfx_ext.resample_plan_info(4099, up, down, nh)["Lp"]
    for T in (0, 1, Lp - 1, Lp, 4099):
        x = rnd((2, T), 6, torch.float32)
        y = resample_poly(x, up, down)
        assert y.shape == (2, math.ceil(T * up / down)) == scipy_ref(x, up, down).shape


def test_argument_errors():
    from torchfx_amd import Resample, resample_poly
    x = rnd((1, 100), 7, torch.float32)
    for up, down in [(0, 1), (1, 0), (-2, 3), (1.5, 2), (True, 2)]:
        with pytest.raises(ValueError):
            resample_poly(x, up, down)
    for dt in (torch.float16, torch.int32, torch.complex64):
        with pytest.raises(TypeError):
            resample_poly(x.to(dt), 2, 3)
    for pad in ("mean", "line", "reflect"):
        with pytest.raises(ValueError, match="constant"):
            resample_poly(x, 2, 3, padtype=pad)
    with pytest.raises(ValueError, match="cval"):
        resample_poly(x, 2, 3, cval=1.0)
    assert torch.equal(resample_poly(x, 2, 3, cval=0), resample_poly(x, 2, 3))
    with pytest.raises(ValueError):
        resample_poly(x, 2, 3, window=np.ones((3, 3)))
    for bad in (0, -16000, 16000.5, "16000"):
        with pytest.raises(ValueError):
            Resample(bad)
    with pytest.raises(ValueError):
        Resample(16000, fs=0)


def _scipy_geometry(T, up, down, nh):
    half = (nh - 1) // 2
    pre = down - half % down
    rem = (half + pre) // down
    n_out = T * up
    n_out = n_out // down + bool(n_out % down)
    post = 0
    while (((T - 1) * up + nh + pre + post) - 1) // down + 1 < n_out + rem:     # scipy's _output_len loop
        post += 1
    return n_out, rem, nh + pre + post


@pytest.mark.parametrize("up,down", TABLE + [(1, 480), (480, 1), (3, 7)])
@pytest.mark.parametrize("T", [0, 1, 20, 4099, 2646000])
def test_plan_info_matches_scipy(up, down, T):
    from torchfx_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    _lib.load()
    nh = 2 * 10 * max(up, down) + 1
    o = [ctypes.c_int64() for _ in range(4)]
    k, lds = ctypes.c_int(), ctypes.c_int64()
    rc = lib.tfx_resample_plan_info(ctypes.c_int64(T), ctypes.c_int64(up), ctypes.c_int64(down), ctypes.c_int64(nh), 0,
                                    *[ctypes.byref(v) for v in o], ctypes.byref(k), ctypes.byref(lds))
    assert rc == 0
    n_out, rem, padded = _scipy_geometry(T, up, down, nh)
    assert (o[0].value, o[1].value, o[2].value) == (n_out, rem, padded)
    assert o[3].value == -(-padded // up)
    assert k.value in (0, 1, 2) and 0 <= lds.value <= 49152


@pytest.mark.parametrize("n", [10, 11, 1, 301])
def test_plan_info_custom_lengths(n):
    from torchfx_amd import torchfx_ext
    for T in (0, 5, 1000):
        info = torchfx_ext.resample_plan_info(T, 3, 2, n)
        assert (info["n_out"], info["n_pre_remove"], info["padded"]) == _scipy_geometry(T, 3, 2, n)


def test_plan_info_table_kernels():
    from torchfx_amd import torchfx_ext
    info = {(u, d): torchfx_ext.resample_plan_info(2646000, u, d, 2 * 10 * max(u, d) + 1) for u, d in TABLE}
    assert info[(160, 147)]["kernel"] == "resample_reg_kernel" and info[(160, 147)]["Lp"] == 21
    assert info[(1, 6)]["kernel"] == "resample_lds_kernel" and info[(1, 6)]["Lp"] == 127
    assert torchfx_ext.resample_plan_info(1000, 1, 480, 9601)["kernel"] == "resample_lds_kernel"
    assert torchfx_ext.resample_plan_info(1000, 1, 8000, 160001)["kernel"] == "resample_gather_kernel"
    assert torchfx_ext.resample_plan_info(1000, 7, 7, 1)["kernel"] == "copy"


def test_capi_checks_arguments_before_the_device():
    from torchfx_amd import _lib
    lib = _lib.load()
    h = (ctypes.c_float * 5)()
    dummy = ctypes.c_void_p(16)
    for args in [(dummy, dummy, 7, 1, 10, 2, 3, h, 5), (dummy, dummy, 0, 1, 10, 0, 3, h, 5), (dummy, dummy, 0, 1, 10, 2, 3, None, 5),
                 (dummy, dummy, 0, 1, 10, 2, 3, h, 0), (None, dummy, 0, 1, 10, 2, 3, h, 5), (dummy, dummy, 0, -1, 10, 2, 3, h, 5)]:
        assert lib.tfx_resample_forward(*args, None) != 0
    out = ctypes.c_int64()
    assert lib.tfx_resample_plan_info(10, 0, 3, 5, 0, *[ctypes.byref(out)] * 4, ctypes.byref(ctypes.c_int()), ctypes.byref(out)) != 0


def test_meta_shape_and_no_cpu_path():
    from torchfx_amd import native
    native.load()
    x = torch.empty(5, 4410, device="meta")
    h = torch.ones(3201)
    y = torch.ops.torchfx_hip.resample_forward(x, 160, 147, h)
    assert tuple(y.shape) == (5, math.ceil(4410 * 160 / 147)) and y.device.type == "meta"
    y3 = torch.ops.torchfx_hip.resample_forward(torch.empty(2, 3, 100, device="meta"), 1, 3, h)
    assert tuple(y3.shape) == (2, 3, 34)
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.torchfx_hip.resample_forward(torch.zeros(2, 100), 160, 147, h)


def test_design_taps_match_scipy():
    from scipy.signal import firwin

    from torchfx_amd.resample import design_taps
    for up, down in [(160, 147), (1, 3), (3, 1)]:
        m = max(up, down)
        for dt in (torch.float32, torch.float64):
            h = firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)).astype(NP[dt])
            h *= up
            assert np.array_equal(design_taps(up, down, ("kaiser", 5.0), dt).numpy(), h)


# ---- Resample and Wave ---------------------------------------------------------------------------------------------------
def test_resample_effect_rates():
    from torchfx_amd import Resample
    r = Resample(48000, fs=44100)
    assert (r.up, r.down) == (160, 147)
    x = rnd((2, 4410), 8, torch.float32)
    assert np.array_equal(r(x).numpy(), scipy_ref(x, 160, 147))
    with pytest.raises(AssertionError):
        Resample(16000).up


def test_wave_pipe_sets_rate():
    from torchfx_amd import Resample, Wave
    w = Wave(rnd((2, 4410), 9, torch.float32), 44100)
    r = w | Resample(16000)
    assert r.fs == 16000 and w.fs == 44100
    assert np.array_equal(r.ys.numpy(), scipy_ref(w.ys, 160, 441))


def test_filters_after_resample_design_at_new_rate():
    from torchfx_amd import Resample, Wave
    from torchfx_amd.filter import LoButterworth
    w = Wave(rnd((2, 4410), 10, torch.float32), 44100)
    ref = LoButterworth(1000, fs=16000)
    ref.compute_coefficients()
    lo = LoButterworth(1000)
    out = w | Resample(16000) | lo
    assert lo.fs == 16000 and torch.equal(lo._sos, ref._sos)
    lo2, r2 = LoButterworth(1000), Resample(16000)
    before = LoButterworth(1000)
    out2 = w | (before | r2 | lo2)
    assert before.fs == 44100 and r2.fs == 44100 and lo2.fs == 16000 and torch.equal(lo2._sos, ref._sos)
    assert out2.fs == 16000 and out.fs == 16000


def test_wave_resample_method_equals_pipe():
    from torchfx_amd import Resample, Wave
    w = Wave(rnd((2, 3000), 11, torch.float64), 48000)
    a = w.resample(44100)
    b = w | Resample(44100)
    assert a.fs == b.fs == 44100 and torch.equal(a.ys, b.ys)
    c = w.resample(44100, window="hann")
    assert np.array_equal(c.ys.numpy(), scipy_ref(w.ys, 147, 160, window="hann"))


def test_plans_differ_by_new_fs():
    from torchfx_amd import Resample, Wave
    x = rnd((1, 4000), 12, torch.float32)
    r = Resample(16000)
    a = (Wave(x, 48000) | r).ys
    r.new_fs = 24000
    b = (Wave(x, 48000) | r).ys
    assert a.shape[-1] == 1334 and b.shape[-1] == 2000
    assert np.array_equal(b.numpy(), scipy_ref(x, 1, 2))


def test_planner_barrier():
    from torchfx_amd import Gain, Resample, Wave
    from torchfx_amd.effect import Epilogued
    from torchfx_amd.filter import FIR, LoButterworth
    w = Wave(rnd((1, 4000), 13, torch.float32), 48000)
    w.fuse_fir = w.fuse_gain = w.fuse_epilogue = True
    f1, f2 = FIR(np.hanning(33) / 16), FIR(np.hanning(17) / 8)
    p = (w | f1 | Resample(16000) | f2).plan()
    assert [type(m).__name__ for m in p] == ["FIR", "Resample", "FIR"]
    p = (w | LoButterworth(1000) | Resample(16000) | Gain(0.5)).plan()
    assert not any(isinstance(m, Epilogued) for m in p) and any(isinstance(m, Resample) for m in p)
    lines = (w | Resample(16000)).explain()
    assert lines == ["Resample: scipy on host -- cpu tensor"]


def test_merge_after_resample():
    from torchfx_amd import Wave
    a = Wave(rnd((2, 4410), 15, torch.float32), 44100).resample(48000)
    b = Wave(rnd((2, 4800), 16, torch.float32), 48000)
    m = Wave.merge([a, b])
    assert m.fs == 48000 and m.ys.shape == (2, 4800)
    with pytest.raises(ValueError, match="mismatch"):
        Wave.merge([Wave(rnd((2, 10), 17, torch.float32), 44100), b])


def test_stream_processor_refuses_resample():
    from torchfx_amd import FilterChain, Gain, Resample
    from torchfx_amd.realtime import StreamProcessor
    with pytest.raises(TypeError, match="Resample"):
        StreamProcessor([Gain(0.5), Resample(16000)], device="cpu")
    with pytest.raises(TypeError, match="Resample"):
        StreamProcessor(FilterChain(Gain(0.5), Resample(16000)), device="cpu")


def test_top_level_exports():
    import torchfx_amd
    assert "Resample" in torchfx_amd.__all__ and "resample_poly" in torchfx_amd.__all__
    assert torchfx_amd.Resample.__module__ == "torchfx_amd.resample"
