"""The polyphase resampler (csrc/resample.hip) on the device against scipy.signal.resample_poly on the same samples.
Bars: TOL_CONV_F32 / TOL_CONV_F64 of max(1, max|ref|) (tests/gpu_common.py)."""
import math

import numpy as np
import pytest
import scipy.signal as ss
import torch

from tests.gpu_common import DEV, TOL_CONV_F32, TOL_CONV_F64, TOL_IIR_F32OUT, close, dev

pytestmark = pytest.mark.gpu

TABLE = [(160, 147), (147, 160), (1, 3), (3, 1), (1, 6), (441, 80), (160, 441), (997, 1000)]
EXTRA = [(1, 480), (480, 1), (3, 7)]
TOL = {np.float32: TOL_CONV_F32, np.float64: TOL_CONV_F64}


def rs():
    from torchfx_amd import resample_poly
    return resample_poly


def sig(shape, seed, dtype):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(dtype)


def lp(up, down):
    from torchfx_amd import torchfx_ext
    return torchfx_ext.resample_plan_info(4099, up, down, 2 * 10 * max(up, down) + 1)["Lp"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("up,down", TABLE + EXTRA)
def test_rate_grid(up, down, dtype):
    for T in sorted({0, 1, 7, lp(up, down), 4099, 65539}):
        for shape in [(T,), (3, T), (2, 2, T)]:
            x = sig(shape, T + len(shape), dtype)
            y = rs()(dev(x), up, down)
            assert y.dtype == dev(x).dtype and y.is_cuda
            close(y, ss.resample_poly(x, up, down, axis=-1).astype(dtype), TOL[dtype], f"{up}/{down} {shape} {dtype.__name__}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 10, 31, 64, 301, 4000])
def test_custom_windows(dtype, n):
    w = np.random.default_rng(n).uniform(-1, 1, n)
    w /= np.abs(w).sum()                              # |y| <= up * max|x|
    x = sig((3, 20000), n, dtype)
    for up, down in [(3, 2), (2, 3), (1, 5), (160, 147)]:
        ref = ss.resample_poly(x, up, down, axis=-1, window=w)
        close(rs()(dev(x), up, down, window=w), ref, TOL[dtype], f"window {n} {up}/{down}")


def test_window_specs():
    x = sig((2, 30000), 5, np.float32)
    for win in ["hann", ("kaiser", 8.0), "boxcar"]:
        close(rs()(dev(x), 2, 3, window=win), ss.resample_poly(x, 2, 3, axis=-1, window=win), TOL_CONV_F32, str(win))


def test_equal_rates_copy():
    x = dev(sig((2, 1000), 6, np.float32))
    y = rs()(x, 44100, 44100)
    assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strided_input(dtype):
    base = dev(sig((4, 3, 10007), 7, dtype))
    for view in [base[:, 1, :], base[::2, :, 5:9000], base.transpose(0, 1)]:
        got = rs()(view, 160, 147)
        assert torch.equal(got, rs()(view.contiguous(), 160, 147))
        close(got, ss.resample_poly(view.cpu().numpy(), 160, 147, axis=-1), TOL[dtype], "strided")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("up,down", [(160, 147), (1, 3), (3, 1), (1, 6), (1, 480)])
def test_non_finite_samples(up, down, dtype):
    T = 20011
    x = sig((4, T), 8, dtype)
    x[1, 0], x[1, T // 2], x[1, T - 1] = np.nan, np.inf, -np.inf
    x[2, 3], x[2, T // 3], x[2, T - 5] = np.inf, np.nan, np.nan
    ref = ss.resample_poly(x, up, down, axis=-1)
    got = rs()(dev(x), up, down).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.isfinite(got[[0, 3]]).all()
    ok = np.isfinite(ref)
    close(got[ok], ref[ok], TOL[dtype], "finite part")


def test_64bit_indexing():
    """One 28.8 M-sample row at 48k -> 44.1k: (m + n_pre_remove) * down passes 2^31 for the last outputs."""
    T = 28_800_000
    x = sig((1, T), 9, np.float32)
    y = rs()(dev(x), 147, 160)
    assert y.shape == (1, math.ceil(T * 147 / 160))
    assert (y.shape[-1] + 11) * 160 > 2 ** 31
    close(y, ss.resample_poly(x, 147, 160, axis=-1), TOL_CONV_F32, "28.8 M samples")


@pytest.mark.parametrize("up,down", [(997, 1000), (441, 80)])
def test_large_tables_f64(up, down):
    x = sig((2, 50000), 10, np.float64)
    close(rs()(dev(x), up, down), ss.resample_poly(x, up, down, axis=-1), TOL_CONV_F64, f"{up}/{down}")


def test_deterministic():
    x = dev(sig((8, 100003), 11, np.float32))
    for up, down in [(160, 147), (1, 3), (1, 6)]:
        assert torch.equal(rs()(x, up, down), rs()(x, up, down))


def test_graph_capture():
    x = dev(sig((4, 48000), 12, np.float32))
    static_in = x.clone()
    ref_out = rs()(static_in, 160, 147)              # warm: the polyphase table is cached
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            static_out = rs()(static_in, 160, 147)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, ref_out)
    new = dev(sig((4, 48000), 13, np.float32))
    static_in.copy_(new)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, rs()(new, 160, 147))


def test_device_pipeline_matches_cpu():
    from torchfx_amd import Resample, Wave
    from torchfx_amd.filter import HiButterworth, LoButterworth
    x = sig((2, 44100), 14, np.float32)
    w = Wave(torch.from_numpy(x), 44100, device=DEV) | LoButterworth(8000) | Resample(48000) | HiButterworth(100)
    assert w.fs == 48000
    got = w.ys
    # the same steps with the CPU resampler in the middle (the IIR steps have no CPU path here: they run on the device)
    lo = LoButterworth(8000, fs=44100)
    hi = HiButterworth(100, fs=48000)
    a = lo(dev(x)).cpu().numpy()
    b = ss.resample_poly(a, 160, 147, axis=-1).astype(np.float32)
    ref = hi(dev(b)).cpu().numpy()
    close(got, ref, TOL_CONV_F32 + TOL_IIR_F32OUT * 100, "pipeline")
    assert Wave(torch.from_numpy(x), 44100, device=DEV).resample(48000).ys.shape[-1] == 48000
    lines = (Wave(torch.from_numpy(x), 44100, device=DEV) | Resample(48000)).explain()
    assert lines == ["Resample: native (resample_reg_kernel)"]


def test_merge_after_device_resample():
    from torchfx_amd import Wave
    a = Wave(torch.from_numpy(sig((2, 44100), 15, np.float32)), 44100, device=DEV).resample(48000)
    b = Wave(torch.from_numpy(sig((2, 48000), 16, np.float32)), 48000, device=DEV)
    ya, yb = a.ys.cpu(), b.ys.cpu()
    m = Wave.merge([a, b])
    assert m.fs == 48000 and m.ys.shape == (2, 48000)
    assert torch.equal(m.ys.cpu(), ya + yb)
