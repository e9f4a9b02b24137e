"""Zero-phase filtering on the device (csrc/sos.hip, the FF passes) against scipy.signal.sosfiltfilt in float64 on
float64(x) -- never against the code under test.  Bars: the project's IIR ones, TOL_IIR_F32OUT (1.5e-7 x scale) for float32
signals and TOL_IIR_F64OUT (2e-11 x scale) for float64 signals (tests/gpu_common.py)."""
import json

import numpy as np
import pytest
import scipy.signal as ss
import torch

from tests.gpu_common import DEV, TOL_IIR_F32OUT, TOL_IIR_F64OUT, allpass_sos, close, dev, rnd

pytestmark = pytest.mark.gpu

FS = 48000
TOL = {np.float32: TOL_IIR_F32OUT, np.float64: TOL_IIR_F64OUT}
PADTYPES = ["odd", "even", "constant", None]


def fx():
    import torchfx_amd
    return torchfx_amd


def filters():
    from torchfx_amd import filter as F
    return {
        "butter4_lp1k": F.LoButterworth(1000, order=4, fs=FS),
        "hi_butter20": F.HiButterworth(20, fs=FS),
        "hi_cheby20": F.HiChebyshev1(20, fs=FS),
        "lo_butter40_o8": F.LoButterworth(40, order=8, fs=FS),
        "ellip12_lp1k": F.LoElliptic(1000, order=12, fs=FS),
        "notch60_q30": F.Notch(60, q=30, fs=FS),
        "biquad_lpf": F.BiquadLPF(cutoff=2000, q=0.707, fs=FS),
    }


GRID = list(filters())
HARD = ["hi_butter20", "hi_cheby20", "lo_butter40_o8", "ellip12_lp1k", "notch60_q30"]          # long memory: poles next to z = 1


def sos_of(name):
    f = filters()[name]
    if f._sos is None:
        f.compute_coefficients()
    return np.ascontiguousarray(f._sos.detach().cpu().numpy(), dtype=np.float64)


def sig(shape, seed, dtype):
    x = np.random.default_rng(seed).uniform(-1, 1, shape)
    return (x / np.abs(x).max()).astype(dtype)


def ref(sos, x, **kw):
    return ss.sosfiltfilt(sos, x.astype(np.float64), axis=-1, **kw)


def check(name, x, what, **kw):
    sos = sos_of(name) if isinstance(name, str) else name          # a filter of the grid, or the coefficients themselves
    y = fx().sosfiltfilt(dev(x), sos, **kw)
    assert y.is_cuda and y.shape == x.shape and y.dtype == dev(x).dtype
    exp = ref(sos, x, **kw)
    got = y.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - exp).max())
    print(f"{what}: max err {err:.3e} (scale {max(1.0, float(np.abs(exp).max())):.3g}, bar {TOL[x.dtype.type]:.1e})")
    close(y, exp, TOL[x.dtype.type], what)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", GRID)
def test_filter_grid_shapes_and_lengths(name, dtype):
    from torchfx_amd.filtfilt import default_padlen
    pad = default_padlen(sos_of(name))
    for T in (pad + 1, 4097, 100_003):
        for shape in [(T,), (3, T), (2, 2, T)]:
            check(name, sig(shape, T + len(shape), dtype), f"{name} {shape} {dtype.__name__}")


@pytest.mark.parametrize("name", HARD)
def test_long_rows_take_several_segments_in_both_passes(name):
    from torchfx_amd import torchfx_ext
    C, T = 4, 3_000_000
    if name == "notch60_q30":
        # its warm-up is 387 028 samples, and the planner does not cut rows into segments shorter than eight warm-ups: it runs
        # 3 000 000 samples as one segment.  8 000 000 samples are the row its own plan cuts (into three).
        T = 8_000_000
    info = torchfx_ext.sos_filtfilt_plan_info(sos_of(name), C, T)
    assert info["nseg_forward"] > 1 and info["nseg_reverse"] > 1, info
    check(name, sig((C, T), 21, np.float32), f"{name} 4 x {T} float32 ({info['nseg_forward']} + {info['nseg_reverse']} segments)")


@pytest.mark.parametrize("name,T", [("butter4_lp1k", 1_000_000), ("hi_butter20", 2_000_000), ("hi_cheby20", 3_000_000),
                                    ("notch60_q30", 8_000_000)])
def test_long_rows_float64(name, T):
    """Float64 signals, several segments per row in both passes, at 2e-11: the rough-output filters with poles next to z = 1
    are the ones the refined start states exist for."""
    from torchfx_amd import torchfx_ext
    C = 2 if T > 4_000_000 else 4
    info = torchfx_ext.sos_filtfilt_plan_info(sos_of(name), C, T)
    assert info["nseg_forward"] > 1 and info["nseg_reverse"] > 1, info
    check(name, sig((C, T), 22, np.float64), f"{name} {C} x {T} float64 ({info['nseg_reverse']} segments)")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dc_offset_pins_the_start_states(dtype):
    """0.8 + 0.01 noise through an 8th-order 40 Hz low-pass: passes started from zero state are off by ~0.8 at the edges."""
    for shape in [(2, 20_000), (4, 600_000)]:
        x = (0.8 + 0.01 * np.random.default_rng(3).standard_normal(shape)).astype(dtype)
        check("lo_butter40_o8", x, f"dc offset {shape} {dtype.__name__}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_long_cascade_leaves_room_for_one_workgroup_per_cu(dtype):
    """100 all-pass sections: from 81 sections on the carry takes so much LDS that one workgroup fits a CU instead of two,
    and the segment plan and the launch both count on one."""
    from torchfx_amd import torchfx_ext
    sos = allpass_sos(100)
    info = torchfx_ext.sos_filtfilt_plan_info(sos, 2, 20_000)
    assert info["warmup"] == -1 and info["nseg_forward"] == info["nseg_reverse"] == 1, info
    check(sos, rnd((2, 20_000), 9, dtype), f"100 all-pass sections {dtype.__name__}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("padtype", PADTYPES)
def test_padtypes_and_explicit_padlen(padtype, dtype):
    from torchfx_amd.filtfilt import default_padlen
    for name in ("butter4_lp1k", "hi_cheby20"):
        big = default_padlen(sos_of(name)) + 500
        x = sig((3, 30_011), 5, dtype) + dtype(0.25)
        check(name, x, f"{name} padtype {padtype}", padtype=padtype)
        check(name, x, f"{name} padtype {padtype} padlen 0", padtype=padtype, padlen=0)
        check(name, x, f"{name} padtype {padtype} padlen {big}", padtype=padtype, padlen=big)
        check(name, x[:, :big + 1], f"{name} padtype {padtype} T = padlen + 1", padtype=padtype, padlen=big)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [8_000, 2_000_000])
def test_non_finite_rows(T, dtype):
    """A NaN anywhere makes its row all NaN (SciPy's result), an Inf makes its row all non-finite, other rows are untouched --
    at one segment per row and at several."""
    from torchfx_amd import torchfx_ext
    for name in ("butter4_lp1k", "hi_butter20"):
        sos = sos_of(name)
        nseg = torchfx_ext.sos_filtfilt_plan_info(sos, 3, T)["nseg_reverse"]
        assert (nseg > 1) == (T > 1_000_000), nseg
        x = sig((3, T), 9, dtype)
        x[0, T // 2] = np.nan
        x[1, T // 3] = np.inf
        y = fx().sosfiltfilt(dev(x), sos).cpu().numpy()
        assert np.isnan(y[0]).all(), f"{name} T={T}: {np.isfinite(y[0]).sum()} finite samples in the NaN row"
        assert (~np.isfinite(y[1])).all(), f"{name} T={T}: {np.isfinite(y[1]).sum()} finite samples in the Inf row"
        close(y[2], ref(sos, x[2]), TOL[dtype], f"{name} T={T} clean row")
        # near the edges too: the first and the last sample
        for pos in (0, T - 1):
            x2 = sig((2, T), 10, dtype)
            x2[0, pos] = np.nan
            y2 = fx().sosfiltfilt(dev(x2), sos).cpu().numpy()
            assert np.isnan(y2[0]).all(), f"{name} T={T}: NaN at {pos}"
            close(y2[1], ref(sos, x2[1]), TOL[dtype], f"{name} T={T} clean row (NaN at {pos} next door)")


def test_memory_is_the_result_plus_one_float64_intermediate():
    from torchfx_amd.filtfilt import default_padlen
    C, T = 16, 2_880_000
    sos = sos_of("butter4_lp1k")
    pad = default_padlen(sos)
    x = dev(sig((C, T), 12, np.float32))
    fx().sosfiltfilt(x[:, :10_000], sos)                   # tables, module load
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = fx().sosfiltfilt(x, sos)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    bound = y.numel() * 4 + 8 * C * (T + 2 * pad) + (16 << 20)
    print(f"peak rise {rise} B, bound {bound} B")
    assert rise <= bound, (rise, bound)
    assert torch.cuda.memory_allocated() - before <= y.numel() * 4 + (16 << 20)      # the intermediate is gone after the call


def test_launches_of_one_call():
    from torchfx_amd import _lib
    lib = _lib.load()
    sos = sos_of("hi_butter20")
    for shape in [(4, 20_000), (4, 3_000_000)]:
        x = dev(sig(shape, 13, np.float32))
        fx().sosfiltfilt(x, sos)
        torch.cuda.synchronize()
        lib.tfx_prof_enable(1)
        lib.tfx_prof_collect()
        fx().sosfiltfilt(x, sos)
        prof = json.loads(lib.tfx_prof_collect().decode())
        lib.tfx_prof_enable(0)
        calls = {k: v["calls"] for k, v in prof.items()}
        print(shape, calls)
        assert set(calls) <= {"sos_filtfilt_forward_kernel", "sos_filtfilt_reverse_kernel", "sos_nonfinite_fix_kernel",
                              "sos_stream_kernel<f64>"}, calls
        assert calls["sos_filtfilt_forward_kernel"] == 1 and calls["sos_filtfilt_reverse_kernel"] == 1, calls
        assert calls.get("sos_nonfinite_fix_kernel", 0) <= 2 and calls.get("sos_stream_kernel<f64>", 0) == 0, calls   # once per pass at most


def test_other_device_dtypes_and_short_rows_are_errors():
    sos = sos_of("butter4_lp1k")
    with pytest.raises(TypeError):
        fx().sosfiltfilt(torch.zeros(2, 1000, dtype=torch.float16, device=DEV), sos)
    with pytest.raises(ValueError, match="greater than padlen, which is 15"):
        fx().sosfiltfilt(torch.zeros(2, 15, device=DEV), sos)
    with pytest.raises(np.linalg.LinAlgError):
        fx().sosfiltfilt(torch.zeros(2, 1000, device=DEV), np.array([[1.0, 0, 0, 1, -1.0, 0]]))
    y = fx().sosfiltfilt(torch.zeros(0, 1000, device=DEV), sos)
    assert y.shape == (0, 1000)


def test_strided_input():
    sos = sos_of("butter4_lp1k")
    base = dev(sig((4, 3, 10_007), 14, np.float32))
    for view in [base[:, 1, :], base[::2, :, 5:9000], base.transpose(0, 1)]:
        close(fx().sosfiltfilt(view, sos), ref(sos, view.cpu().numpy()), TOL_IIR_F32OUT, "strided")


def test_zero_phase_in_a_wave_equals_the_steps():
    from torchfx_amd import Gain, Wave
    from torchfx_amd import filter as F
    x = sig((2, 200_000), 15, np.float32)
    lp, zp, g = F.LoButterworth(4000, order=4), F.ZeroPhase(F.HiButterworth(80, order=2), F.Notch(60, q=30)), Gain(0.5)
    w = Wave(dev(x), FS, device=DEV) | lp | zp | g
    lines = w.explain()
    assert any("ZeroPhase: native (sos_filtfilt_forward_kernel + sos_filtfilt_reverse_kernel" in ln for ln in lines), lines
    y = w.ys
    step = F.LoButterworth(4000, order=4, fs=FS)(dev(x))                                    # the device's own forward cascade
    sos = np.vstack([sos_of_module(F.HiButterworth(80, order=2, fs=FS)), sos_of_module(F.Notch(60, q=30, fs=FS))])
    exp = (ref(sos, step.cpu().numpy()).astype(np.float32) * np.float32(0.5))
    close(y, exp, TOL_IIR_F32OUT, "wave | lp | ZeroPhase | gain")
    assert zp.filters[0]._state_x is None and lp.fs == FS


def sos_of_module(f):
    if f._sos is None:
        f.compute_coefficients()
    return f._sos.detach().cpu().numpy().astype(np.float64)
