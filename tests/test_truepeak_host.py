"""True peak (ITU-R BS.1770-4 Annex 2) and loudness range (EBU Tech 3342) without a GPU: the CPU path of
torchfx_amd.loudness on the Tech 3341 / Tech 3342 test tones, shapes, silence, non-finite samples and argument errors,
LoudnessNormalize(max_true_peak=...), and the host-only half of the C ABI (tfx_true_peak_forward's checks,
tfx_true_peak_plan_info)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import truepeak_signals as S


def fx():
    import torchfx_amd
    return torchfx_amd


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- true peak: Tech 3341 tones -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [48000, 44100, 96000])
@pytest.mark.parametrize("div,phase", S.TONES)
def test_tech3341_tones_read_within_tolerance(fs, div, phase):
    err = float(fx().true_peak(t(S.tone(div, phase)), fs)) - 20.0 * math.log10(0.5)
    print(f"fs {fs} fs/{div} {phase} deg: {err:+.4f} dB")
    assert -S.TP_TOL_BELOW <= err <= S.TP_TOL_ABOVE


def test_tone_above_full_scale_reads_within_tolerance():
    err = float(fx().true_peak(t(S.tone(4, 45.0, amp=1.41)), 48000)) - 20.0 * math.log10(1.41)
    print(f"1.41: {err:+.4f} dB")
    assert -S.TP_TOL_BELOW <= err <= S.TP_TOL_ABOVE


def test_an_abrupt_onset_really_overshoots():
    """The same fs/8 tone without fades reads above the tolerance: the overshoot of the band-limited onset is signal, not an
    error of the meter.  (Which is why the conformance tones are faded.)"""
    err = float(fx().true_peak(t(S.tone(8, 67.5, fade=0)), 48000)) - 20.0 * math.log10(0.5)
    print(f"unfaded: {err:+.4f} dB")
    assert err > S.TP_TOL_ABOVE


def test_sample_peak_misses_three_db_and_oversampling_follows_the_rate():
    L = fx()
    x = t(S.tone(4, 45.0))
    assert abs(float(L.true_peak(x, 48000, oversample=1)) - (-9.03)) <= 0.005       # 0.5 sin(45 deg) = 0.35355
    assert abs(float(L.true_peak(x, 48000)) - (-6.0)) <= 0.02
    assert torch.equal(L.true_peak(x, 192000), L.true_peak(x, 48000, oversample=1))  # from 192 kHz: the sample peak
    assert torch.equal(L.true_peak_linear(x, 192000), x.abs().amax())
    assert torch.equal(L.true_peak(x, 96000), L.true_peak(x, 48000, oversample=2))
    assert torch.equal(L.true_peak(x, 95999), L.true_peak(x, 48000, oversample=4))
    assert torch.equal(L.true_peak(x, 191999), L.true_peak(x, 48000, oversample=2))
    from scipy.signal import resample_poly
    for up in (2, 4, 8):
        ref = np.abs(resample_poly(x.numpy(), up, 1)).max()
        assert float(L.true_peak_linear(x, 48000, oversample=up)) == float(ref)


# ---- shapes, silence, non-finite samples, errors --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_shapes_dtypes_silence_and_nan(dtype):
    L = fx()
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(2, 3, 700, generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    for sig, shape in ((x[0, 0], ()), (x[0], (3,)), (x, (2, 3))):
        db, lin = L.true_peak(sig, 48000), L.true_peak_linear(sig, 48000)
        assert db.shape == shape and db.dtype == torch.float64
        assert lin.shape == shape and lin.dtype == dtype
        assert torch.equal(db, 20.0 * torch.log10(lin.to(torch.float64)))
    assert torch.equal(L.true_peak(x, 48000)[1], L.true_peak(x[1], 48000))
    assert torch.equal(L.true_peak(x, 48000)[1, 2], L.true_peak(x[1, 2], 48000))
    silent = L.true_peak(torch.zeros(2, 500, dtype=dtype), 48000)
    assert bool(torch.isneginf(silent).all())
    assert bool(torch.isneginf(L.true_peak(torch.zeros(2, 0, dtype=dtype), 48000)).all())
    assert torch.equal(L.true_peak_linear(torch.zeros(3, 0, dtype=dtype), 48000, oversample=1), torch.zeros(3, dtype=dtype))
    clean = L.true_peak(x[0], 48000)
    bad = x[0].clone()
    bad[1, 350] = math.nan
    got = L.true_peak(bad, 48000)
    assert bool(torch.isnan(got[1])) and torch.equal(got[[0, 2]], clean[[0, 2]])
    bad[1, 350] = math.inf
    got = L.true_peak(bad, 48000)
    assert not bool(torch.isfinite(got[1])) and not bool(torch.isneginf(got[1])) and torch.equal(got[[0, 2]], clean[[0, 2]])
    assert bool(torch.isnan(L.true_peak(torch.full((5,), math.nan, dtype=dtype), 192000)))


def test_argument_errors():
    L = fx()
    x = torch.zeros(2, 100)
    with pytest.raises(TypeError, match="torch.Tensor"):
        L.true_peak(np.zeros(10), 48000)
    with pytest.raises(ValueError, match=r"\[T\], \[C, T\], or \[B, C, T\]"):
        L.true_peak(torch.zeros(1, 1, 2, 100), 48000)
    with pytest.raises(ValueError, match=r"\[T\], \[C, T\], or \[B, C, T\]"):
        L.true_peak(torch.zeros(()), 48000)
    with pytest.raises(TypeError, match="float32 or float64"):
        L.true_peak(torch.zeros(2, 100, dtype=torch.int16), 48000)
    for fs in (7999, 48000.0, True):
        with pytest.raises(ValueError, match="fs must be an integer >= 8000"):
            L.true_peak(x, fs)
    for up in (0, 3, 16, 4.5, True, "4"):
        with pytest.raises(ValueError, match="oversample must be one of"):
            L.true_peak(x, 48000, oversample=up)
    with pytest.raises(ValueError, match="at most 64"):
        L.true_peak(x, 48000, taps=np.ones(257))
    with pytest.raises(ValueError, match="at most 64"):
        L.true_peak(x, 48000, oversample=2, taps=np.ones(129))
    with pytest.raises(ValueError, match="1-D"):
        L.true_peak(x, 48000, taps=np.ones((2, 8)))
    with pytest.raises(ValueError, match="1-D"):
        L.true_peak(x, 48000, taps=[])
    assert L.true_peak(x, 48000, taps=np.ones(256)).shape == (2,)


def test_the_callers_own_interpolator():
    L = fx()
    from torchfx_amd.resample import design_taps
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 999, generator=g) * 2 - 1
    assert torch.equal(L.true_peak(x, 48000, taps=design_taps(4, 1)), L.true_peak(x, 48000))
    assert torch.equal(L.true_peak(x, 48000, taps=design_taps(4, 1).numpy()), L.true_peak(x, 48000))
    assert torch.equal(L.true_peak(x, 96000, taps=design_taps(2, 1)), L.true_peak(x, 96000))
    # a filter that only repeats each sample (4 ones): the "oversampled" signal holds x's samples, so the sample peak comes back
    hold = L.true_peak_linear(x, 48000, taps=[1.0, 1.0, 1.0, 1.0])
    assert torch.equal(hold, x.abs().amax(-1))


# ---- loudness range: Tech 3342 tones --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit_lufs():
    """fs -> integrated loudness of 5 s of the stereo sine at amplitude 1 (the calibration of the Tech 3342 signals)."""
    return {fs: float(fx().integrated_loudness(t(S.stereo_sine(fs, S.LRA_TONE[fs], 5)), fs)) for fs in S.LRA_TONE}


def test_calibration_tones(unit_lufs):
    assert abs(unit_lufs[48000] - 0.007) <= 2e-3 and abs(unit_lufs[8000] - (-0.454)) <= 2e-3


@pytest.mark.parametrize("levels,seconds,expected", S.LRA_CASES)
def test_tech3342_tones_at_8k(unit_lufs, levels, seconds, expected):
    lra = fx().loudness_range(t(S.lra_signal(levels, seconds, 8000, unit_lufs[8000])), 8000)
    print(f"{levels} x {seconds} s: {float(lra):.4f} LU")
    assert lra.shape == () and lra.dtype == torch.float64
    assert abs(float(lra) - expected) <= S.LRA_TOL


def test_tech3342_first_tone_at_48k(unit_lufs):
    levels, seconds, expected = S.LRA_CASES[0]
    x = t(S.lra_signal(levels, seconds, 48000, unit_lufs[48000]).astype(np.float32))
    assert abs(float(fx().loudness_range(x, 48000)) - expected) <= S.LRA_TOL


def test_loudness_range_edges_and_batches(unit_lufs):
    L = fx()
    fs = 8000
    a = t(S.lra_signal((-20.0, -30.0), 8, fs, unit_lufs[fs]))
    b = t(S.lra_signal((-25.0, -20.0), 8, fs, unit_lufs[fs]))
    assert float(L.loudness_range(a[:, :3 * fs - 1], fs)) == 0.0                 # shorter than one 3 s window
    assert float(L.loudness_range(torch.zeros(2, 10 * fs), fs)) == 0.0           # nothing passes the absolute gate
    assert float(L.loudness_range(a[0, :fs], fs)) == 0.0
    batch = L.loudness_range(torch.stack([a, b]), fs)
    assert batch.shape == (2,) and batch.dtype == torch.float64
    assert torch.equal(batch[0], L.loudness_range(a, fs)) and torch.equal(batch[1], L.loudness_range(b, fs))
    assert L.loudness_range(torch.zeros(3, 2, fs), fs).tolist() == [0.0, 0.0, 0.0]
    mono = L.loudness_range(a[0], fs)
    assert mono.shape == () and abs(float(mono) - 10.0) <= S.LRA_TOL
    bad = a.clone()
    bad[0, 5 * fs] = math.nan
    assert bool(torch.isnan(L.loudness_range(bad, fs)))
    assert torch.isnan(L.loudness_range(torch.stack([bad, b]), fs)).tolist() == [True, False]
    with pytest.raises(ValueError, match="channel_weights"):
        L.loudness_range(a, fs, channel_weights=[1.0])


def test_percentiles_are_nearest_rank_with_halves_rounded_up():
    """Six short-term values 0.5 LU apart pass the gates: (n - 1) * 0.10 = 0.5 rounds UP to rank 1 (half-to-even would take
    rank 0) and (n - 1) * 0.95 = 4.75 to rank 5, so the range is 2.0 LU, not 2.5.  The values come in unsorted."""
    from unittest import mock

    L = fx()
    lj = -20.0 + 0.5 * np.array([3, 0, 5, 1, 4, 2])
    p = torch.from_numpy(10.0 ** ((lj + 0.691) / 10.0))
    with mock.patch("torchfx_amd.loudness._window_power", return_value=(p, 6)):
        assert abs(float(L.loudness_range(torch.zeros(2, 8), 8000)) - 2.0) <= 1e-9
    quiet = torch.cat([p, p[:1] * 1e-3])                               # a seventh value 30 LU down: out at the relative gate
    with mock.patch("torchfx_amd.loudness._window_power", return_value=(quiet, 7)):
        assert abs(float(L.loudness_range(torch.zeros(2, 8), 8000)) - 2.0) <= 1e-9


# ---- LoudnessNormalize with a true-peak ceiling ---------------------------------------------------------------------------
def test_loudness_normalize_with_a_true_peak_ceiling():
    L = fx()
    fs = 48000
    x = t(S.accent_tone())                                            # 2 s of the faded (4, 45 deg) tone with a 10 ms accent
    free = L.LoudnessNormalize(-14, fs=fs)(x)
    over = float(L.true_peak(free, fs).amax())
    print(f"loudness gain alone: {over:+.3f} dBTP")
    assert over > -1.0 + 1.0                                          # the loudness gain alone passes the ceiling
    y = L.LoudnessNormalize(-14, max_true_peak=-1.0, fs=fs)(x)
    got = float(L.true_peak(y, fs).amax())
    print(f"with the ceiling: {got:+.6f} dBTP")
    assert y.dtype == x.dtype and abs(got - (-1.0)) <= 1e-3
    assert float(L.integrated_loudness(y, fs)) < -14.0
    # stereo and batched: the programme peak is the largest channel's, one gain per batch item
    st = torch.stack([x, 0.5 * x])
    ys = L.LoudnessNormalize(-14, max_true_peak=-1.0, fs=fs)(st)
    assert abs(float(L.true_peak(ys, fs).amax()) - (-1.0)) <= 1e-3
    quiet_item = torch.stack([t(S.tone(4, 45.0, 0.05, 96000)), t(S.tone(4, 45.0, 0.02, 96000))])
    yb = L.LoudnessNormalize(-14, max_true_peak=-1.0, fs=fs)(torch.stack([st, quiet_item]))
    assert torch.equal(yb[0], ys) and torch.equal(yb[1], L.LoudnessNormalize(-14, fs=fs)(quiet_item))


def test_a_ceiling_that_does_not_bind_changes_nothing():
    L = fx()
    x = t(S.tone(4, 45.0, 0.05, 96000))                               # a steady tone lands at about -14.3 dBTP
    assert torch.equal(L.LoudnessNormalize(-14, max_true_peak=-1.0, fs=48000)(x), L.LoudnessNormalize(-14, fs=48000)(x))
    silent = torch.zeros(2, 48000)
    assert torch.equal(L.LoudnessNormalize(-14, max_true_peak=-1.0, fs=48000)(silent), silent)
    short = t(S.tone(4, 45.0, 0.9, 4800))                             # under 400 ms: loudness -inf, left alone
    assert torch.equal(L.LoudnessNormalize(-14, max_true_peak=-20.0, fs=48000)(short), short)
    with pytest.raises(ValueError, match="max_true_peak"):
        L.LoudnessNormalize(-14, max_true_peak=math.inf)
    assert "max_true_peak=-1.0" in repr(L.LoudnessNormalize(-14, max_true_peak=-1, fs=48000))
    assert "max_true_peak" not in repr(L.LoudnessNormalize(-14, fs=48000))
    assert L.LoudnessNormalize(-14, max_true_peak=-1.0, fs=48000).route(x).startswith("scipy on host")


def test_wave_methods():
    L = fx()
    x = t(np.stack([S.tone(4, 45.0, 0.5, 48000), S.tone(6, 60.0, 0.25, 48000)]))
    w = L.Wave(x, 48000)
    assert isinstance(w.true_peak(), float) and w.true_peak() == float(L.true_peak(x, 48000).amax(-1))
    assert w.true_peak(oversample=1) == float(L.true_peak(x, 48000, oversample=1).amax(-1))
    assert isinstance(w.loudness_range(), float) and w.loudness_range() == 0.0
    assert L.Wave(torch.zeros(2, 4800), 48000).true_peak() == -math.inf


# ---- C ABI, host only ----------------------------------------------------------------------------------------------------
def test_plan_info_runs_without_a_device():
    from torchfx_amd import torchfx_ext as E
    info = E.true_peak_plan_info(64, 2_880_000, 4, 81)
    assert info["Lp"] == 21 and info["tile_in"] >= 256
    assert info["tiles"] == -(-(2_880_000 + 1) // info["tile_in"]) and info["work_elems"] == 64 * info["tiles"]
    one = E.true_peak_plan_info(1, 2_880_000, 4, 81)
    assert (one["tiles"], one["tile_in"]) == (info["tiles"], info["tile_in"])        # the tiling does not depend on the rows
    assert E.true_peak_plan_info(3, 0, 4, 81)["work_elems"] == 0
    assert E.true_peak_plan_info(3, 7, 2, 41, torch.float64)["Lp"] == 21
    assert E.true_peak_plan_info(3, 7, 8, 161)["Lp"] == 21
    assert E.true_peak_plan_info(3, 7, 8, 512)["Lp"] == 65
    for rows, T, up, nh in ((1, 10, 3, 81), (1, 10, 1, 21), (1, 10, 16, 321), (1, 10, 4, 257), (1, 10, 4, 0), (-1, 10, 4, 81),
                            (1, -10, 4, 81)):
        with pytest.raises(RuntimeError, match="true_peak_forward"):
            E.true_peak_plan_info(rows, T, up, nh)


def test_bad_arguments_are_errors_not_crashes():
    from torchfx_amd import _lib
    lib = _lib.load()
    taps = (ctypes.c_float * 257)()
    buf = (ctypes.c_float * 64)()
    fwd, info = lib.tfx_true_peak_forward, lib.tfx_true_peak_plan_info
    o = [ctypes.c_int64() for _ in range(4)]
    refs = [ctypes.byref(v) for v in o]
    cases = {
        "null signal": fwd(None, 0, buf, 2, 10, 4, taps, 81, buf, None),
        "null result": fwd(buf, 0, None, 2, 10, 4, taps, 81, buf, None),
        "null work": fwd(buf, 0, buf, 2, 10, 4, taps, 81, None, None),
        "null taps": fwd(buf, 0, buf, 2, 10, 4, None, 81, buf, None),
        "no taps": fwd(buf, 0, buf, 2, 10, 4, taps, 0, buf, None),
        "negative rows": fwd(buf, 0, buf, -2, 10, 4, taps, 81, buf, None),
        "negative length": fwd(buf, 0, buf, 2, -10, 4, taps, 81, buf, None),
        "bad dtype": fwd(buf, 7, buf, 2, 10, 4, taps, 81, buf, None),
        "up 1": fwd(buf, 0, buf, 2, 10, 1, taps, 21, buf, None),
        "up 3": fwd(buf, 0, buf, 2, 10, 3, taps, 61, buf, None),
        "up 16": fwd(buf, 0, buf, 2, 10, 16, taps, 257, buf, None),
        "too many taps": fwd(buf, 0, buf, 2, 10, 4, taps, 257, buf, None),
        "too many taps for up 2": fwd(buf, 0, buf, 2, 10, 2, taps, 129, buf, None),
        "plan_info null output": info(2, 10, 4, 81, 0, None, refs[1], refs[2], refs[3]),
        "plan_info up": info(2, 10, 5, 81, 0, *refs),
    }
    assert all(rc != 0 for rc in cases.values()), cases
    for args in ((None, 0, buf, 2, 10, 4, taps, 81, buf, None), (buf, 0, buf, 2, 10, 3, taps, 81, buf, None),
                 (buf, 0, buf, 2, 10, 4, taps, 257, buf, None)):
        assert fwd(*args) != 0
        assert b"true_peak_forward" in lib.tfx_last_error()
    assert fwd(buf, 0, buf, 2, 10, 4, taps, 257, buf, None) != 0 and b"64 * up" in lib.tfx_last_error()
    # no rows or no samples: nothing to do, nothing touched
    assert fwd(None, 0, None, 0, 10, 4, taps, 81, None, None) == 0
    assert fwd(None, 0, None, 2, 0, 4, taps, 81, None, None) == 0
    assert info(2, 10, 4, 81, 0, *refs) == 0 and o[0].value == 21


def test_op_has_a_meta_kernel_and_no_cpu_kernel():
    import torchfx_amd.ops  # noqa: F401
    from torchfx_amd import torchfx_ext as E
    taps = torch.zeros(81)
    m = torch.ops.torchfx_hip.true_peak(torch.empty(2, 3, 4812, device="meta"), taps, 4)
    assert m.shape == (2, 3) and m.dtype == torch.float32
    assert torch.ops.torchfx_hip.true_peak(torch.empty(100, device="meta", dtype=torch.float64), taps, 4).shape == ()
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.true_peak(torch.zeros(2, 4800), taps, 4)
