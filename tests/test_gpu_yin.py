"""YIN on the device (torchfx_amd/csrc/yin.hip) against tests/yin_reference.py: the normalised difference function under the
derived bound at every frame and lag, the pick against the host pick on the device's own cmndf, the tone cases, bit equality
across rows and frame offsets, the reach of a non-finite sample and degenerate input.  The geometries are the smallest that
take each route (tests/test_yin_host.py checks their plans): four shared blocks, one block, gcd 10 (direct), hop > W."""
import numpy as np
import pytest
import torch

from tests import yin_reference as R
from tests.gpu_common import DEV
from tests.test_yin_host import GEOMETRIES, fx, length

pytestmark = pytest.mark.gpu

FS = 8000.0
# (leading shape, center, pad_mode, fmin, T): fmin 80 gives 102 lags, 230 gives 37 (the tone's period lies outside: arg-min
# route); T None is tests.test_yin_host.length(hop), 200 a row shorter than a frame (and than its workgroup's span)
VARIANTS = [((), False, "constant", 80.0, None), ((2,), True, "reflect", 80.0, None), ((2, 3), True, "constant", 230.0, None),
            ((), True, "constant", 80.0, 200), ((2,), True, "reflect", 80.0, 200)]


def run(x, fmin, n, W, hop, center=True, pad_mode="constant", fs=FS, fmax=2000.0):
    out = fx().yin(torch.from_numpy(x).to(DEV), fs, fmin, fmax, n, W, hop, center=center, pad_mode=pad_mode, return_aperiodicity=True,
                   return_cmndf=True)
    return tuple(v.cpu().numpy() for v in out)


def check_against_reference(x, fs, fmin, fmax, n, W, hop, center, pad_mode):
    """cmndf under the derived bound at every frame and lag; tau, f0 and aperiodicity those of the host pick on the device's cmndf."""
    dtype = x.dtype.type
    f0, ap, cm = run(x, fmin, n, W, hop, center, pad_mode, fs, fmax)
    ref = R.reference(x, fs, fmin, fmax, n, W, hop, center=center, pad_mode=pad_mode)
    assert cm.shape == ref["cmndf"].shape and cm.dtype == dtype and f0.shape == ap.shape == ref["f0"].shape
    share = np.abs(cm - ref["cmndf"]) / (R.cmndf_bound(W, cm.shape[-1], dtype) * ref["cmndf"])
    print(f"largest share of the cmndf bound: {share.max():.4f}")
    assert share.max() <= 1.0
    for i in np.ndindex(*f0.shape):
        tau, delta, f, b = R.pick(cm[i], fs, ref["tau_min"], ref["tau_max"], 0.1)
        assert round(float(dtype(fs) / f0[i] - delta)) == tau and ap[i] == b, i
        assert abs(f0[i] - f) <= R.f0_tolerance(cm[i], tau, fs, 0.0, 2 * R.unit(dtype)), i
    return f0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("lead, center, pad_mode, fmin, T", VARIANTS)
def test_cmndf_meets_the_bound_and_the_pick_is_the_host_pick(lead, center, pad_mode, fmin, T, geometry, dtype):
    n, W, hop = geometry
    x = R.tone(220.0, FS, T or length(hop), dtype, noise=0.3, seed=n + hop, shape=lead)
    f0 = check_against_reference(x, FS, fmin, 2000.0, n, W, hop, center, pad_mode)
    only = fx().yin(torch.from_numpy(x).to(DEV), FS, fmin, 2000.0, n, W, hop, center=center, pad_mode=pad_mode)
    assert torch.equal(only.cpu(), torch.from_numpy(f0))                # without return_cmndf: the same frequencies


@pytest.mark.parametrize("dtype, n, tau_max", [(np.float32, 8192, 4000), (np.float64, 4096, 1900)])
def test_the_longest_frames_run_with_more_than_64_KB_of_LDS(dtype, n, tau_max):
    from torchfx_amd import torchfx_ext as E
    fmin, T = 48000.0 / (tau_max - 0.5), n + n // 2 + 77                  # three frames of one row, center=False
    assert E.yin_plan_info(T, 48000.0, fmin, 4000.0, n, rows=1, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, center=False)["lds_bytes"] > 65536
    check_against_reference(R.tone(110.0, 48000.0, T, dtype, noise=0.3, seed=n), 48000.0, fmin, 4000.0, n, n // 2, n // 4, False, "constant")
    with pytest.raises(ValueError, match="frame_length"):
        fx().yin(torch.zeros(8 * n, dtype=torch.from_numpy(np.zeros(1, dtype)).dtype, device=DEV), 48000.0, frame_length=2 * n)


@pytest.mark.parametrize("f", R.TONES)
def test_tone_reads_the_reference_lag_on_every_interior_frame(f):
    g = R.TONE
    x = R.tone(f, g["fs"], R.TONE_T, np.float32)
    f0, ap, cm = run(x, g["fmin"], g["frame_length"], g["win_length"], g["hop"], fs=g["fs"], fmax=g["fmax"])
    ref = R.reference(x, g["fs"], g["fmin"], g["fmax"], g["frame_length"], g["win_length"], g["hop"])
    beta = R.cmndf_bound(g["win_length"], cm.shape[-1], np.float32)
    for i in range(5, 52):
        tau = int(ref["tau"][i])
        assert ap[i] < 0.1 and R.pick(cm[i], g["fs"], ref["tau_min"], ref["tau_max"], 0.1)[0] == tau, i
        assert abs(f0[i] - ref["f0"][i]) <= R.f0_tolerance(ref["cmndf"][i], tau, g["fs"], beta[tau + 1], 2 * R.unit(np.float32)), i


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_bits_do_not_depend_on_the_row_or_the_frame_index(geometry, dtype):
    n, W, hop = geometry
    x = R.tone(220.0, FS, length(hop), dtype, noise=0.3, seed=5, shape=(3,))
    whole = run(x, 80.0, n, W, hop, center=False)
    for r in range(3):
        for a, b in zip(whole, run(x[r], 80.0, n, W, hop, center=False)):
            assert np.array_equal(a[r], b)
    for a, b in zip(whole, run(np.ascontiguousarray(x[:, 3 * hop:]), 80.0, n, W, hop, center=False)):
        assert np.array_equal(a[:, 3:], b)


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_a_non_finite_sample_reaches_exactly_the_frames_that_read_it(geometry, value):
    n, W, hop = geometry
    x = R.tone(220.0, FS, length(hop), np.float32, noise=0.3, seed=9, shape=(2,))
    clean = run(x, 80.0, n, W, hop, pad_mode="reflect")
    for at in (20 * hop + 3, 5):                                        # interior; inside the reflected edge: read twice by early frames
        y = x.copy()
        y[1, at] = value
        f0, ap, cm = run(y, 80.0, n, W, hop, pad_mode="reflect")
        hit = R.reference(y, FS, 80.0, 2000.0, n, W, hop, pad_mode="reflect")["bad"]
        assert hit.any() and not hit.all() and not hit[0].any()
        assert np.array_equal(np.isnan(f0), hit) and np.array_equal(np.isnan(ap), hit) and np.array_equal(np.isnan(cm).all(-1), hit)
        assert np.array_equal(cm[~hit], clean[2][~hit])
        assert np.array_equal(f0[~hit], clean[0][~hit]) and np.array_equal(ap[~hit], clean[1][~hit])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("level, T, center", [(0.0, 200, True), (0.25, 600, False)])      # silence: a row shorter than a frame
def test_silence_and_a_constant_are_unvoiced_at_the_shortest_lag(level, T, center, dtype):
    f0, ap, cm = run(np.full((2, T), level, dtype=dtype), 80.0, 256, 128, 32, center=center)
    assert f0.shape[-1] >= 1 and np.all(cm == 1) and np.all(ap == 1) and np.all(f0 == dtype(FS) / dtype(4))
