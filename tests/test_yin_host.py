"""YIN without a GPU: the NumPy route of ``torchfx_amd.yin`` against tests/yin_reference.py, the argument errors, the plans of
the geometries the device tests run, and the tone cases both suites rest on."""
import numpy as np
import pytest
import torch

from tests import yin_reference as R

# (frame_length, win_length, hop) of tests/test_gpu_yin.py with the route each must take: (block, blocks_per_frame)
GEOMETRIES = {(256, 128, 32): (32, 4), (256, 128, 128): (128, 1), (256, 120, 50): (120, 1), (256, 128, 160): (128, 1)}


def fx():
    import torchfx_amd
    return torchfx_amd


def length(hop):
    """More than 32 frames (the most a workgroup takes) and a last workgroup that is not full."""
    return 37 * hop + 7


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("center, pad_mode", [(False, "constant"), (True, "reflect"), (True, "constant")])
def test_cpu_route_meets_the_bound_and_picks_from_its_own_cmndf(center, pad_mode, geometry, dtype):
    n, W, hop = geometry
    x = R.tone(220.0, 8000.0, length(hop), dtype, noise=0.3, seed=n + hop, shape=(2,))
    kw = dict(fmin=80.0, fmax=2000.0, frame_length=n, win_length=W, hop_length=hop, center=center, pad_mode=pad_mode)
    f0, ap, cm = (v.numpy() for v in fx().yin(torch.from_numpy(x), 8000.0, return_aperiodicity=True, return_cmndf=True, **kw))
    ref = R.reference(x, 8000.0, 80.0, 2000.0, n, W, hop, center=center, pad_mode=pad_mode)
    assert cm.shape == ref["cmndf"].shape and cm.dtype == dtype and f0.shape == ref["f0"].shape == ap.shape
    share = np.abs(cm - ref["cmndf"]) / (R.cmndf_bound(W, cm.shape[-1], dtype) * ref["cmndf"])
    assert share.max() <= 1.0, share.max()
    for i in np.ndindex(*f0.shape):
        tau, _, f, b = R.pick(cm[i], 8000.0, ref["tau_min"], ref["tau_max"], 0.1)
        assert ap[i] == b and abs(f0[i] - f) <= R.f0_tolerance(cm[i], tau, 8000.0, 0.0, 2 * R.unit(dtype)), i


@pytest.mark.parametrize("f", R.TONES)
def test_tone_is_voiced_and_read_at_the_reference_lag(f):
    x = R.tone(f, R.TONE["fs"], R.TONE_T, np.float32)
    g = R.TONE
    f0, ap, cm = (v.numpy() for v in fx().yin(torch.from_numpy(x), g["fs"], g["fmin"], g["fmax"], g["frame_length"], g["win_length"], g["hop"],
                                              return_aperiodicity=True, return_cmndf=True))
    ref = R.reference(x, g["fs"], g["fmin"], g["fmax"], g["frame_length"], g["win_length"], g["hop"])
    beta = R.cmndf_bound(g["win_length"], cm.shape[-1], np.float32)
    assert f0.shape == (57,)
    for i in range(5, 52):
        tau = int(ref["tau"][i])
        assert ap[i] < 0.1 and R.pick(cm[i], g["fs"], ref["tau_min"], ref["tau_max"], 0.1)[0] == tau
        tol = R.f0_tolerance(ref["cmndf"][i], tau, g["fs"], beta[tau + 1], 2 * R.unit(np.float32))
        assert abs(f0[i] - f) <= abs(ref["f0"][i] - f) + tol, (i, f0[i], ref["f0"][i], tol)


@pytest.mark.parametrize("kw, name", [
    (dict(fs=0.0), "fs"), (dict(fmin=-1.0), "fmin"), (dict(fmax=float("nan")), "fmax"), (dict(fmin=20.0), "fmin"),
    (dict(fmin=3000.0, fmax=2000.0), "fmin"), (dict(frame_length=1), "frame_length"), (dict(win_length=0), "win_length"),
    (dict(win_length=4096), "win_length"), (dict(hop_length=0), "hop_length"), (dict(threshold="x"), "threshold"),
    (dict(pad_mode="circular"), "pad_mode"), (dict(frame_length=8192, fmin=65.0, pad_mode="reflect"), "pad_mode"),
    (dict(center=False, frame_length=8192), "frame_length")])
def test_bad_arguments_name_themselves(kw, name):
    args = dict(fs=48000.0)
    args.update(kw)
    with pytest.raises(ValueError, match=name):
        fx().yin(torch.zeros(2, 4000), **args)
    with pytest.raises(ValueError, match="x must be"):
        fx().yin(torch.zeros(2, 4000, dtype=torch.float16), 48000.0)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_plans_reach_every_route_and_more_than_one_workgroup(geometry):
    from torchfx_amd import torchfx_ext as E
    n, W, hop = geometry
    p = E.yin_plan_info(length(hop), 8000.0, 80.0, 2000.0, n, W, hop, rows=2)
    assert (p["tau_min"], p["tau_max"], p["lags"], p["lags_per_thread"]) == (4, 100, 102, 9) and p["lags"] % 9
    assert (p["block"], p["blocks_per_frame"]) == GEOMETRIES[geometry]
    assert p["frames"] == 38 and p["workgroups"] > 2 and p["frames"] % p["frames_per_workgroup"] and p["lds_bytes"] <= 160 * 1024
    assert E.yin_plan_info(length(hop), 8000.0, 230.0, 2000.0, n, W, hop)["lags"] == 37
    forced = E.yin_plan_info(length(hop), 8000.0, 80.0, 2000.0, n, W, hop, block=W)
    assert (forced["block"], forced["blocks_per_frame"]) == (W, 1)


def test_plan_serves_the_longest_frames_and_the_benchmark_shapes():
    from torchfx_amd import torchfx_ext as E
    p = E.yin_plan_info(2_880_000, 48000.0, 65.0, rows=64)
    assert (p["block"], p["blocks_per_frame"], p["lags"]) == (512, 2, 741) and p["frames_per_workgroup"] > 1
    p = E.yin_plan_info(160_000, 16000.0, 65.0, frame_length=1024, win_length=512, hop_length=160, rows=256)
    assert (p["block"], p["blocks_per_frame"]) == (512, 1)                 # blocks of gcd = 32 do not pay: every frame sums alone


@pytest.mark.parametrize("n, W, hop, tau_max", [(2048, 1024, 64, 379), (2048, 1024, 512, 739), (1024, 512, 160, 247), (256, 128, 32, 100)])
def test_the_block_does_not_depend_on_the_number_of_frames(n, W, hop, tau_max):
    """The block fixes the order of a frame's sum, so it may follow (W, hop, Lmax, dtype) alone: a longer or shorter row, or a
    row of one frame, takes the same one (at 2048 / 1024 / 64 a cost weighed over the row's own frames would change it at 11)."""
    from torchfx_amd import torchfx_ext as E
    plans = [E.yin_plan_info(n + k * hop, 8000.0, 8000.0 / (tau_max - 0.5), 4000.0, n, W, hop, center=False) for k in (0, 1, 4, 9, 10, 11, 31, 32, 500)]
    assert [p["frames"] for p in plans] == [1, 2, 5, 10, 11, 12, 32, 33, 501]
    assert len({(p["block"], p["blocks_per_frame"]) for p in plans}) == 1 and all(p["frames_per_workgroup"] <= p["frames"] for p in plans)
    for dtype, n in ((torch.float32, 8192), (torch.float64, 4096)):
        for W, hop in ((n // 2, n // 4), (n // 2, 250), (n - 40, n)):
            p = E.yin_plan_info(5 * n, 48000.0, 48000.0 / (n - W - 2.5), 4000.0, n, W, hop, dtype=dtype)
            assert p["lags"] == n - W and p["frames_per_workgroup"] >= 1 and p["lds_bytes"] <= 160 * 1024
        with pytest.raises(RuntimeError, match="frame_length"):
            E.yin_plan_info(5 * n, 48000.0, 65.0, frame_length=2 * n, dtype=dtype)
