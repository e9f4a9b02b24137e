"""Identity phase locking on the device (phase_lock_kernel) against tests/phaselock_reference.py."""
import numpy as np
import pytest
import torch

from tests import phaselock_reference as L
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu
RDT = {"f32": torch.float32, "f64": torch.float64}
# bins: no neighbour, fewer than the window, one mask word, a word boundary, a one-bin tail word, three, five and nine bins a lane;
# segments by force; at rate 0.5 output frames 2 m and 2 m + 1 share i, and the cuts (9 of 18, 47 and 94 of 140) part such pairs
CASES = [(1, 1, 1, 1), (3, 2, 3, 1), (64, 9, 1, 2), (65, 70, 3, 3), (129, 9, 3, 2), (513, 70, 1, 3), (1025, 9, 1, 2), (4097, 3, 1, 2)]
WORST = {}


def fx():
    import torchfx_amd
    return torchfx_amd


def locked(X, rate, segments=0):
    return ext().phase_vocoder_forward(X, rate, segments, 1)


@pytest.mark.parametrize("rate", [0.5, 0.8, 1.0, 1.25, 2.5])
@pytest.mark.parametrize("bins,F,rows,segments", CASES)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_locked_result_meets_the_derived_bound(dt, bins, F, rows, segments, rate):
    Xh = L.ladder(rows, bins, F, dt)
    ref = L.reference(Xh, rate)
    assert ref[3] >= 1e-3, ref[3]                                       # the reference's own decisions have margin
    p = ext().phase_vocoder_plan_info(F, bins, rate, rows, RDT[dt], segments, 1)
    assert p["segments"] == min(segments, p["out_frames"]) and p["threads"] * p["bins_per_thread"] >= bins
    got = locked(torch.from_numpy(Xh).to(DEV), rate, segments)
    WORST[dt] = max(WORST.get(dt, 0.0), L.within(got.cpu().numpy(), ref, f"locked {dt} bins {bins} F {F} rate {rate} segments {segments}"))
    print(f"largest error / bound so far, {dt}: {WORST[dt]:.3f}")

def tie_spectrum():
    """257 bins (five mask words) x 6 frames of exact moduli 5, 13 and 25 (3+4i, 5+12i, 7+24i turned by quarter turns): frame 0
    has peaks at 0, 64 and 256 (bins 32 and 160 equidistant), frame 1 at 63 and 67 (65 equidistant) and a two-bin plateau at 10,
    11, frames 2 and 3 are flat (no peak), frame 4 has its one peak at bin 0 and frame 5 at the last bin: the scans cross up to
    four empty words, downwards and upwards."""
    g = np.random.default_rng(5)
    unit = np.array([1, 1j, -1, -1j])[g.integers(0, 4, (2, 257, 6))]
    X = (3 + 4j) * unit
    for f, ks, v in ((0, (0, 64, 256), 7 + 24j), (1, (63, 67), 7 + 24j), (1, (10, 11), 5 + 12j), (4, (0,), 5 + 12j), (5, (256,), 7 + 24j)):
        X[:, list(ks), f] = v * unit[:, list(ks), f]
    return X


@pytest.mark.parametrize("rate", [0.5, 1.25])                            # dyadic: device and reference see the same ties
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_exact_ties_and_peak_placement(dt, rate):
    Xh = tie_spectrum().astype(np.complex64 if dt == "f32" else np.complex128)
    ref = L.reference(Xh, rate)
    flat = [t for t in range(ref[2].shape[-1]) if not any(L.peaks(ref[2][0, :, t].tolist()))]
    assert flat and 0 < flat[0] and flat[-1] < ref[2].shape[-1] - 1     # frames without a peak between frames that have some
    for s in (1, 2):
        L.within(locked(torch.from_numpy(Xh).to(DEV), rate, s).cpu().numpy(), ref, f"ties {dt} rate {rate} segments {s}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_bit_equalities_with_the_plain_vocoder_and_across_cuts_and_batches(dt):
    X = torch.from_numpy(L.ladder(4, 129, 70, dt)).to(DEV)
    assert torch.equal(locked(X, 1.0), ext().phase_vocoder_forward(X, 1.0))
    flat = torch.where(X.real > 0, torch.tensor(3 + 4j, dtype=X.dtype), torch.tensor(-4 + 3j, dtype=X.dtype)).to(DEV)
    for rate in (0.5, 0.8, 1.25, 2.5):
        assert torch.equal(locked(flat, rate, 2), ext().phase_vocoder_forward(flat, rate)), rate
        one = locked(X, rate, 1)
        for s in (2, 3):
            assert torch.equal(locked(X, rate, s), one), (rate, s)
        assert torch.equal(locked(X[2], rate, 3), one[2])                # a row alone
        assert torch.equal(locked(X.reshape(2, 2, 129, 70), rate, 2).reshape(one.shape), one)
        assert torch.equal(fx().phase_vocoder(X, rate, phase_lock="identity"), one)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_non_finite_bin_poisons_every_bin_of_its_row_from_the_frame_that_reads_it(dt, value):
    F, bins, rate, row, k = 70, 129, 0.8, 1, 70
    X = torch.from_numpy(L.ladder(3, bins, F, dt)).to(DEV)
    clean = locked(X, rate, 3)
    i = np.floor(np.arange(clean.shape[-1]) * rate).astype(np.int64)
    for j in (5, 40):                                                   # read in the first segment; in the second of three only
        Y = X.clone()
        Y[row, k, j] = complex(value, 1.0)
        first = int(np.argmax(i + 1 >= j))
        assert (first < 30) == (j == 5)                                 # 88 output frames: segments of 30
        for s in (3, 1):
            got = locked(Y, rate, s)
            assert torch.equal(got[row, :, :first], clean[row, :, :first])
            assert bool(torch.isnan(torch.view_as_real(got[row, :, first:])).all())
            assert torch.equal(got[[0, 2]], clean[[0, 2]])


def test_effects_on_the_device_against_the_host_path():
    fs, T = 48000, 12000
    g = np.random.default_rng(9)
    x = torch.from_numpy(g.standard_normal((2, T)) * np.hanning(T)).to(torch.float64)
    for effect in (fx().TimeStretch(0.8, n_fft=512, phase_lock="identity"), fx().PitchShift(3, n_fft=512, phase_lock="identity")):
        dev = fx().Wave(x, fs, device=DEV) | effect
        host = fx().Wave(x, fs) | effect
        assert "identity phase locking" in dev.explain()[0] and dev.ys.is_cuda and dev.ys.shape == host.ys.shape
        # float64: angle errors of (2 t + 3) E_ANGLE rad over t < 120 frames stay below 1e-11 of the largest modulus; the
        # inverse transform and the resampler are convex sums of such values.  This rests on both paths taking the same peak
        # decisions: their moduli may differ by an ulp (sqrt(fma) and a contracted mix against np.abs), which flips a decision
        # only where two of a frame's moduli agree to 1e-16 -- on this fixed noise none does
        assert float((dev.ys.cpu() - host.ys).abs().max()) <= 1e-9 * float(host.ys.abs().max())
    with pytest.raises(ValueError, match="phase_lock"):
        fx().TimeStretch(0.8, phase_lock="scaled")
    with pytest.raises(ValueError, match="phase_lock"):                 # refused by the plan, before the transform runs
        fx().time_stretch(torch.zeros(1, 40000, device=DEV), 0.8, n_fft=16384, phase_lock="identity")
