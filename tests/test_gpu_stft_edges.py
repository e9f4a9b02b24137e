"""The short-time Fourier transform (torchfx_amd/csrc/stft.hip) where tests/test_gpu_stft.py leaves it free to be wrong, at the
cases of tests/spectral_cases.py (tests/test_spectral_cases_host.py holds the plan answers they rely on):

G  the staging switch at hop > n_fft: hops n - 1 (one image), n + 1, n + 3 and 3 n + 5 (frame by frame, every frame start at
   another alignment), 2 G + 1 frames.  Centred with reflection: within the bound of tests/stft_reference.py and, float32,
   within 4x the CPU float32 torch.stft.  Not centred: frames 0, G - 1, G and 2 G have the bits of the one-frame call on their
   own n_fft samples.
H  rows no longer than the zero padding (T = 1, 2, pad - 1, pad, pad + 1): torch's shape, within the bound; a single sample under
   a rectangular window comes back exactly in bin 0 and, up to its sign, in bin n / 2; a zero row gives exact zeros as complex
   values, magnitudes and powers.
I  center=False leaves nothing to pad: "constant", "replicate" and "circular" take the kernel and return the bits of "reflect".

At most 4 rows."""
import warnings

import numpy as np
import pytest
import torch

from tests import spectral_cases as C
from tests import stft_reference as R
from tests.gpu_common import ext
from tests.test_gpu_stft import DTYPES, TDT, check, gauss, hann, run

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # torch's "a window was not provided"
        yield


def bits(a, dtype):
    """A complex result as its real and imaginary parts side by side, for a comparison that tells -0 from 0."""
    return np.ascontiguousarray(a).view(dtype)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", C.APART_SIZES)
def test_hops_around_the_staging_switch(n_fft, dt):
    dtype = DTYPES[dt]
    w = hann(n_fft, dtype)
    for hop in C.apart_hops(n_fft):
        G, Tc, Tu = C.apart_lengths(n_fft, hop, dt)
        x = gauss(3, Tc, n_fft + hop, dtype)
        got = run(x, n_fft, hop, w)
        assert got.shape[-1] == 2 * G + 1
        s, _ = check(got, x, n_fft, hop, f"G n_fft {n_fft} hop {hop} {dt}, centred", w)
        if dtype == np.float32:
            cpu = torch.stft(torch.from_numpy(x), n_fft, hop, window=torch.from_numpy(w), return_complex=True).numpy()
            X = R.exact(s)
            e_dev, e_cpu = R.frame_errors(got, X)[0].max(), R.frame_errors(cpu, X)[0].max()
            print(f"G n_fft {n_fft} hop {hop}: largest frame l2 error, device / CPU torch.stft = {e_dev / e_cpu:.3f}")
            assert e_dev <= 4 * e_cpu
        x = gauss(3, Tu, n_fft + hop + 1, dtype)
        got = run(x, n_fft, hop, w, center=False)
        assert got.shape[-1] == 2 * G + 1
        check(got, x, n_fft, hop, f"G n_fft {n_fft} hop {hop} {dt}, not centred", w, center=False)
        for f in sorted({0, G - 1, G, 2 * G, got.shape[-1] - 1}):
            for r in range(3):
                alone = run(x[r:r + 1, f * hop:f * hop + n_fft], n_fft, hop, w, center=False)
                assert alone.shape == (1, n_fft // 2 + 1, 1)
                assert np.array_equal(bits(alone[0, :, 0], dtype), bits(got[r, :, f], dtype)), (hop, f, r)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", C.APART_SIZES)
def test_rows_no_longer_than_the_zero_padding(n_fft, dt):
    dtype = DTYPES[dt]
    pad = n_fft // 2
    w = hann(n_fft, dtype)
    for hop in C.short_hops(n_fft):
        for T in C.short_rows(n_fft):
            x = gauss(3, T, n_fft + T, dtype).copy()
            x[2] = 0
            shape = torch.stft(torch.from_numpy(x), n_fft, hop, center=True, pad_mode="constant", return_complex=True).shape
            assert shape[-1] == 1 + T // hop
            for what, win in (("hann", w), ("rectangular", None)):
                got = run(x, n_fft, hop, win, pad_mode="constant")
                assert got.shape == tuple(shape)
                check(got, x, n_fft, hop, f"H n_fft {n_fft} hop {hop} T {T} {what} {dt}", win, pad_mode="constant")
                assert (got[2] == 0).all()
                for kw in (dict(normalized=True), dict(power=1.0), dict(power=2.0), dict(power=1.0, normalized=True), dict(power=2.0, normalized=True)):
                    assert (run(x, n_fft, hop, win, pad_mode="constant", **kw)[2] == 0).all(), (T, hop, what, kw)
            if T == 1:                                  # the sample sits at n / 2 - f hop of frame f: the only non-zero term of any bin
                for f in range(shape[-1]):
                    at = pad - f * hop
                    assert 0 <= at < n_fft
                    sign = -1.0 if at % 2 else 1.0
                    assert np.array_equal(got[:2, 0, f], x[:2, 0].astype(got.dtype)), (hop, f)
                    assert np.array_equal(got[:2, pad, f], (sign * x[:2, 0]).astype(got.dtype)), (hop, f)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_fft", C.NOTHING_TO_PAD_SIZES)
def test_pad_modes_with_nothing_to_pad_are_the_reflect_call(n_fft, dt):
    dtype = DTYPES[dt]
    hop = n_fft // 4
    G = C.plan_g(n_fft, dtype)
    x = gauss(2, 2 * G * hop + n_fft + 1, n_fft + 3, dtype)
    w = hann(n_fft, dtype)
    want = run(x, n_fft, hop, w, center=False, pad_mode="reflect")
    check(want, x, n_fft, hop, f"I n_fft {n_fft} {dt} reflect, not centred", w, center=False)
    for mode in C.NOTHING_TO_PAD:
        assert ext().stft_plan_info(n_fft, hop, n_fft, x.shape[-1], 2, TDT[dtype], False, mode)["route"] == "lds"
        got = run(x, n_fft, hop, w, center=False, pad_mode=mode)
        assert got.dtype == want.dtype and np.array_equal(bits(got, dtype), bits(want, dtype)), mode
