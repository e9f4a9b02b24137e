"""The inverse short-time Fourier transform (torchfx_amd/csrc/istft.hip) where tests/test_gpu_istft.py leaves it free to be wrong,
at the cases of tests/spectral_cases.py (tests/test_spectral_cases_host.py holds what they rely on):

A  asymmetric windows -- a ramp over n_fft, and a ramp over n_fft - 55 values, whose zeros split 27 | 28 and whose hop does not
   divide the tile -- on Gaussian bins, within the per-sample bound of tests/istft_reference.py and, float32, within 4x the error
   of the CPU float32 torch.istft.  A reversed window, a short window reversed before it is padded and a window one sample late
   each miss that bound by more than 100x on these very inputs, and the CPU transform uses less than 0.05 of it (host file).
B  one tap at hop 1: output t is sample 127 of frame t + 1, to the bit, for 4098 frames a row (72 batches a tile); a tap of 2
   halves and a tap of 0.5 doubles it, exactly.
C  a lone non-zero frame at frames 0, G - 1, G, tile / hop - 1, tile / hop and the last: the same bits wherever it lies, halved
   exactly where two rectangular windows cover it, exact zeros everywhere else.
D  the flag: a falling ramp ends in 0, so the envelope vanishes at the row's last sample alone -- the call raises at the natural
   length and passes one sample short of it; constant windows of 1e-5 and 1e-6 lie on either side of the 1e-11 threshold.
E  `length` for float64 at 4096, where the tile is n_fft and a batch holds one frame: prefixes and zero tails to the bit.
F  stft then istft under the short ramp against the same round trip through CPU torch.

Shapes come from the plan (three_tiles of tests/test_gpu_istft.py); at most 4 rows."""
import warnings

import numpy as np
import pytest
import torch

from tests import istft_reference as R
from tests import spectral_cases as C
from tests.gpu_common import DEV, ext
from tests.test_gpu_istft import CDT, RDT, S, check, plan, relayout, spectrum, three_tiles

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # torch's "a window was not provided", "the length is longer"
        yield


def on_device(X):
    """CPU bins ``[rows, bins, frames]`` -> the device, in the layout stft returns."""
    return relayout(X.to(DEV))


def window(values, dt):
    return torch.from_numpy(np.asarray(values, np.float64)).to(RDT[dt]).to(DEV)


@pytest.mark.parametrize("dt", C.DTS)
@pytest.mark.parametrize("c", C.A_CASES, ids=C.placed_id)
def test_asymmetric_windows_are_placed_as_the_contract_says(c, dt):
    w = torch.from_numpy(C.placed_window(c, dt)).to(DEV)
    assert w.shape == (c.wl,) and w.dtype == RDT[dt]
    got = check(on_device(C.placed_input(c, dt)), c.n, c.hop, dt, w, c.wl, normalized=c.normalized, what=f"A {dt} {C.placed_id(c)}")
    assert got.shape == (C.A_ROWS, (C.placed_frames(c, dt) - 1) * c.hop)


@pytest.mark.parametrize("dt", C.DTS)
def test_one_tap_at_hop_one_returns_sample_127_of_every_frame_to_the_bit(dt):
    n = C.TAP_N
    X = on_device(C.tap_input(dt))
    F = X.shape[-1]
    assert F == C.tap_frames(dt)
    frames = S().istft(X, n, n, center=False)                          # rectangular, side by side: sample f n + i is s_f[i]
    assert frames.shape == (2, F * n)
    want = C.tap_expected(frames)
    assert want.shape == (2, F - 1) and C.scales_exactly(want.cpu().numpy()) and bool((want != 0).any())
    for tap, factor in C.TAPS:
        for w in ([None] if tap == 1.0 else []) + [window([tap], dt)]:
            y = S().istft(X, n, 1, 1, w)
            assert y.shape == want.shape and torch.equal(y, want * factor), (tap, w is None, int((y != want * factor).sum()))
    check(X, n, 1, dt, None, 1, what=f"B {dt} one tap, hop 1, {F} frames", cpu_ratio=False)


@pytest.mark.parametrize("dt", C.DTS)
@pytest.mark.parametrize("n", [256, 4096])
def test_a_lone_frame_has_the_same_bits_wherever_it_lies(n, dt):
    blocks = C.lone_blocks(n, dt)
    seen = {}                                                           # row -> its block at hop = n, first placement
    for hop in (n, n // 2):
        frames, G, tile, at = C.lone_geometry(n, hop, dt)
        for k, f in enumerate(at):
            where = (f, at[-1 - k])                                     # row 1 visits the placements in the opposite order
            X = torch.zeros(2, n // 2 + 1, frames, dtype=CDT[dt])
            for r in range(2):
                X[r, :, where[r]] = blocks[r]
            y = S().istft(on_device(X), n, hop, center=False)
            assert y.shape == (2, (frames - 1) * hop + n)
            for r in range(2):
                lo = where[r] * hop
                block = y[r, lo:lo + n]
                assert bool((y[r, :lo] == 0).all()) and bool((y[r, lo + n:] == 0).all()), (hop, where[r], r)
                if r not in seen:
                    assert hop == n and C.scales_exactly(block.cpu().numpy()) and bool((block != 0).all())
                    seen[r] = block.clone()
                cover = torch.from_numpy(C.lone_cover(n, hop, frames, where[r])).to(RDT[dt]).to(DEV)
                assert torch.equal(block, seen[r] / cover), (hop, where[r], r, int((block != seen[r] / cover).sum()))


@pytest.mark.parametrize("dt", C.DTS)
@pytest.mark.parametrize("n", [256, 4096])
def test_the_flag_reaches_the_rows_last_sample_and_no_further(n, dt):
    hop = n // 4
    frames = three_tiles(n, hop, dt)
    X = spectrum(n, hop, frames, 2, dt, 4)
    w = window(C.falling(n), dt)
    natural = R.natural_length(frames, n, hop, 0)
    with pytest.raises(RuntimeError, match="window overlap add min"):
        S().istft(X, n, hop, window=w, center=False)
    _, flag = ext().istft_forward(X, w, n, hop, 0)
    assert int(flag.item()) == 1
    y, flag = ext().istft_forward(X, w, n, hop, 0, natural - 1)
    assert int(flag.item()) == 0 and y.shape == (2, natural - 1)
    got = check(X, n, hop, dt, w, center=False, length=natural - 1, what=f"D {dt} {n} falling ramp, natural - 1", cpu_ratio=False)
    assert torch.equal(got, y)


def test_the_flag_on_either_side_of_the_threshold():
    for n, hop, center in C.NEAR_GEOMETRIES:
        X = spectrum(n, hop, three_tiles(n, hop, "f32"), 2, "f32", 5)
        for value, passes in C.NEAR:
            w = torch.full((n,), value, dtype=torch.float32, device=DEV)
            _, flag = ext().istft_forward(X, w, n, hop, n // 2 if center else 0)
            assert int(flag.item()) == (0 if passes else 1), (n, hop, value)
            if passes:
                check(X, n, hop, "f32", w, center=center, what=f"D f32 {n}/{hop} constant window {value}", cpu_ratio=False)
            else:
                with pytest.raises(RuntimeError, match="window overlap add min"):
                    S().istft(X, n, hop, window=w, center=center)


def test_length_where_the_tile_is_one_frame():
    n, hop, dt = 4096, 1024, "f64"
    frames = three_tiles(n, hop, dt)
    p = plan(n, hop, frames, dt, center=False)
    tile, natural = p["tile"], p["length"]
    assert tile == n and p["frames_per_batch"] == 1 and natural == R.natural_length(frames, n, hop, 0)
    X = spectrum(n, hop, frames, 2, dt, 6)
    nat = check(X, n, hop, dt, None, center=False, what="E f64 4096/1024 rectangular, natural length")
    assert nat.shape == (2, natural)
    for length in (1, tile - 1, tile, tile + 1, natural - 1):
        assert torch.equal(S().istft(X, n, hop, center=False, length=length), nat[:, :length]), length
    for length in (natural + 1, natural + tile + 3):
        got = S().istft(X, n, hop, center=False, length=length)
        assert got.shape == (2, length) and torch.equal(got[:, :natural], nat) and bool((got[:, natural:] == 0).all()), length


@pytest.mark.parametrize("dt", C.DTS)
@pytest.mark.parametrize("c", C.F_CASES, ids=C.placed_id)
def test_round_trip_under_a_short_ramp(c, dt):
    frames = C.placed_frames(c, dt)
    g = np.random.default_rng(c.n + c.hop)
    x = torch.from_numpy(g.standard_normal((2, (frames - 1) * c.hop)).astype(C.NP[dt]))
    wc = torch.from_numpy(C.placed_window(c, dt))
    w = wc.to(DEV)
    back = S().istft(S().stft(x.to(DEV), c.n, c.hop, c.wl, w), c.n, c.hop, c.wl, w)
    cpu = torch.istft(torch.stft(x, c.n, c.hop, c.wl, wc, return_complex=True), c.n, c.hop, c.wl, wc)
    err, cpu_err = float((back.cpu() - x).abs().max()), float((cpu - x).abs().max())
    print(f"F {dt} {C.placed_id(c)}: round trip error {err:.3e}, through CPU torch {cpu_err:.3e}, ratio {err / cpu_err:.2f}")
    assert back.shape == x.shape and err <= 4 * cpu_err
