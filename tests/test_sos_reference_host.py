"""The wide reference of the SOS accuracy tests and the facts of their grid, on the host (no GPU).

tests/test_gpu_sos_accuracy.py holds the device to a small multiple of what the sequential float64 recursion loses against a
__float128 recursion.  That only means something if (a) the wide recursion is right, (b) it is far closer to the truth than the
float64 one on every case, and (c) the float32 condition of the device test (at most 1 % of the float32 outputs differ from the
rounded truth) is one a correct float64 implementation meets with room: the sequential recursion is below 0.1 % everywhere.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import sos_reference as R


def test_wide_type_has_at_least_64_mantissa_bits():
    assert O.wide_mant_dig() >= 64


def test_wide_recursion_equals_exact_rational_arithmetic_bit_for_bit():
    """T = 48, K = 2, one row, start states included; coefficients and samples with short mantissas: an exact value gains two
    bits per sample, so the last ones need about 110 bits -- more than a double holds, less than the wide type does."""
    T, K = 48, 2
    sos = np.array([[0.5, 0.25, -0.5, 1.0, -0.75, 0.25],
                    [0.75, -0.5, 0.25, 1.0, 0.25, 0.5]])
    rng = np.random.default_rng(3)
    x = rng.integers(-15, 16, (1, T)) / 16.0
    sx0 = rng.integers(-7, 8, (K, 1, 2)) / 8.0
    sy0 = rng.integers(-7, 8, (K, 1, 2)) / 8.0
    sx0_given, sy0_given = sx0.copy(), sy0.copy()
    y, sx, sy, sec = O.sos_forward_wide(x, sos, sx0, sy0, sections=True)

    co = [[Fraction(float(v)) for v in row] for row in sos]
    v1 = [Fraction(float(sx0[s, 0, 0])) for s in range(K)]
    v2 = [Fraction(float(sx0[s, 0, 1])) for s in range(K)]
    y1 = [Fraction(float(sy0[s, 0, 0])) for s in range(K)]
    y2 = [Fraction(float(sy0[s, 0, 1])) for s in range(K)]
    exact, bits = np.empty((K, T)), 0
    for n in range(T):
        val = Fraction(float(x[0, n]))
        for s in range(K):
            b0, b1, b2, _, a1, a2 = co[s]
            yn = b0 * val + b1 * v1[s] + b2 * v2[s] - a1 * y1[s] - a2 * y2[s]
            v2[s], v1[s], y2[s], y1[s] = v1[s], val, y1[s], yn
            val = yn
            exact[s, n] = float(yn)                 # Fraction -> float rounds correctly (to nearest, ties to even)
            assert yn.denominator & (yn.denominator - 1) == 0
            bits = max(bits, abs(yn.numerator).bit_length())
    assert 53 < bits <= min(O.wide_mant_dig(), 113), bits      # (a long double fallback cannot pass this test)
    assert np.abs(exact[-1]).max() > 0.1            # the case is not degenerate
    assert np.array_equal(sec[:, 0, :], exact)
    assert np.array_equal(y[0], exact[-1])
    for s in range(K):
        assert sx[s, 0, 0] == float(v1[s]) and sx[s, 0, 1] == float(v2[s])
        assert sy[s, 0, 0] == float(y1[s]) and sy[s, 0, 1] == float(y2[s])
    # the inputs are not modified, and the float64 oracle differs (or this test would not tell the two apart)
    assert np.array_equal(sx0, sx0_given) and np.array_equal(sy0, sy0_given)
    assert not np.array_equal(O.sos_forward(x, sos, sx0, sy0)[0], y)


def test_wide_and_float64_oracles_agree_on_a_benign_cascade():
    for fs in R.RATES:
        c = R.case("lp2k_butter4", fs)
        assert c.e_seq <= 2e-14, (fs, c.e_seq)
        assert np.array_equal(c.sx[0, :, 0], c.x[:, -1].astype(np.float64)) and np.array_equal(c.sx[0, :, 1], c.x[:, -2].astype(np.float64))


def test_a_stale_oracle_library_is_named(monkeypatch):
    class Stale:
        pass

    monkeypatch.setattr(O, "_LIB", Stale())
    with pytest.raises(RuntimeError, match="make -C oracle oracle"):
        O.sos_forward_wide(np.zeros((1, 4)), np.array([[1.0, 0, 0, 1, 0, 0]]))


@pytest.fixture(scope="module")
def spot():
    """Row 0 of every case in numpy's long double, one pass over the grid."""
    ld = R.long_double_rows([R.design(n, fs) for n, fs in R.GRID], R.signal()[0])
    return {key: ld[i] for i, key in enumerate(R.GRID)}


@pytest.mark.parametrize("name,fs", R.GRID, ids=R.GRID_IDS)
def test_grid_facts(name, fs, spot):
    c = R.case(name, fs)
    assert c.x.dtype == np.float32 and c.x.shape == (R.ROWS, R.T) and np.abs(c.x).max() < 1.0
    # (b) the wide recursion against an independent one in another wide format, same row: they differ by what 64 mantissa bits
    #     lose, and the float64 recursion's own loss is at least 64 times that (measured: 1000 to 2000 times).  The wide result
    #     is compared as the double it was rounded to, so half an ulp of the scale is the least the difference can be held to:
    #     that floor decides on the benign control alone, whose bar in the device test is 32 times it.
    scale = R.scale_of(c.y[0])
    d_ld = float(np.abs(spot[(name, fs)] - c.y[0].astype(np.longdouble)).max()) / scale
    e_row = R.err(c.y_seq[0], c.y[0])
    print(f"{name}@{fs}: e_seq {c.e_seq:.2e} (row 0: {e_row:.2e}), wide - long double {d_ld:.2e}, "
          f"wrong32 of the sequential recursion {R.wrong32(c.y_seq, c.y):.1e}")
    if O.wide_mant_dig() > 64:
        assert d_ld <= max(e_row / 64, 2.0 ** -53 * (1 + 2.0 ** -8)), (e_row, d_ld)
    # (c) float32 outputs of the sequential float64 recursion that are not the rounded truth: at most 0.1 % on the grid's own
    #     signal, and -- the sturdier statement, since three rows resolve a share of 0.09 % to +-0.01 % only -- over four
    #     times as many rows drawn with other seeds
    assert R.wrong32(c.y_seq, c.y) <= 1e-3
    more = np.concatenate([R.signal(R.ROWS, R.T, seed) for seed in (11, 12, 13, 14)])
    w12 = R.wrong32(O.sos_forward(more, c.sos)[0], O.sos_forward_wide(more, c.sos)[0])
    print(f"{name}@{fs}: wrong32 of the sequential recursion over 12 more rows {w12:.1e}")
    assert w12 <= 1e-3
    for e in c.e_sec:
        assert np.isfinite(e)


def test_the_refinement_rule_leaves_the_benchmarked_cascades_alone_and_takes_the_hard_ones():
    """tfx_sos_refine_info (host only).  The cascades bench.py builds -- cfg 2 and the chain (LoButterworth-6 | ParametricEQ
    at 48 kHz), the cascades of its reference-style table at 44.1 kHz -- keep the unrefined kernels, so their launches and
    bits are what they were; so does the grid's benign control.  bench.py's signals and results are float32, so the float32
    rule is the one that decides its launches; with a float64 result, which bench.py never asks for, LoButterworth-6 alone
    and the 44.1 kHz cascades would refine (blocked 6e-14 against seq 1e-14 at 16 samples per lane), and nothing is asserted
    about that.  The hard designs refine at every rate.  The last loop checks that the reported decision is the documented
    rule applied to the reported errors; that the rule is the right one is what tests/test_gpu_sos_accuracy.py measures."""
    import torch
    from torchfx_amd import filter as F
    from torchfx_amd import torchfx_ext as E

    def sos_of(fs, *fl):
        for f in fl:
            f.fs = fs
            f.compute_coefficients()
        return torch.cat([f._sos for f in fl])

    lo6, peq = F.LoButterworth(2000, order=6), F.ParametricEQ(frequency=1000, q=2.0, gain=3.0)
    bench = [sos_of(48000, lo6, peq), sos_of(48000, lo6), sos_of(48000, peq), sos_of(44100, F.LoButterworth(2000, order=6)),
             sos_of(44100, F.HiButterworth(1000, order=2), F.LoButterworth(5000, order=2), F.HiChebyshev1(1500, order=2),
                    F.LoChebyshev1(1800, order=2)),
             sos_of(44100, F.LoButterworth(2000, order=4)), sos_of(44100, F.LoButterworth(2000, order=8))]
    bench += [torch.from_numpy(R.design("lp2k_butter4", fs)) for fs in R.RATES]
    for i, sos in enumerate(bench):
        info = E.sos_plan_info(sos)
        # bench.py's signals and results are float32: the float32 rule decides its launches
        assert not info["refine_f32"] and info["blocked_error"][0] < 1e-13, info       # a thousand times inside the rule
        if i == 0 or i >= 7:              # cfg 2 / the chain as built, and the benign control: not with a float64 result either
            assert not info["refine_f64"], info
    for name in ("hp20_butter4", "hp20_cheby1_4", "notch50_q30", "peak30_q8_12db"):
        for fs in R.RATES:
            info = E.sos_plan_info(R.design(name, fs))
            assert info["refine_f32"] and info["refine_f64"], (name, fs, info)
    for name, fs in R.GRID:
        info = E.sos_plan_info(R.design(name, fs))
        (b64, b16), (s64, s16) = info["blocked_error"], info["sequential_error"]
        assert info["refine_f32"] == (b64 > 1e-10) and info["refine_f64"] == (b16 > 2 * max(s16, 2.0 ** -50)), (name, fs, info)
        # the replayed sequential recursion is the oracle's, on another signal: the same loss within the spread between signals
        assert 0.25 * R.case(name, fs).e_seq <= max(s64, 2.0 ** -53) and s64 <= 4 * max(R.case(name, fs).e_seq, 2.0 ** -53), (name, fs, s64)
