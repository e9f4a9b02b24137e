"""The phaser's reference (tests/phaser_reference.py) against what is known in closed form: the impulse response of one constant
section, a scipy.signal.lfilter cascade for a constant coefficient, the long-double track against its float64 evaluation, and the
size of delta_a."""
import numpy as np
import pytest

from tests import phaser_reference as R

FS = 48000


def constant_track(T, freq, fs=FS):
    a = R.coef_track_ld(T, fs, freq, freq, 1.0)
    assert float(np.ptp(a.astype(np.float64))) == 0.0              # min_freq == max_freq: a constant filter
    return a.astype(np.float64)[None, :]


def test_impulse_response_of_one_constant_section():
    T = 64
    coef = constant_track(T, 1000.0)
    a = coef[0, 0]
    g = np.tan(np.pi * 1000.0 / FS)
    assert abs(a - (g - 1.0) / (g + 1.0)) < 1e-15 and -1.0 < a < 0.0
    x = np.zeros((1, T))
    x[0, 0] = 1.0
    for dtype in (np.float64, np.longdouble):
        y, s = R.phaser_loop(x, coef, 1, 0.0, 1.0, dtype=dtype)
        want = np.concatenate([[a], (1.0 - a * a) * (-a) ** np.arange(T - 1)])
        assert np.abs(y[0].astype(np.float64) - want).max() < 1e-15
        assert s.shape == (1, 2) and s[0, 0] == 0.0 and s[0, 1] == y[0, -1]


@pytest.mark.parametrize("stages", [1, 4, 12])
def test_constant_coefficient_against_an_lfilter_cascade(stages):
    from scipy.signal import lfilter

    T = 3000
    coef = constant_track(T, 700.0)
    a = coef[0, 0]
    x = np.random.default_rng(stages).uniform(-1.0, 1.0, (2, T))
    want = x
    for _ in range(stages):
        want = lfilter([a, 1.0], [1.0, a], want, axis=-1)
    y, _ = R.phaser_loop(x, coef, stages, 0.25, 0.75, channels=2)
    assert np.abs(y - (0.25 * x + 0.75 * want)).max() < 1e-12
    yld, sld, e_ref = R.reference(x, coef, stages, 0.25, 0.75, 2)
    assert 0.0 < e_ref < 1e-13 and float(np.abs(y.astype(np.longdouble) - yld).max()) == e_ref


def test_state_continues_the_loop_exactly():
    T, cut = 500, 123
    coef = R.coef_track_ld(T, FS, 200.0, 2000.0, 30.0, 0.2).astype(np.float64)[None, :]
    x = np.random.default_rng(5).uniform(-1.0, 1.0, (3, T))
    whole, s = R.phaser_loop(x, coef, 4, 0.5, 0.5)
    a, sa = R.phaser_loop(x[:, :cut], coef[:, :cut], 4, 0.5, 0.5)
    b, sb = R.phaser_loop(x[:, cut:], coef[:, cut:], 4, 0.5, 0.5, state=sa)
    assert np.array_equal(np.concatenate([a, b], -1), whole) and np.array_equal(sb, s)


@pytest.mark.parametrize("lfo", ["sine", "triangle"])
def test_the_long_double_track_and_delta_a(lfo):
    T = 4000
    ld = R.coef_track_ld(T, FS, 20.0, 8000.0, 30.0, 0.3, 0.25, 1, lfo, position=1 << 40)
    assert ld.dtype == np.longdouble and np.all(np.abs(ld) < 1)
    assert ld.min() < -0.99 and ld.max() > -0.35                    # the sweep covers its range
    tol = R.coef_tolerance(FS, 20.0, 8000.0)
    assert 1e-15 < tol < 1e-14
    assert 1e-15 < R.coef_tolerance(FS, 200.0, 2000.0) < 2e-15 and 2e-14 < R.coef_tolerance(192000, 10.0, 0.45 * 192000) < 4e-14
    # the channel offset and the position enter as the definition says
    assert not np.array_equal(ld, R.coef_track_ld(T, FS, 20.0, 8000.0, 30.0, 0.3, 0.25, 0, lfo, position=1 << 40))
    assert np.array_equal(ld[100:], R.coef_track_ld(T - 100, FS, 20.0, 8000.0, 30.0, 0.3, 0.25, 1, lfo, position=(1 << 40) + 100))
