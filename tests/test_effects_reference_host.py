"""CPU: the effects' reference (tests/effects_reference.py) against the obvious loops and the golden delay-line fixture, and the
host-only plan query the edge tests (tests/test_gpu_effects_edges.py) take their shapes from -- so those tests cannot fail, or
pass, by their own construction."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import effects_reference as R

DTYPES = [np.float32, np.float64]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """Bit for bit outside NaNs, and NaN exactly where the other has one."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def specials(dtype):
    one, ulp = dtype(1), np.finfo(dtype).eps
    tiny = np.finfo(dtype).smallest_subnormal
    return np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, one, -one, one + ulp, -(one + ulp), one - ulp / 2, tiny, -tiny, 37 * tiny,
                     np.finfo(dtype).tiny, 0.6, -0.6, 1.368, -1.368, 2.0, -0.5], dtype)


# ---- plan query
def test_plan_info_values_and_groups():
    from torchfx_amd import torchfx_ext as E
    assert E.effects_plan_info(0) == dict(vec=4, tile=1024, group=8192, groups=0, finish_threads=1024, stream_tile=1024)
    assert E.effects_plan_info(0, torch.float64) == dict(vec=2, tile=512, group=4096, groups=0, finish_threads=1024, stream_tile=1024)
    for dt, G in ((torch.float32, 8192), (torch.float64, 4096)):
        for T, groups in ((1, 1), (G - 1, 1), (G, 1), (G + 1, 2), (1025 * G + 5, 1026), (1024 * G, 1024)):
            assert E.effects_plan_info(T, dt)["groups"] == groups, (dt, T)
    assert "effects_plan_info" in E.__all__
    with pytest.raises(RuntimeError, match="effects_plan_info"):
        E.effects_plan_info(-1)


def test_plan_info_c_abi_refuses_null_outputs_and_bad_dtypes():
    from torchfx_amd import _lib
    lib = _lib.load()
    outs = [ctypes.c_int64() for _ in range(6)]
    assert lib.tfx_effects_plan_info(100, 0, *[ctypes.byref(o) for o in outs]) == 0
    assert [o.value for o in outs] == [4, 1024, 8192, 1, 1024, 1024]
    assert lib.tfx_effects_plan_info(100, 0, None, *[ctypes.byref(o) for o in outs[1:]]) != 0
    assert b"effects_plan_info" in lib.tfx_last_error()
    assert lib.tfx_effects_plan_info(100, 7, *[ctypes.byref(o) for o in outs]) != 0


# ---- gain
@pytest.mark.parametrize("dtype", DTYPES)
def test_gain_ref_is_the_loop(dtype):
    x = np.concatenate([specials(dtype), np.random.default_rng(1).uniform(-2, 2, 200).astype(dtype)])
    for g in (0.731, -2.0, 0.0):
        for clamp in (False, True):
            exp = np.empty_like(x)
            with np.errstate(all="ignore"):
                for i, v in enumerate(x):
                    p = v * dtype(g)
                    exp[i] = p if not clamp else (dtype(-1) if p < -1 else dtype(1) if p > 1 else p)
            got = R.gain_ref(x, g, clamp)
            assert same(got, exp), (g, clamp)
            if clamp:
                assert np.nanmax(np.abs(got)) <= 1 and np.isnan(got).sum() == np.isnan(exp).sum() >= 1
    assert np.signbit(R.gain_ref(np.array([-0.0, 0.0], dtype), 0.731, True)).tolist() == [True, False]
    assert np.signbit(R.gain_ref(np.array([1.0, -1.0], dtype), 0.0, True)).tolist() == [False, True]


def test_gain_ref_matches_torch_and_the_golden_gain(golden):
    g = golden("effects")
    assert np.array_equal(R.gain_ref(g["x"], 1.9, True), g["gain_clamp"]) and np.array_equal(R.gain_ref(g["x"], 0.37, False), g["gain_amp"])
    x = np.random.default_rng(2).uniform(-1, 1, 1000).astype(np.float32)
    assert np.array_equal(R.gain_ref(x, 1.9, True), torch.clamp(torch.from_numpy(x) * 1.9, -1, 1).numpy())


# ---- statistics
@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_refs_are_the_loops(dtype):
    x = np.random.default_rng(3).uniform(-1, 1, (3, 1001)).astype(dtype)
    x[1] = 0
    am, ss = R.absmax_ref(x), R.sumsq_ref(x)
    assert am.dtype == ss.dtype == np.float64 and am.shape == ss.shape == (3,)
    for r in range(3):
        assert am[r] == max(abs(float(v)) for v in x[r])
        exact = math.fsum(float(v) * float(v) for v in x[r]) if dtype == np.float32 else None
        if exact is not None:
            assert ss[r] == exact                                        # float32 squares are exact in float64
        else:
            from fractions import Fraction
            s = sum(Fraction(float(v)) ** 2 for v in x[r])
            assert abs(Fraction(float(ss[r])) - s) <= s * Fraction(1, 2 ** 52)
    assert R.absmax_ref(x.reshape(-1)) == am.max()
    y = x.copy()
    y[2, 17] = -np.nan
    assert np.isnan(R.absmax_ref(y)[2]) and R.absmax_ref(y)[0] == am[0] and np.isnan(R.absmax_ref(y.reshape(-1)))
    assert np.isnan(R.rms_ref(y)[2]) and R.rms_ref(y)[0] == np.sqrt(ss[0] / 1001)
    y[2, 17] = -np.inf
    assert R.absmax_ref(y)[2] == np.inf
    z = np.full((1, 9), -0.0, dtype)
    assert R.absmax_ref(z)[0] == 0 and not np.signbit(R.absmax_ref(z)[0]) and R.absmax_ref(z[:, :0])[0] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_signal_has_an_exact_sum_of_squares(dtype):
    """x[n] = (n mod 7) - 3: every partial sum is an integer below 2^53, so any order of float64 additions gives it exactly."""
    for n in (1, 2, 7, 1000, 8193, 1025 * 8192 + 5):
        k = np.arange(n, dtype=np.int64) % 7 - 3
        S = int((k * k).sum())
        assert S < 2 ** 53 and S == 28 * (n // 7) + sum((j - 3) ** 2 for j in range(n % 7))
        if n <= 8193:
            x = k.astype(dtype)
            assert R.sumsq_ref(x) == S and R.rms_ref(x) == np.sqrt(np.float64(S) / np.float64(n))
            assert float(np.cumsum(x.astype(np.float64)[::-1] ** 2)[-1]) == S


# ---- normalize apply
@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_apply_ref_is_the_loop(dtype):
    x = np.random.default_rng(4).uniform(-3, 3, (4, 77)).astype(dtype)
    x[1] = 0
    x[1, ::3] = -0.0
    x[3, 5] = np.inf
    for s in (np.array([2.5]), R.absmax_ref(x), np.array([0.0]), np.array([np.nan]), np.array([1.7, 0.0, np.nan, np.inf])):
        got = R.normalize_apply_ref(x, s, 0.9)
        exp = np.empty_like(x)
        with np.errstate(all="ignore"):
            for r in range(4):
                sv = dtype(s[r] if s.size > 1 else s[0])
                for n in range(77):
                    exp[r, n] = (x[r, n] / sv) * dtype(0.9) if sv > 0 else x[r, n]
        assert same(got, exp), s
    got = R.normalize_apply_ref(x, R.absmax_ref(x), 0.9)
    assert same(got[1], x[1]) and np.isnan(got[3, 5]) and not got[3, :5].any()          # zero row untouched; inf / inf; x / inf
    assert same(R.normalize_apply_ref(x[0], np.array([2.5]), 0.9), R.normalize_apply_ref(x[:1], np.array([2.5]), 0.9)[0])


# ---- delay line
def loop_delay(x, D, c, hist):
    rows, T = x.shape
    y = np.zeros((rows, T), np.longdouble)
    for r in range(rows):
        for n in range(T):
            y[r, n] = np.longdouble(x[r, n])
            if n >= D:
                y[r, n] += np.longdouble(c) * np.longdouble(x[r, n - D])
            elif hist is not None:
                y[r, n] += np.longdouble(c) * np.longdouble(hist[r, n])
    return y


@pytest.mark.parametrize("dtype", DTYPES)
def test_delay_line_ref_is_the_loop(dtype):
    g = np.random.default_rng(5)
    for D, T in ((0, 9), (1, 9), (3, 40), (8, 9), (9, 9), (12, 9), (5, 0)):
        x = g.uniform(-1, 1, (2, T)).astype(dtype)
        for hist in (None, g.uniform(-1, 1, (2, D)).astype(dtype)):
            y, bnd, term = R.delay_line_ref(x, D, 0.6, 0.45, hist)
            c = dtype(0.45 * 0.6)
            assert y.dtype == np.longdouble and y.shape == bnd.shape == term.shape == x.shape
            assert np.array_equal(y, loop_delay(x, D, c, hist))
            v = np.concatenate([np.zeros((2, D), dtype) if hist is None else hist, x], axis=1)[:, :T]
            assert np.allclose(term, np.abs(np.float64(c) * v), rtol=1e-15, atol=0)
            assert np.array_equal(bnd, R.EPS[np.dtype(dtype)] * (term + np.abs(y).astype(np.float64)))
            assert np.array_equal(R.hist_ref(x, D, hist), np.concatenate([np.zeros((2, D), dtype) if hist is None else hist, x], 1)[:, T:])
            assert R.hist_ref(x, D, hist).shape == (2, D)
            # both evaluations the build may choose are inside the bound
            two = x + c * v.astype(dtype)
            if hist is None:
                two[:, :min(D, T)] = x[:, :min(D, T)]
            assert (np.abs(two.astype(np.longdouble) - y) <= bnd).all()
            fused = y.astype(dtype)
            assert (np.abs(fused.astype(np.longdouble) - y) <= bnd).all()


def test_delay_line_ref_exact_cases():
    x = np.zeros((1, 20), np.float32)
    x[0, 4] = 1
    y, bnd, _ = R.delay_line_ref(x, 7, 0.5, 0.3)
    exp = np.zeros(20)
    exp[4], exp[11] = 1, np.float32(0.15)
    assert np.array_equal(y[0].astype(np.float64), exp) and (bnd[0][exp == 0] == 0).all()
    x[0, 4] = np.nan
    y, _, _ = R.delay_line_ref(x, 7, 0.5, 0.3)
    assert np.flatnonzero(np.isnan(y[0])).tolist() == [4, 11]
    y, _, _ = R.delay_line_ref(x, 7, 0.0, 0.3)
    assert np.flatnonzero(np.isnan(y[0])).tolist() == [4, 11]               # 0 * NaN: the term is added whatever the coefficient


def test_delay_line_ref_against_the_golden_fixture(golden):
    """tests/golden/delay.npz: the reference's own delay line (D = 100, decay 0.5, mix 0.3, float32) lies inside the bound."""
    g = golden("delay")
    y, bnd, term = R.delay_line_ref(g["x"], 100, 0.5, 0.3)
    err = np.abs(g["y"].astype(np.longdouble) - y)
    assert (err <= bnd).all(), float((err / np.maximum(bnd, 1e-300)).max())
    assert (term[:, 100:] > 1e3 * bnd[:, 100:]).any() and not term[:, :100].any()
    assert np.array_equal(g["y"][:, :100], g["x"][:, :100])
