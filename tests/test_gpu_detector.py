"""The limiter's detector on the device at every register-tap bucket and every phase split (limiter_kernel<T, LP, false | true>,
csrc/limiter.hip; the cases are tests/detector_cases.py).  With A = H = 1 the gain is g[n] = min(fl(1 - fl(1 - r[n])), r[n]) and
r one rounded division of c by p: on a signal with |x| in [1, 2] the gain shows p[i] at EVERY position, so a wrong value of any
interpolator output that owns a maximum is seen -- bit for bit against the composition of the resampler and an IEEE division,
and within a derived bound of the float64 definition.  Then the default window at (A, H) = (72, 480), the stream form against the
one-shot call, and non-finite samples, all at the new geometries.  Geometry comes from the plan functions and is asserted."""
import math

import numpy as np
import pytest
import torch

from tests import detector_cases as D
from tests.gpu_common import DEV, dev
from tests.test_gpu_limiter import expected_one_hot, fx, loud
from tests.test_gpu_stream_limiter import signal
from tests.test_limiter_host import params, reference
from tests.test_stream_limiter_host import kwargs, random_sizes, run, stateful

pytestmark = pytest.mark.gpu

FS = D.FS
IDS = [D.case_id(c) for c in D.CASES]
F32, F64 = torch.float32, torch.float64


def case_params(cases):
    return pytest.mark.parametrize("dtype,up,nh", cases, ids=["%s-%s" % ("f32" if d == F32 else "f64", D.case_id(D.find(u, n)))
                                                               for d, u, n in cases])


# ---- A = H = 1: p[i] at every position ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("k", range(len(D.CASES)), ids=IDS)
def test_the_gain_shows_the_detector_at_every_position(k, dtype):
    """Bit equality of g and y with expected_one_hot (resample_poly on the device, division on the host), and against the float64
    reference |g - g_ref| <= c beta / (p_ref (p_ref - beta)) + 2u, |y - y_ref| <= that |x| + u |y_ref|, beta[i] the largest
    resample_reference.bound over the outputs of positions i - 1 and i (u = 2^-24 / 2^-53).  Largest err / tol measured: 0.28 (g)
    and 0.31 (y) in float32, 0.34 and 0.37 in float64."""
    c = D.CASES[k]
    geo = D.check(c, dtype)
    assert geo["tile"] == 8190 and D.LIMITER_T == 2 * geo["tile"] + 3
    st = D.limiter_statement(k, dtype)
    if k in D.FULL:                                                            # what keeps the test from hiding a failure
        share, missing = D.share_and_coverage(D.candidates(st["groups"][0]["x"], st["P"].taps.numpy(), c.up), c.up)
        assert share >= 0.9 and not missing, (share, missing)
    x = dev(np.array(st["x"]))                                                 # the shared statement stays read-only
    y, g = fx().limit(x, FS, link=st["link"], return_gain=True, **D.limiter_kwargs(c, dtype))
    ye, ge = expected_one_hot(x, st["P"], st["link"], 0)
    assert g.shape == ge.shape == (len(st["groups"]), D.LIMITER_T)
    assert torch.equal(g, ge), (int((g != ge).sum()), float((g - ge).abs().max()))
    assert torch.equal(y, ye)
    eg, ey = D.limiter_errors(st, g.cpu().numpy(), y.cpu().numpy(), dtype, 2 * D.U[dtype])
    print(D.case_id(c), dtype, "g err / tol %.3f, y err / tol %.3f" % (eg, ey))
    assert eg <= 1.0 and ey <= 1.0, (eg, ey)
    assert float(g.min()) > 0.0 and float(g.max()) < 0.9                       # p > c at every position


# ---- the default window ----------------------------------------------------------------------------------------------------
WINDOW_CASES = [(F32, 4, 28), (F32, 4, 61), (F32, 2, 41), (F32, 2, 63), (F32, 4, 189), (F32, 4, 253), (F32, 4, 256), (F32, 8, 187),
                (F64, 4, 28), (F64, 4, 83), (F64, 2, 128), (F64, 8, 381)]


@case_params(WINDOW_CASES)
def test_default_window_at_every_bucket(dtype, up, nh):
    """(A, H) = (72, 480) against the float64 reference: |g - g_ref| <= (A + 4) u + max beta / c (|r - r_ref| <= c beta / p^2 <=
    beta / c because p > c), y within the same times max |x|.  Largest err / tol measured: 0.054 in float32, 0.025 in float64."""
    A, H = 72, 480
    c = D.find(up, nh)
    geo = D.check(c, dtype, A, H)
    T = 2 * geo["tile"] + 3
    kw = D.limiter_kwargs(c, dtype, A, H)
    P = params(dtype, **kw)
    assert (P.A, P.H, P.up) == (A, H, up) and geo["tile"] == 8193 - 2 * A - H
    x = D.over_signal((2, T), 8000 + D.CASES.index(c), dtype)
    y, g = fx().limit(dev(x), FS, return_gain=True, **kw)
    y_ref, g_ref, _ = reference(x, P)
    tol = (A + 4) * D.U[dtype] + float(D.beta(x, P.taps.numpy(), up, c.Lp).max()) / P.c
    eg = float(np.abs(g[0].cpu().numpy() - g_ref).max())
    ey = float(np.abs(y.cpu().numpy() - y_ref).max())
    print(D.case_id(c), dtype, "g err %.3e y err %.3e tol %.3e: err / tol %.3f" % (eg, ey, tol, max(eg, ey / 2.0) / tol))
    assert eg <= tol and ey <= tol * float(np.abs(x).max()), (eg, ey, tol)
    assert float(g.max()) < 0.9


# ---- the stream form ---------------------------------------------------------------------------------------------------------
STREAM_CASES = [(F32, 4, 28), (F32, 4, 61), (F32, 4, 81), (F32, 4, 83), (F32, 4, 127), (F32, 4, 189), (F32, 4, 253), (F32, 4, 256),
                (F32, 8, 187), (F64, 4, 28), (F64, 4, 83), (F64, 4, 256)]


def test_the_stream_cases_cover_what_they_should():
    f32 = [D.find(u, n) for d, u, n in STREAM_CASES if d == F32]
    assert {c.bucket for c in f32} == set(D.BUCKETS) and {c.rem for c in f32 if c.up == 4} == {0, 1, 2, 3}
    assert {D.find(u, n).bucket for d, u, n in STREAM_CASES if d == F64} == {8, 24, 72} and any(c.up == 8 for c in f32)


@case_params(STREAM_CASES)
def test_stream_chunks_plus_flush_equal_the_one_shot_result(dtype, up, nh):
    A, H = 5, 7
    c = D.find(up, nh)
    geo = D.check(c, dtype, A, H)
    tile = geo["tile"]
    n = tile + 300
    h = D.taps(c, dtype)
    x = signal((2, n), dtype, 40 + D.CASES.index(c), A, H, tile)
    ref, g = fx().limit(x, FS, return_gain=True, **kwargs(A, H, oversample=up, taps=h))
    assert float(g.min()) < 0.9 and bool((g == 1).any())
    lim = stateful(A, H, oversample=up, taps=h)
    info = D.ext().limiter_stream_plan_info(512, A, H, up, nh, dtype)
    assert lim.latency == info["latency"] == A - 1 + c.i_lo + (c.rem >= 2)
    assert lim.history_length == info["history"] == geo["history"]
    assert lim.route(x, 512).startswith("native (limiter_stream_kernel")
    for name, sizes in {"rt512": [512] * (n // 512 + 1), "random": random_sizes(n, 2, 9000)}.items():
        outs, tail = run(lim, x, sizes)
        got = torch.cat(outs + [tail], dim=-1)
        assert got.shape == ref.shape and torch.equal(got, ref), (name, int((got != ref).sum()))


@case_params([(F32, 4, 83), (F32, 4, 253)])
def test_stream_of_one_sample_chunks(dtype, up, nh):
    A, H = 5, 7
    c = D.find(up, nh)
    D.check(c, dtype, A, H)
    h = D.taps(c, dtype)
    x = signal((2, 300), dtype, 3, A, H, 10 ** 6)
    ref = fx().limit(x, FS, **kwargs(A, H, oversample=up, taps=h))
    assert not torch.equal(ref, x)
    lim = stateful(A, H, oversample=up, taps=h)
    Dl = lim.latency
    assert Dl == A - 1 + c.i_lo + 1                                            # rem >= 2: one more sample of forward reach
    outs, tail = run(lim, x, [1] * 300)
    assert [o.shape[-1] for o in outs] == [0] * Dl + [1] * (300 - Dl)
    assert torch.equal(torch.cat(outs + [tail], dim=-1), ref)


# ---- non-finite samples ------------------------------------------------------------------------------------------------------
@case_params([(F32, 4, 256), (F32, 4, 83)])
def test_non_finite_samples_at_the_new_geometries(dtype, up, nh):
    """test_gpu_limiter.test_non_finite_samples' assertions at bucket 72 and with two phases of the previous sample."""
    L = fx()
    c = D.find(up, nh)
    kw = dict(detector="true_peak", oversample=up, taps=D.taps(c, dtype))
    P = params(dtype, **kw)
    info = D.ext().limiter_plan_info(1, P.A, P.H, up, nh, dtype)
    geo = D.check(c, dtype, P.A, P.H)
    assert (info["halo_left"], info["halo_right"]) == (geo["halo_left"], geo["halo_right"])
    tile, reach = info["tile"], info["halo_left"] + info["halo_right"] + info["tile"]
    T = 3 * tile + 100
    x = dev(loud((3, 2, T), 31, dtype))
    clean = L.limit(x, FS, **kw)
    assert not bool(torch.isnan(clean).any())
    n = torch.arange(T, device=DEV)
    for bad in (math.nan, math.inf):
        for pos in (tile + 5, 0, T - 1):
            xb = x.clone()
            xb[1, 0, pos] = bad
            y = L.limit(xb, FS, **kw)
            assert bool(torch.isnan(y[1, :, pos]).all()), (bad, pos)          # NaN in every channel of its group
            far = (n - pos).abs() > reach
            assert bool(far.any()) and torch.equal(y[1][:, far], clean[1][:, far]), (bad, pos)
            assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2])    # the other groups never see it
