"""The look-ahead limiter on the device (csrc/limiter.hip through torchfx_ext.limiter_forward): bit equality with a torch
composition where the definition is exact, the float64 restatement (tests/limiter_reference.py) where it is not, the
properties that follow from the definition, the true peak of the result, independence of the batch and non-finite samples.
Shapes come from limiter_plan_info (tile seams, a halo longer than a tile), never from the workload."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import limiter_reference as R
from tests.gpu_common import DEV, TOL_CONV_F32, TOL_CONV_F64, dev, ext
from tests.test_limiter_host import FS, NP, U, noise, params, reference, tp_signals

pytestmark = pytest.mark.gpu


def fx():
    import torchfx_amd
    return torchfx_amd


def plan(T, P, dtype):
    return ext().limiter_plan_info(T, P.A, P.H, P.up, 0 if P.taps is None else int(P.taps.numel()), dtype)


def windowed_min_ext(r, A, H):
    """``m[k] = min r[k-H+1 .. k+A-1]`` (r = 1 outside) for k in [-(A-1), T): [..., T + A - 1], exact, in torch."""
    pad = torch.nn.functional.pad(r, (H - 1 + A - 1, A - 1), value=1.0)
    return pad.unfold(-1, A + H - 1, 1).amin(-1)


def expected_one_hot(x, P, link, j0):
    """The limiter with a one-hot window at j0 (A = 1: j0 = 0) from ops that are exact or rounded once: returns (y, g)."""
    T = x.shape[-1]
    p = x.abs()
    if P.up > 1:
        v = fx().resample_poly(x, P.up, 1, window=(P.taps / P.up).numpy()).abs()
        q = v.reshape(*x.shape, P.up).amax(-1)
        p = torch.maximum(torch.maximum(p, q), torch.nn.functional.pad(q, (1, 0))[..., :-1])
    channels = x.shape[-2] if (link and x.dim() >= 2) else 1
    p = p.reshape(-1, channels, T).amax(1)                                   # [groups, T]
    pn, c = p.cpu().numpy(), NP[x.dtype](P.c)
    with np.errstate(divide="ignore"):
        r = dev(np.where(pn > c, c / pn, NP[x.dtype](1)).astype(NP[x.dtype]))   # IEEE division on the host
    m = windowed_min_ext(r, P.A, P.H)[..., P.A - 1 - j0:P.A - 1 - j0 + T]      # m[n - j0]
    g = torch.minimum(1 - (1 - m), r)
    return (g.unsqueeze(1) * x.reshape(-1, channels, T)).reshape(x.shape), g


SHAPES = [((), True), ((2,), True), ((2,), False), ((2, 2), True), ((2, 2), False)]


def loud(shape, seed, dtype):
    """Uniform noise at 0.5 with bursts up to 3: most of the signal under the ceiling, the rest well over it."""
    x = noise(shape, seed, 0.5, NP[dtype])
    T = shape[-1]
    g = np.random.default_rng(seed + 1)
    for _ in range(max(1, T // 700)):
        s = int(g.integers(0, T))
        x[..., s:s + int(g.integers(1, 40))] *= 6.0
    return x


# ---- bit equality where the definition allows it ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("up", [1, 2, 4])
def test_bit_equal_with_a_look_ahead_of_one(dtype, up):
    """A = 1: step 5 is the single product 1 * (1 - m); everything else is exact or rounded once."""
    k = 0
    for H in (1, 2, 480, 4096):
        P = params(dtype, lookahead=0.0, hold=H / FS, detector="true_peak" if up > 1 else "sample", oversample=up)
        assert (P.A, P.H, P.up) == (1, H, up)
        tile = plan(1, P, dtype)["tile"]
        assert tile == 8193 - 2 - H
        for T in (1, 2, H, tile - 1, tile, tile + 1, 2 * tile + 3):
            lead, link = SHAPES[k % len(SHAPES)]
            k += 1
            x = dev(loud(lead + (T,), 100 + k, dtype))
            y, g = fx().limit(x, FS, lookahead=0.0, hold=H / FS, oversample=up, detector="true_peak" if up > 1 else "sample",
                              link=link, return_gain=True)
            ye, ge = expected_one_hot(x, P, link, 0)
            assert torch.equal(g, ge), (H, T, lead, link, float((g - ge).abs().max()))
            assert torch.equal(y, ye), (H, T, lead, link)
            assert T < 100 or float(g.min()) < 0.9              # the limiter did work


@pytest.mark.parametrize("dtype,up", [(torch.float32, 1), (torch.float32, 4), (torch.float64, 1), (torch.float64, 2)])
def test_bit_equal_with_a_one_hot_window(dtype, up):
    """g[n] = min(1 - fl(1 - m[n - j0]), r[n]) exactly: the smoothing loop's indexing across every tile seam, and a halo
    longer than a tile (A, H = 512, 4096)."""
    k = 0
    for A, H in ((2, 1), (72, 480), (512, 4096)):
        for j0 in sorted({0, 1, A - 1}):
            w = np.zeros(A)
            w[j0] = 0.25
            kw = dict(lookahead=A / FS, hold=H / FS, detector="true_peak" if up > 1 else "sample", oversample=up)
            P = params(dtype, window=w, **kw)
            assert (P.A, P.H) == (A, H) and float(P.w[j0]) == 1.0
            tile = plan(1, P, dtype)["tile"]
            lead, link = SHAPES[k % len(SHAPES)]
            k += 1
            T = 2 * tile + 3
            x = dev(loud(lead + (T,), 300 + k, dtype))
            y, g = fx().limit(x, FS, window=w, link=link, return_gain=True, **kw)
            ye, ge = expected_one_hot(x, P, link, j0)
            assert torch.equal(g, ge), (A, H, j0, lead, link, float((g - ge).abs().max()))
            assert torch.equal(y, ye)
            assert float(g.min()) < 0.9


# ---- against the float64 reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("detector", ["sample", "true_peak"])
def test_default_window_against_the_reference(dtype, detector):
    """|g - g_ref| <= (A + 4) u (A fma, two subtractions, the rounding of w, the division) -- plus the interpolator's float error,
    the project's figure against SciPy, with the oversampled detector; y within the same times max |x|."""
    for A, H in ((72, 480), (67, 442), (512, 4096)):
        kw = dict(lookahead=A / FS, hold=H / FS, detector=detector)
        P = params(dtype, **kw)
        assert (P.A, P.H) == (A, H)
        tile = plan(1, P, dtype)["tile"]
        T = 2 * tile + 3
        x = noise((2, T), 40 + A, 0.3, NP[dtype])
        for i, n in enumerate((0, 1, tile - 1, tile, tile + 1, T - 1)):       # lone peaks
            x[i % 2, n] = 2.0 + 0.25 * i
        y, g = fx().limit(dev(x), FS, return_gain=True, **kw)
        y_ref, g_ref, _ = reference(x, P)
        tol = (A + 4) * U[dtype] + (0.0 if detector == "sample" else TOL_CONV_F32 if dtype == torch.float32 else TOL_CONV_F64)
        eg = float(np.abs(g[0].cpu().numpy() - g_ref).max())
        ey = float(np.abs(y.cpu().numpy() - y_ref).max())
        print(dtype, detector, A, H, "g err %.3e y err %.3e tol %.3e" % (eg, ey, tol))
        assert eg <= tol and ey <= tol * float(np.abs(x).max()), (A, H, eg, ey, tol)
        assert float(g.min()) < 0.5


# ---- properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_properties_on_the_device(dtype):
    L = fx()
    P = params(dtype)
    tile = plan(1, P, dtype)["tile"]
    T = tile + 777
    quiet = dev(noise((2, T), 3, 0.4, NP[dtype]))
    quiet[1, 17] = -0.0
    for det in ("sample", "true_peak"):                                        # transparent, bit for bit
        y, g = L.limit(quiet, FS, detector=det, return_gain=True)
        assert torch.equal(y, quiet) and bool(torch.signbit(y[1, 17])) and bool((g == 1).all())
    x = dev(loud((2, T), 5, dtype))
    for det in ("sample", "true_peak"):
        y, g = L.limit(x, FS, detector=det, return_gain=True)
        assert Fraction(float(y.abs().max())) <= Fraction(P.c) * (1 + Fraction(U[dtype])) ** 2          # sample ceiling
        assert float(y.abs().max()) > 0.9 * P.c and g.shape == (1, T)
        assert torch.equal(y, g * x)                                           # linked: one curve for both channels
        nz = x != 0
        ratio = (y.to(torch.float64) / x.to(torch.float64))[nz]                # return_gain is y / x to the product's rounding
        assert float((ratio - g.expand(2, T).to(torch.float64)[nz]).abs().max()) <= U[dtype]
        yu, gu = L.limit(x, FS, detector=det, link=False, return_gain=True)   # unlinked: every row on its own
        for ch in range(2):
            yc, gc = L.limit(x[ch], FS, detector=det, return_gain=True)
            assert torch.equal(yu[ch], yc) and torch.equal(gu[ch:ch + 1], gc)
        assert not torch.equal(gu[0], gu[1])


def test_time_course_on_the_device():
    A, H, n0 = 72, 480, 9000                                                  # the peak sits behind the first tile seam (7569)
    x = torch.zeros(12000, device=DEV)
    x[n0] = 2.0
    g = fx().limit(x, FS, detector="sample", return_gain=True)[1][0].cpu().numpy().astype(np.float64)
    r0 = float(np.float32(10 ** -0.05) / np.float32(2.0))
    assert (g[:n0 - A + 1] == 1).all() and g[n0 - A + 1] < 1 and (g[n0 + H + A - 1:] == 1).all() and g[n0 + H + A - 2] < 1
    assert g[n0] <= r0 and np.abs(g[n0:n0 + H] - r0).max() <= (A + 4) * 2.0 ** -24


# ---- the true peak of the result ---------------------------------------------------------------------------------------
def test_true_peak_of_the_result():
    """The device's float32 result reads no more than the float64 reference's own output + 1e-3 dB (the margin of float32
    against float64 readings in test_loudness_normalize_ceiling_on_the_device)."""
    L = fx()
    P = params(torch.float32)
    h = P.taps.numpy().astype(np.float64)
    for name, x in tp_signals().items():
        ref_db = R.true_peak_db(reference(x, P)[0], 4, h)
        got = float(L.true_peak(L.limit(dev(x), FS), FS).max())
        print(name, "device %.5f dBTP, reference %.5f dBTP" % (got, ref_db))
        assert got <= ref_db + 1e-3, (name, got, ref_db)
        assert got > -1.5


def programme():
    """Three seconds of a stereo 997 Hz tone with six 5-sample clicks 16 dB over it, alternating between the channels."""
    n = np.arange(3 * FS)
    s = 0.1 * np.sin(2 * np.pi * 997 * n / FS)
    x = np.stack([s, 0.8 * s])
    for k in range(6):
        p = 12000 + 24000 * k
        x[k % 2, p:p + 5] += 0.6 * np.hanning(7)[1:6]
    return x.astype(np.float32)


def test_mastering_chain_on_the_device():
    """wave | LoudnessNormalize(-14) | Limiter(-1.0).  Normalised to -14 LUFS the programme reads +3.69 dBTP; the float64
    reference on the CPU limits it to -1.0000 dBTP and -14.073 LUFS (the gain is down for 12 ms around six clicks: 0.07 LU),
    so 0.5 LU is a wide bound."""
    L = fx()
    x = dev(programme())
    out = L.Wave(x, FS, device=DEV) | L.LoudnessNormalize(-14.0) | L.Limiter(-1.0)
    tp, lufs = out.true_peak(), out.loudness()
    print("true peak %.5f dBTP, loudness %.4f LUFS" % (tp, lufs))
    assert tp <= -1.0 + 1e-3
    assert abs(lufs - (-14.0)) <= 0.5
    before = L.Wave(x, FS, device=DEV) | L.LoudnessNormalize(-14.0)
    assert before.true_peak() > 3.0                                           # the limiter had 4.7 dB to take down


# ---- independence and repeatability ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batch_independence_and_views(dtype):
    L = fx()
    tile = plan(1, params(dtype), dtype)["tile"]
    T = tile + 1234
    x = dev(loud((3, 2, T), 21, dtype))
    y, g = L.limit(x, FS, return_gain=True)
    y2, g2 = L.limit(x, FS, return_gain=True)
    assert torch.equal(y, y2) and torch.equal(g, g2)                         # two calls are equal
    for b in range(3):                                                        # a batch is the stack of its groups run alone
        yb, gb = L.limit(x[b], FS, return_gain=True)
        assert torch.equal(y[b], yb) and torch.equal(g[b:b + 1], gb)
    wide = dev(loud((3, 2, 2 * T), 22, dtype))
    view = wide[..., ::2]
    assert not view.is_contiguous() and torch.equal(L.limit(view, FS), L.limit(view.contiguous(), FS))
    tr = dev(loud((T, 2), 23, dtype)).t()
    assert not tr.is_contiguous() and torch.equal(L.limit(tr, FS), L.limit(tr.contiguous(), FS))


@pytest.mark.parametrize("dtype,detector", [(torch.float32, "true_peak"), (torch.float64, "true_peak"), (torch.float32, "sample")])
def test_non_finite_samples(dtype, detector):
    L = fx()
    P = params(dtype, detector=detector)
    info = plan(1, P, dtype)
    tile, reach = info["tile"], info["halo_left"] + info["halo_right"] + info["tile"]
    T = 3 * tile + 100
    x = dev(loud((3, 2, T), 31, dtype))
    clean = L.limit(x, FS, detector=detector)
    n = torch.arange(T, device=DEV)
    for bad in (math.nan, math.inf):
        for pos in (tile + 5, 0, T - 1):
            xb = x.clone()
            xb[1, 0, pos] = bad
            y = L.limit(xb, FS, detector=detector)
            assert bool(torch.isnan(y[1, :, pos]).all()), (bad, pos)          # NaN in every channel of its group
            far = (n - pos).abs() > reach
            assert bool(far.any()) and torch.equal(y[1][:, far], clean[1][:, far]), (bad, pos)
            assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2])    # the other groups never see it


# ---- planner and errors ------------------------------------------------------------------------------------------------
def test_route_names_the_kernel():
    L = fx()
    x = dev(noise((2, 24000), 1, 0.9))
    w = L.Wave(x, FS, device=DEV) | L.Gain(2.0) | L.Limiter(-1.0)
    lines = w.explain()
    assert any(ln.startswith("Limiter: native (limiter_kernel, 4x oversampled detector") and "4 tile(s)" in ln for ln in lines), lines
    assert "limiter_kernel" in L.Limiter(-1.0, detector="sample", fs=FS).route(x) and "sample-peak" in L.Limiter(-1.0, detector="sample", fs=FS).route(x)
    assert torch.equal(w.ys, L.limit(x * 2.0, FS))


def test_argument_errors_on_the_device_match_the_cpu_path():
    L = fx()
    for kw in (dict(ceiling_db=math.nan), dict(lookahead=-1e-3), dict(hold=4097 / FS), dict(lookahead=513 / FS), dict(window=np.ones(3)),
               dict(window=np.zeros(72)), dict(detector="rms"), dict(oversample=3)):
        msgs = []
        for device in ("cpu", DEV):
            with pytest.raises(ValueError) as e:
                L.limit(torch.zeros(2, 1000, device=device), FS, **kw)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], kw
    with pytest.raises(TypeError, match="float32 or float64"):
        L.limit(torch.zeros(2, 100, device=DEV, dtype=torch.float16), FS)
    y, g = L.limit(torch.zeros(2, 0, device=DEV), FS, return_gain=True)
    assert y.shape == (2, 0) and g.shape == (1, 0) and y.device.type == "cuda"
    E = ext()
    with pytest.raises(RuntimeError, match="512"):
        E.limiter_forward(torch.zeros(2, 100, device=DEV), 0.89, 513, 1, torch.ones(513), 1, None, 1, False)
    with pytest.raises(RuntimeError, match="groups of 3"):
        E.limiter_forward(torch.zeros(2, 100, device=DEV), 0.89, 1, 1, torch.ones(1), 1, None, 3, False)
