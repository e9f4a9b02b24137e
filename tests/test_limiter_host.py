"""The look-ahead limiter without a GPU: the CPU path of torchfx_amd.limiter against the float64 restatement
(tests/limiter_reference.py), the properties that follow from the definition, Limiter in a Wave pipeline, the planner, the
stream refusals, the host-only half of the C ABI, and the true-peak figures the documentation quotes."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import limiter_reference as R
from tests.gpu_common import TOL_CONV_F32, TOL_CONV_F64
from tests.truepeak_signals import accent_tone, tone

FS = 48000
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
NP = {torch.float32: np.float32, torch.float64: np.float64}


def fx():
    import torchfx_amd
    return torchfx_amd


def params(dtype, **kw):
    from torchfx_amd.limiter import LimiterParams
    return LimiterParams(FS, dtype, **kw)


def reference(x, P):
    """tests/limiter_reference on one group ``x [C, T]`` with the call's rounded parameters."""
    h = None if P.taps is None else P.taps.numpy().astype(np.float64)
    return R.limit_reference(np.asarray(x, dtype=np.float64), P.c, P.A, P.H, P.w.astype(np.float64), P.up, h)


def noise(shape, seed, scale, dtype=np.float32):
    return (np.random.default_rng(seed).uniform(-1, 1, shape) * scale).astype(dtype)


# ---- the CPU path against the reference ---------------------------------------------------------------------------------
# The CPU path multiplies and adds where the definition has one fma: 2A roundings in the sum instead of A, each of at most u
# (the partial sums stay below ~1), plus the two subtractions, the rounding of w and the division: (2A + 4) u.  With the
# oversampled detector the interpolator's float error comes on top, the project's figure against SciPy (TOL_CONV_*).
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("detector", ["sample", "true_peak"])
def test_cpu_path_matches_the_reference(dtype, detector):
    tol_conv = 0.0 if detector == "sample" else (TOL_CONV_F32 if dtype == torch.float32 else TOL_CONV_F64)
    for shape, ngroups, kw in [((3000,), 1, {}), ((2, 2500), 1, dict(lookahead=67 / FS, hold=442 / FS)),
                               ((2, 2, 1200), 2, dict(lookahead=8 / FS, hold=2 / FS))]:
        x = torch.from_numpy(noise(shape, 11, 1.5, NP[dtype]))
        P = params(dtype, detector=detector, **kw)
        y, g = fx().limit(x, FS, detector=detector, return_gain=True, **kw)
        assert y.shape == x.shape and y.dtype == dtype and g.dtype == dtype and g.shape == (ngroups, shape[-1])
        groups = x.numpy().reshape(g.shape[0], -1, x.shape[-1])
        tol = (2 * P.A + 4) * U[dtype] + tol_conv
        for k in range(g.shape[0]):
            y_ref, g_ref, _ = reference(groups[k], P)
            assert np.abs(g[k].numpy() - g_ref).max() <= tol, (shape, k)
            assert np.abs(y.numpy().reshape(groups.shape)[k] - y_ref).max() <= tol * np.abs(groups[k]).max()


# ---- what follows from the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_transparent_below_the_ceiling_bit_for_bit(dtype):
    x = torch.from_numpy(noise((2, 6000), 3, 0.4, NP[dtype]))           # true peak of uniform noise at 0.4 stays under 0.89
    x[1, 17] = -0.0
    for det in ("sample", "true_peak"):
        y, g = fx().limit(x, FS, detector=det, return_gain=True)
        assert torch.equal(y, x) and math.copysign(1.0, float(y[1, 17])) == -1.0
        assert bool((g == 1).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sample_ceiling(dtype):
    x = torch.from_numpy(noise((2, 8000), 5, 3.0, NP[dtype]))
    for det, kw in (("sample", {}), ("true_peak", {}), ("sample", dict(lookahead=0.0, hold=0.0))):
        P = params(dtype, detector=det, **kw)
        y = fx().limit(x, FS, detector=det, **kw)
        assert Fraction(float(y.abs().max())) <= Fraction(P.c) * (1 + Fraction(U[dtype])) ** 2, det      # exact: 1 + 2^-53 is no float
        assert float(y.abs().max()) > 0.5 * P.c


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_time_course_of_a_lone_peak(dtype):
    T, n0 = 4000, 1500
    x = torch.zeros(T, dtype=dtype)
    x[n0] = 2.0
    for A, H in ((72, 480), (5, 1), (1, 7)):
        P = params(dtype, detector="sample", lookahead=A / FS, hold=H / FS)
        assert (P.A, P.H) == (A, H)
        _, g = fx().limit(x, FS, detector="sample", lookahead=A / FS, hold=H / FS, return_gain=True)
        g = g[0].numpy().astype(np.float64)
        r0 = float(NP[dtype](P.c) / NP[dtype](2.0))
        assert (g[:n0 - A + 1] == 1).all() and g[n0 - A + 1] < 1                  # starts falling at n0 - A + 1
        assert np.all(np.diff(g[n0 - A:n0 + 1]) <= 0)                              # ... and falls monotonically
        hold = g[n0:n0 + H]
        assert g[n0] <= r0 and np.abs(hold - r0).max() <= (2 * A + 4) * U[dtype]  # r[n0] from n0 through n0 + H - 1
        assert (g[n0 + H + A - 1:] == 1).all()                                     # back at exactly 1
        if A > 1:
            assert g[n0 + H + A - 2] < 1


def test_linked_and_unlinked_stereo():
    x = torch.from_numpy(noise((2, 5000), 7, 1.0))
    x[0] *= 0.3                                        # the quiet channel never passes the ceiling on its own
    x[1, 2000:2100] *= 2.0
    L = fx()
    y, g = L.limit(x, FS, return_gain=True)
    assert g.shape == (1, 5000) and float(g.min()) < 0.8
    assert torch.equal(y, g * x)                       # one curve for both channels
    yu, gu = L.limit(x, FS, link=False, return_gain=True)
    assert gu.shape == (2, 5000) and bool((gu[0] == 1).all()) and torch.equal(yu[0], x[0])
    for ch in range(2):
        yc, gc = L.limit(x[ch], FS, return_gain=True)
        assert torch.equal(yu[ch], yc) and torch.equal(gu[ch:ch + 1], gc)
    assert torch.equal(gu[1:2], g)                     # the loud channel alone drives the linked curve here
    xb = torch.stack([x, x.flip(0) * 0.5])
    yb, gb = L.limit(xb, FS, return_gain=True)
    assert gb.shape == (2, 5000) and torch.equal(yb[0], y) and torch.equal(yb[1], L.limit(xb[1], FS))
    assert L.limit(xb, FS, link=False, return_gain=True)[1].shape == (4, 5000)


def test_argument_errors():
    L = fx()
    x = torch.zeros(2, 1000)
    for kw, exc, what in [
        (dict(ceiling_db=math.nan), ValueError, "ceiling_db"), (dict(ceiling_db=-math.inf), ValueError, "ceiling_db"),
        (dict(lookahead=-1e-3), ValueError, "lookahead"), (dict(hold=-1.0), ValueError, "hold"),
        (dict(lookahead=513 / FS), ValueError, "limit of 512"), (dict(hold=4097 / FS), ValueError, "limit of 4096"),
        (dict(window=np.ones(71)), ValueError, "A = 72"), (dict(window=-np.ones(72)), ValueError, ">= 0"),
        (dict(window=np.full(72, np.nan)), ValueError, "finite"), (dict(window=np.zeros(72)), ValueError, "sum to 0"),
        (dict(detector="rms"), ValueError, "detector"), (dict(oversample=3), ValueError, "oversample"),
        (dict(taps=np.ones(4 * 64 + 1)), ValueError, "taps"),
    ]:
        with pytest.raises(exc, match=what):
            L.limit(x, FS, **kw)
    with pytest.raises(TypeError, match="float32 or float64"):
        L.limit(torch.zeros(2, 100, dtype=torch.int16), FS)
    with pytest.raises(TypeError, match="float32 or float64"):
        L.limit(torch.zeros(2, 100, dtype=torch.float16), FS)
    with pytest.raises(TypeError, match="torch.Tensor"):
        L.limit(np.zeros(100), FS)
    with pytest.raises(ValueError, match=r"\[T\], \[C, T\], or \[B, C, T\]"):
        L.limit(torch.zeros(1, 1, 2, 100), FS)
    with pytest.raises(ValueError, match="fs"):
        L.limit(x, 44100.0)
    y, g = L.limit(torch.zeros(2, 0), FS, return_gain=True)
    assert y.shape == (2, 0) and g.shape == (1, 0)
    assert L.limit(torch.zeros(3, 2, 0, dtype=torch.float64), FS).shape == (3, 2, 0)
    # an accepted caller's window: one-hot at j0 delays the reduction by j0 and nothing else
    w = np.zeros(72)
    w[5] = 3.0
    xs = torch.zeros(600, dtype=torch.float64)
    xs[300] = 2.0
    g = L.limit(xs, FS, detector="sample", window=w, hold=0.0, return_gain=True)[1][0]
    r0 = float(np.float64(10 ** -0.05) / 2.0)
    assert r0 - 2.0 ** -52 <= float(g[300]) <= r0 and bool((g[:300 - 71 + 5] == 1).all()) and float(g[300 - 71 + 5]) < 1


# ---- pipeline, planner, streams ---------------------------------------------------------------------------------------
def test_limiter_in_a_wave_pipeline(oracle_backend):
    from torchfx_amd import filter as F
    from torchfx_amd.effect import Gain
    L = fx()
    x = torch.from_numpy(noise((2, 24000), 13, 0.9))
    lim = L.Limiter(-3.0)
    w = L.Wave(x, FS) | F.HiButterworth(100, order=2) | F.LoButterworth(8000, order=2) | lim | Gain(0.5)
    assert lim.fs == FS                                 # the rate comes from the Wave
    names = [type(m.producer).__name__ if type(m).__name__ == "Epilogued" else type(m).__name__ for m in w.plan()]
    assert names[:2] == ["FusedSOSCascade", "Limiter"] and "Limiter" not in names[2:], names
    assert type(w.plan()[1]).__name__ == "Limiter"     # a step of its own: nothing attached to it, nothing merged across it
    assert any(ln.startswith("Limiter: numpy on host -- cpu tensor") for ln in w.explain()), w.explain()
    out = L.Wave(x * 2, FS) | L.Limiter(-3.0, detector="sample")
    c = float(np.float32(10 ** (-3.0 / 20)))
    assert Fraction(float(out.ys.abs().max())) <= Fraction(c) * (1 + Fraction(2.0 ** -24)) ** 2 and float(out.ys.abs().max()) > 0.9 * c
    assert torch.equal(out.ys, L.limit(x * 2, FS, -3.0, detector="sample"))
    # the parameters are part of the plan: another ceiling is another result
    a = (L.Wave(x * 2, FS) | L.Limiter(-3.0, detector="sample")).ys
    b = (L.Wave(x * 2, FS) | L.Limiter(-9.0, detector="sample")).ys
    assert float(b.abs().max()) < 0.6 * float(a.abs().max())
    with pytest.raises(ValueError, match="sample rate"):
        L.Limiter()(x)
    with pytest.raises(ValueError, match="ceiling_db"):
        L.Limiter(math.nan)
    with pytest.raises(ValueError, match="lookahead"):
        L.Limiter(lookahead=-1.0)
    assert "Limiter" in fx().__all__ and "limit" in fx().__all__


def test_streams_refuse_the_limiter():
    from torchfx_amd import filter as F
    from torchfx_amd.realtime import AudioBackend, RealtimeProcessor, StreamConfig, StreamProcessor
    lim = fx().Limiter(-1.0, fs=FS)

    class Nested(fx().FX):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x)

    class NoBackend(AudioBackend):
        def open_stream(self, config, callback=None):
            raise AssertionError("the refusal comes before a stream is opened")

        def start(self):
            pass

        def stop(self):
            pass

        def close(self):
            pass

    for effects in ([lim], [F.HiButterworth(100, fs=FS), Nested(lim)]):
        with pytest.raises(TypeError, match=r"looks A - 1 samples ahead.*streaming limiter.*not provided"):
            StreamProcessor(effects, chunk_size=4096, device="cpu")
        with pytest.raises(TypeError, match=r"looks A - 1 samples ahead.*streaming limiter.*not provided"):
            RealtimeProcessor(effects, NoBackend(), StreamConfig(), device="cpu")


# ---- C ABI, host only ----------------------------------------------------------------------------------------------------
def test_plan_info_runs_without_a_device():
    from torchfx_amd import _lib
    from torchfx_amd import torchfx_ext as E
    info = E.limiter_plan_info(2_880_000, 72, 480, 4, 81)
    assert info["tile"] == 8193 - 2 * 72 - 480 and info["tiles"] == -(-2_880_000 // info["tile"]) and info["Lp"] == 21
    assert info["halo_left"] >= 72 + 480 - 1 + 10 and info["halo_right"] >= 72 - 1 + 10
    assert 0 < info["lds_bytes"] <= 80 * 1024                                        # two workgroups per CU
    assert E.limiter_plan_info(2_880_000, 72, 480, 4, 81, groups=32, channels=2) == info      # the tiling does not depend on the batch
    wide = E.limiter_plan_info(100_000, 512, 4096, 8, 161, torch.float64)
    assert wide["tile"] == 8193 - 1024 - 4096 and wide["tile"] < 512 + 4096 - 1      # the halo is longer than the tile
    assert wide["lds_bytes"] <= 160 * 1024
    sample = E.limiter_plan_info(5, 1, 1, 1, 0)
    assert sample == {"tile": 8190, "tiles": 1, "halo_left": 1, "halo_right": 1, "Lp": 0, "lds_bytes": info["lds_bytes"]}
    assert E.limiter_plan_info(0, 72, 480)["tiles"] == 0
    for bad, what in [(dict(A=513), "512"), (dict(H=4097), "4096"), (dict(A=0), "look-ahead"), (dict(H=0), "hold"), (dict(up=3), "up must be"),
                      (dict(up=4, taps=257), "64 \\* up"), (dict(up=2, taps=0), "no taps"), (dict(length=-1), "negative")]:
        kw = dict(length=1000, A=72, H=480, up=1, taps=0)
        kw.update(bad)
        with pytest.raises(RuntimeError, match=what):
            E.limiter_plan_info(**kw)
    lib = _lib.load()
    w = (ctypes.c_float * 72)(*([1.0 / 72] * 72))
    neg = (ctypes.c_float * 72)(*([-1.0] * 72))
    o = [ctypes.c_int64(0) for _ in range(6)]
    refs = [ctypes.byref(v) for v in o]
    cases = [
        lib.tfx_limiter_forward(None, None, None, 0, 2, 2, 100, 0.89, 72, 480, w, 1, None, 0, None),        # null signal
        lib.tfx_limiter_forward(None, None, None, 7, 0, 2, 100, 0.89, 72, 480, w, 1, None, 0, None),        # bad dtype
        lib.tfx_limiter_forward(None, None, None, 0, 0, 2, 100, 0.0, 72, 480, w, 1, None, 0, None),         # ceiling 0
        lib.tfx_limiter_forward(None, None, None, 0, 0, 2, 100, math.nan, 72, 480, w, 1, None, 0, None),
        lib.tfx_limiter_forward(None, None, None, 0, 0, 2, 100, 0.89, 72, 480, None, 1, None, 0, None),     # no window
        lib.tfx_limiter_forward(None, None, None, 0, 0, 2, 100, 0.89, 72, 480, neg, 1, None, 0, None),      # negative weight
        lib.tfx_limiter_forward(None, None, None, 0, 0, 2, 100, 0.89, 513, 480, w, 1, None, 0, None),
        lib.tfx_limiter_forward(None, None, None, 0, 0, 0, 100, 0.89, 72, 480, w, 1, None, 0, None),        # no channels
        lib.tfx_limiter_forward(None, None, None, 0, 0, 2, 100, 0.89, 72, 480, w, 4, None, 81, None),       # up > 1 without taps
        lib.tfx_limiter_plan_info(1, 1, 100, 72, 480, 1, 0, 0, None, *refs[1:]),                            # null output
        lib.tfx_limiter_plan_info(1, 1, 100, 72, 4097, 1, 0, 0, *refs),
    ]
    assert all(rc != 0 for rc in cases), cases
    assert b"limiter" in lib.tfx_last_error()
    assert lib.tfx_limiter_forward(None, None, None, 0, 0, 2, 100, 0.89, 72, 480, w, 1, None, 0, None) == 0   # empty work touches nothing
    assert lib.tfx_limiter_forward(None, None, None, 0, 3, 2, 0, 0.89, 72, 480, w, 1, None, 0, None) == 0


# ---- the true peak of the result: measured, not guaranteed -----------------------------------------------------------
def tp_signals():
    """The three signals of the true-peak checks (float32, [C, T]); tests/test_gpu_limiter.py limits the same ones on the device."""
    return {"accent": accent_tone()[None] * np.float32(10.0), "tone": tone(4, 45.0)[None] * np.float32(2.8),
            "noise": noise((2, 12000), 0, 1.5)}


@pytest.fixture(scope="module")
def tp_readings():
    """name -> dB over the ceiling of the float64 reference's own output at the defaults (A, H = 72, 480)."""
    P = params(torch.float32)
    assert (P.A, P.H, P.up) == (72, 480, 4)
    h = P.taps.numpy().astype(np.float64)
    return {k: R.true_peak_db(reference(x, P)[0], 4, h) - 20 * math.log10(P.c) for k, x in tp_signals().items()}, P


def test_true_peak_of_the_reference_output_at_the_defaults(tp_readings):
    """Measured: accent +0.0000, tone +0.0000, noise +0.00015 dB over the ceiling (the issue's prototype figures)."""
    over, _ = tp_readings
    print({k: round(v, 6) for k, v in over.items()})
    for k, v in over.items():
        assert v <= 1e-3, (k, v)
    assert min(over.values()) > -0.5                  # ... and the limiter did not simply turn everything down


def test_a_short_lookahead_overshoots_the_true_peak():
    """The documented caveat is real: at A, H = 8, 2 the noise reads more than 0.1 dB over the ceiling (measured +0.27 dB)."""
    P = params(torch.float32, lookahead=8 / FS, hold=2 / FS)
    assert (P.A, P.H) == (8, 2)
    h = P.taps.numpy().astype(np.float64)
    over = R.true_peak_db(reference(tp_signals()["noise"], P)[0], 4, h) - 20 * math.log10(P.c)
    print(round(over, 4))
    assert over > 0.1
    got = float(fx().true_peak(fx().limit(torch.from_numpy(tp_signals()["noise"]), FS, lookahead=8 / FS, hold=2 / FS), FS).max())
    assert got - 20 * math.log10(P.c) > 0.1           # the library's CPU path shows the same
