"""Zero-phase filtering without a device: the SciPy route of CPU tensors, argument errors, the ZeroPhase effect in the
planner and the streaming refusals, the steady-state start of the device kernel restated in DF1, and the host-only entry
points of the C ABI (tfx_sos_filtfilt_plan_info, argument checks of tfx_sos_filtfilt_forward)."""
import ctypes

import numpy as np
import pytest
import scipy.signal as ss
import torch

PADTYPES = ["odd", "even", "constant", None]


def fx():
    import torchfx_amd
    return torchfx_amd


def F():
    from torchfx_amd import filter as flt
    return flt


def sig(shape, seed, dtype=np.float64):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(dtype)


SOS = ss.butter(4, 1000, fs=48000, output="sos")


@pytest.mark.parametrize("padtype", PADTYPES)
@pytest.mark.parametrize("shape", [(500,), (3, 500), (2, 3, 500)])
def test_cpu_tensors_equal_scipy(shape, padtype):
    x = sig(shape, len(shape))
    y = fx().sosfiltfilt(torch.from_numpy(x), SOS, padtype=padtype)
    assert y.dtype == torch.float64 and y.shape == x.shape
    assert np.array_equal(y.numpy(), ss.sosfiltfilt(SOS, x, axis=-1, padtype=padtype))
    x32 = x.astype(np.float32)
    y32 = fx().sosfiltfilt(torch.from_numpy(x32), torch.from_numpy(SOS), padtype=padtype)
    assert y32.dtype == torch.float32
    assert np.array_equal(y32.numpy(), ss.sosfiltfilt(SOS, x32.astype(np.float64), axis=-1, padtype=padtype).astype(np.float32))


def test_padlen_edge_and_errors():
    from torchfx_amd.filtfilt import default_padlen
    pad = default_padlen(SOS)
    assert pad == 3 * (2 * 2 + 1 - min(int((SOS[:, 2] == 0).sum()), int((SOS[:, 5] == 0).sum())))
    x = sig((2, pad + 1), 3)
    assert np.array_equal(fx().sosfiltfilt(torch.from_numpy(x), SOS).numpy(), ss.sosfiltfilt(SOS, x, axis=-1))
    with pytest.raises(ValueError, match=f"The length of the input vector x must be greater than padlen, which is {pad}."):
        fx().sosfiltfilt(torch.from_numpy(x[:, :pad]), SOS)
    with pytest.raises(ValueError, match="must be greater than padlen, which is 40"):
        fx().sosfiltfilt(torch.from_numpy(x[:, :40]), SOS, padlen=40)
    # explicit padlen, and padtype None ignores it
    x = sig((2, 300), 4)
    for kw in [dict(padlen=0), dict(padlen=100), dict(padtype=None, padlen=7), dict(padtype="even", padlen=31)]:
        assert np.array_equal(fx().sosfiltfilt(torch.from_numpy(x), SOS, **kw).numpy(), ss.sosfiltfilt(SOS, x, axis=-1, **kw))
    with pytest.raises(ValueError, match="padtype"):
        fx().sosfiltfilt(torch.from_numpy(x), SOS, padtype="reflect")
    with pytest.raises(ValueError, match="padlen"):
        fx().sosfiltfilt(torch.from_numpy(x), SOS, padlen=-1)
    with pytest.raises(ValueError):
        fx().sosfiltfilt(torch.from_numpy(x), SOS[:, :5])
    with pytest.raises(ValueError):
        fx().sosfiltfilt(torch.zeros(2, 2, 2, 300), SOS)
    with pytest.raises(TypeError):
        fx().sosfiltfilt(x, SOS)


def test_pole_at_one_is_scipys_error():
    integ = np.array([[1.0, 0, 0, 1, -1.0, 0]])
    x = sig((2, 300), 5)
    try:
        ss.sosfiltfilt(integ, x, axis=-1)
    except Exception as e:            # whatever SciPy raises from sosfilt_zi is what the caller sees
        with pytest.raises(type(e)):
            fx().sosfiltfilt(torch.from_numpy(x), integ)
    else:
        pytest.fail("SciPy accepted a cascade with a pole at z = 1")


# ---- the device kernel's start state, restated ----------------------------------------------------------------------
def df1_filtfilt(sos, x, gains, pad):
    """What the device computes for one row: odd extension by `pad`, a DF1 cascade forward and backward, every pass started
    from the steady state for its first sample v -- section s holds v * gains[s] as past inputs, v * gains[s + 1] as past
    outputs."""
    def run(v):
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
            x1 = x2 = v[0] * gains[s]
            y1 = y2 = v[0] * gains[s + 1]
            w = v if s == 0 else out
            out = np.empty_like(v)
            for n in range(v.size):
                y = b0 * w[n] + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
                x2, x1, y2, y1 = x1, w[n], y1, y
                out[n] = y
        return out
    ext = np.concatenate([2 * x[0] - x[pad:0:-1], x, 2 * x[-1] - x[-2:-pad - 2:-1]])
    return run(run(ext)[::-1])[::-1][pad:pad + x.size]


@pytest.mark.parametrize("name", ["butter4", "hp20", "ellip12", "notch", "biquad"])
def test_steady_state_gains_reproduce_sosfiltfilt(name):
    from torchfx_amd.filtfilt import default_padlen, steady_state_gains
    sos = {"butter4": SOS, "hp20": ss.butter(2, 20, "highpass", fs=48000, output="sos"),
           "ellip12": ss.ellip(12, 0.1, 60, 1000, fs=48000, output="sos"),
           "notch": ss.tf2sos(*ss.iirnotch(60, 30, fs=48000)),
           "biquad": ss.butter(2, 2000, fs=48000, output="sos")}[name]
    g = steady_state_gains(sos)
    assert g.shape == (sos.shape[0] + 1,) and g[0] == 1.0
    for s in range(sos.shape[0]):                           # restated: the DC gain of the sections in front of s + 1
        w, h = ss.sosfreqz(sos[:s + 1], worN=[0.0])
        assert abs(g[s + 1] - h[0].real) <= 1e-9 * max(1.0, abs(h[0].real))
    x = sig((3000,), 11, np.float32).astype(np.float64) * 0.5 + 0.4
    got = df1_filtfilt(sos, x, g, default_padlen(sos))
    ref = ss.sosfiltfilt(sos, x)
    assert np.abs(got - ref).max() <= 2e-11 * max(1.0, np.abs(ref).max())
    # the start state matters: from zero state the offset signal is off by far more
    assert np.abs(df1_filtfilt(sos, x, np.zeros_like(g), default_padlen(sos)) - ref).max() > 1e-3


# ---- ZeroPhase ---------------------------------------------------------------------------------------------------------
def test_zero_phase_designs_at_the_waves_rate_and_is_stateless():
    lp = F().LoButterworth(1000, order=4)
    assert lp.fs is None
    zp = F().ZeroPhase(lp)
    x = sig((2, 4000), 6, np.float32)
    w = fx().Wave(torch.from_numpy(x), 44100) | zp
    assert lp.fs == 44100 and zp.fs == 44100
    ref = ss.sosfiltfilt(ss.butter(4, 1000, fs=44100, output="sos"), x.astype(np.float64), axis=-1).astype(np.float32)
    assert np.array_equal(w.ys.numpy(), ref)
    assert lp._state_x is None and lp._state_y is None          # never touched
    marker = torch.full((2, 2, 2), 7.0, dtype=torch.float64)
    lp._state_x, lp._state_y = marker.clone(), marker.clone()
    zp(torch.from_numpy(x))
    assert torch.equal(lp._state_x, marker) and torch.equal(lp._state_y, marker)
    assert "padtype='odd'" in repr(zp) and "padlen=None" in repr(zp)


def test_zero_phase_of_several_filters_is_one_sosfiltfilt():
    a, b = F().HiButterworth(200, order=2, fs=48000), F().BiquadLPF(cutoff=3000, q=0.707, fs=48000)
    c = F().FusedSOSCascade(F().LoButterworth(5000, order=4, fs=48000), F().Notch(60, q=30, fs=48000))
    zp = F().ZeroPhase(a, b, c, padtype="even", padlen=50)
    got = zp.sos().numpy()                                     # designs the members whose design is pending
    sos = np.vstack([a._sos.numpy(), b._sos.numpy(), c._sos.numpy()])
    assert sos.shape == (1 + 1 + 3, 6) and np.array_equal(got, sos)
    x = sig((2, 3, 2000), 7)
    assert np.array_equal(zp(torch.from_numpy(x)).numpy(), ss.sosfiltfilt(sos, x, axis=-1, padtype="even", padlen=50))
    with pytest.raises(TypeError):
        F().ZeroPhase(F().DesignableFIR(cutoff=1000, num_taps=31, fs=48000))
    with pytest.raises(ValueError):
        F().ZeroPhase()
    with pytest.raises(ValueError):
        F().ZeroPhase(a, padtype="reflect")


def test_planner_keeps_zero_phase_as_a_barrier(oracle_backend):
    flt, E = F(), __import__("torchfx_amd.effect", fromlist=["Gain"])
    x = sig((2, 6000), 8, np.float32)
    mk = lambda: [flt.LoButterworth(4000, order=4), flt.HiButterworth(100, order=2),            # noqa: E731
                  flt.ZeroPhase(flt.LoButterworth(1000, order=2)), flt.HiButterworth(50, order=2), flt.Notch(60, q=30),
                  E.Gain(0.5)]
    w = fx().Wave(torch.from_numpy(x), 48000)
    for m in mk():
        w = w | m
    plan = w.plan()
    inner = [type(m.producer).__name__ if type(m).__name__ == "Epilogued" else type(m).__name__ for m in plan]
    assert inner[:3] == ["FusedSOSCascade", "ZeroPhase", "FusedSOSCascade"], inner
    assert plan[0]._sos.shape[0] == 3 and type(plan[1]).__name__ == "ZeroPhase"     # nothing attached to or folded into it
    lines = w.explain()
    assert any(ln.startswith("ZeroPhase: scipy on host -- cpu tensor") for ln in lines), lines
    # the planned pipeline equals the steps run one by one
    y = torch.from_numpy(x)
    for m in mk():
        if hasattr(m, "fs") and m.fs is None:
            m.fs = 48000
        if hasattr(m, "compute_coefficients") and not m._has_computed_coeff:
            m.compute_coefficients()
        y = m(y)
    assert np.abs(w.ys.numpy() - y.numpy()).max() <= 3e-7
    # a Gain right behind it stays a pass of its own
    w2 = fx().Wave(torch.from_numpy(x), 48000) | flt.ZeroPhase(flt.LoButterworth(1000, order=2)) | E.Gain(0.5)
    assert [type(m).__name__ for m in w2.plan()] == ["ZeroPhase", "Gain"]


def test_streams_refuse_zero_phase():
    from torchfx_amd.realtime import StreamProcessor
    zp = F().ZeroPhase(F().LoButterworth(1000, fs=48000))

    class Nested(fx().FX):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x)

    with pytest.raises(TypeError, match="non-causal"):
        StreamProcessor([zp], chunk_size=4096, device="cpu")
    with pytest.raises(TypeError, match="non-causal"):
        StreamProcessor([F().HiButterworth(100, fs=48000), Nested(zp)], chunk_size=4096, device="cpu")     # found inside an effect too
    from torchfx_amd.realtime import AudioBackend, RealtimeProcessor, StreamConfig

    class NoBackend(AudioBackend):
        def open_stream(self, config, callback=None):
            raise AssertionError("the refusal comes before a stream is opened")

        def start(self):
            pass

        def stop(self):
            pass

        def close(self):
            pass

    for effects in ([zp], [F().HiButterworth(100, fs=48000), Nested(zp)]):
        with pytest.raises(TypeError, match="non-causal"):
            RealtimeProcessor(effects, NoBackend(), StreamConfig(), device="cpu")


# ---- C ABI, host only ------------------------------------------------------------------------------------------------
def test_plan_info_runs_without_a_device():
    from torchfx_amd import torchfx_ext as E
    info = E.sos_filtfilt_plan_info(SOS, 4, 3_000_000)
    assert info["default_padlen"] == info["padlen"] == 15
    assert info["work_elems"] == 4 * (3_000_000 + 30)
    assert 100 < info["warmup"] < 2000
    assert info["nseg_forward"] > 1 and info["nseg_reverse"] > 1             # long rows are cut in BOTH passes
    short = E.sos_filtfilt_plan_info(SOS, 4, 4097)
    assert short["nseg_forward"] == short["nseg_reverse"] == 1
    assert E.sos_filtfilt_plan_info(SOS, 4, 5000, padtype=None, padlen=99)["padlen"] == 0
    assert E.sos_filtfilt_plan_info(SOS, 4, 5000, padtype="constant", padlen=99)["work_elems"] == 4 * (5000 + 198)
    # a filter that never forgets runs one segment per row
    slow = np.array([[1.0, 0, 0, 1, -1.9999999, 0.99999991]])
    info = E.sos_filtfilt_plan_info(slow, 4, 3_000_000)
    assert info["warmup"] == -1 and info["nseg_forward"] == info["nseg_reverse"] == 1
    with pytest.raises(RuntimeError, match="greater than padlen, which is 15"):
        E.sos_filtfilt_plan_info(SOS, 4, 15)
    with pytest.raises(RuntimeError, match="pole at z = 1"):
        E.sos_filtfilt_plan_info(np.array([[1.0, 0, 0, 1, -1.0, 0]]), 4, 5000)


def test_bad_arguments_are_errors_not_crashes():
    from torchfx_amd import _lib
    lib = _lib.load()
    sos = (ctypes.c_double * 6)(1, 0, 0, 1, -0.5, 0)
    cases = [
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 100, sos, 1, 0, -1, None, None),          # null signal
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, -1, 100, sos, 1, 0, -1, None, None),         # negative size
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, -100, sos, 1, 0, -1, None, None),
        lib.tfx_sos_filtfilt_forward(None, 7, None, 0, 2, 100, sos, 1, 0, -1, None, None),          # bad dtype
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 100, None, 1, 0, -1, None, None),         # null coefficients
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 100, sos, 0, 0, -1, None, None),          # no sections
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 100, sos, 1, 4, -1, None, None),          # bad padtype
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 100, sos, 1, 0, -2, None, None),          # negative padlen
        lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 6, sos, 1, 0, -1, None, None),            # T <= padlen
        lib.tfx_sos_filtfilt_plan_info(2, 100, None, 1, 0, -1, None, None, None, None, None, None),
        lib.tfx_sos_filtfilt_plan_info(-2, 100, sos, 1, 0, -1, None, None, None, None, None, None),
    ]
    assert all(rc != 0 for rc in cases), cases
    assert lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 6, sos, 1, 0, -1, None, None) != 0
    assert b"greater than padlen, which is 6" in lib.tfx_last_error()
    assert lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 2, 100, sos, 1, 0, -1, None, None) != 0
    assert b"null" in lib.tfx_last_error()
    # no rows: nothing to do, nothing touched
    assert lib.tfx_sos_filtfilt_forward(None, 0, None, 0, 0, 100, sos, 1, 0, -1, None, None) == 0


def test_op_has_a_meta_kernel_and_no_cpu_kernel():
    import torchfx_amd.ops  # noqa: F401
    y = torch.ops.torchfx_hip.sos_filtfilt(torch.empty(2, 3, 100, device="meta"), torch.from_numpy(SOS))
    assert y.shape == (2, 3, 100) and y.dtype == torch.float32
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.torchfx_hip.sos_filtfilt(torch.zeros(2, 100), torch.from_numpy(SOS))
