"""The compressor without a device: the definition's properties on the per-sample reference (tests/compressor_reference.py),
the NumPy host path of torchfx_amd.dynamics.compress against it, argument errors, the plan query and the C ABI's refusals,
the planner, the torchfx_dynamics namespace and StatefulCompressor over CPU chunks.  Bounds as in tests/test_gpu_compressor.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import compressor_reference as R

FS = 48000


def fx():
    import torchfx_amd
    return torchfx_amd


def host(x, **kw):
    y, g, st = fx().compress(torch.from_numpy(np.ascontiguousarray(x)), FS, return_gain=True, return_state=True, **kw)
    return y.numpy(), g.numpy(), st.numpy()


def within(got, ref, dtype):
    (y, g, st), (yr, gr, sr) = got, ref
    yr = yr.reshape(y.shape)
    top = np.abs(yr).max()
    if dtype == np.float64:
        assert np.abs(y - yr).max() <= 1e-11 * top
        assert np.abs(20 * np.log10(g) - 20 * np.log10(gr)).max() <= 1e-10
    else:
        assert np.all(np.abs(y.astype(np.float64) - yr) <= 2.0 ** -23 * np.abs(yr) + 1e-11 * top)
        assert np.all(np.abs(g.astype(np.float64) - gr) <= (2.0 ** -24 + 2e-11) * gr)
    assert np.abs(st - sr).max() <= 1e-10


# ---- the definition's properties, on the reference -------------------------------------------------------------------------

@pytest.mark.parametrize("ratio,level_db", [(4.0, -6.0), (2.0, -10.0), (math.inf, -3.0), (1.0, -6.0)])
def test_static_curve_settles(ratio, level_db):
    th, T = -20.0, 6000
    x = np.full(T, 10 ** (level_db / 20))
    y, g, _ = R.compress_ref(x, FS, th, ratio, attack=1e-3, release=5e-3, knee_db=6.0)
    want = th + (level_db - th) / ratio
    assert abs(20 * math.log10(abs(y[-1])) - want) <= 1e-6


def test_attack_and_release_closed_forms():
    aA, aR = R.alphas(FS, 5e-3, 100e-3)
    v0, n = 7.25, np.arange(2000)
    y1, yl = R.detector(np.full(2000, v0), aA, aR)
    assert np.abs(yl - v0 * (1 - aA ** (n + 1))).max() <= 1e-12 * v0
    assert np.all(y1 == v0)
    y1, _ = R.detector(np.zeros(2000), aA, aR, state=(v0, 0.0))
    assert np.abs(y1 - v0 * aR ** (n + 1)).max() <= 1e-12 * v0


def test_hard_knee_infinite_ratio_and_instant_times():
    assert R.curve(10 ** (-20 / 20) * (1 - 1e-9), -20.0, 0.75, 0.0) == 0.0
    assert R.curve(10 ** (-10 / 20), -20.0, 0.75, 0.0) == pytest.approx(7.5, abs=1e-12)
    assert R.curve(10 ** (-20 / 20), -20.0, 0.75, 6.0) == pytest.approx(0.75 * 9 / 12, abs=1e-12)      # mid knee: s (W/2)^2 / (2W)
    assert R.curve(0.5, -20.0, 1.0, 0.0) == pytest.approx(20 * math.log10(0.5) + 20, abs=1e-12)         # ratio = inf: s = 1
    x = np.array([0.01, 0.5, 0.5, 0.01, 0.01])
    _, g, _ = R.compress_ref(x, FS, attack=0.0, release=0.0, knee_db=0.0)
    v = np.array([R.curve(p, -20.0, 0.75, 0.0) for p in x])
    assert np.abs(-20 * np.log10(g[0]) - v).max() <= 1e-12                                               # the gain follows v at once
    _, g, _ = R.compress_ref(x, FS, attack=0.0, release=50e-3, knee_db=0.0)
    assert g[0, 3] < 1.0 and g[0, 1] == pytest.approx(10 ** (-v[1] / 20))                                # instant attack, slow release


def test_silence_is_exact_and_nan_goes_to_the_end_of_its_group():
    y, g, st = R.compress_ref(np.zeros((2, 500)), FS)
    assert np.all(y == 0) and np.all(g == 1.0) and np.all(st == 0)
    x = R.bursty(np.random.default_rng(0), (2, 2, 600))
    clean = R.compress_ref(x, FS)
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[1, 0, 300] = bad
        for got in (R.compress_ref(xb, FS), host(xb)):
            y, g, st = got
            assert np.abs(y[0] - clean[0][0]).max() <= 1e-11 * np.abs(clean[0][0]).max()                 # the other group
            assert np.isnan(y[1][:, 300:]).all() and np.isnan(g[1][300:]).all() and np.isnan(st[1]).all()
            assert np.isfinite(y[1][:, :300]).all() and np.isfinite(st[0]).all()


# ---- the host path against the reference -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("link", [True, False])
@pytest.mark.parametrize("shape", [(3000,), (2, 3000), (2, 2, 2500)])
def test_host_path_against_the_definition(shape, link, dtype):
    x = R.bursty(np.random.default_rng(len(shape)), shape, dtype=dtype)
    for kw in ({}, {"attack": 0.0, "release": 50e-3}, {"attack": 1e-3, "release": 0.0}, {"ratio": math.inf, "knee_db": 0.0, "makeup_db": 3.0}):
        within(host(x, link=link, **kw), R.compress_ref(x, FS, link=link, **kw), dtype)


def test_host_path_crosses_its_block_seam(monkeypatch):
    from torchfx_amd import dynamics

    monkeypatch.setattr(dynamics, "_HOST_BLOCK", 700)
    x = R.bursty(np.random.default_rng(5), (2, 3000))
    within(host(x), R.compress_ref(x, FS), np.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_transparent_bit_for_bit(dtype):
    x = (np.random.default_rng(1).uniform(-1, 1, (2, 2, 5000)) * 10 ** (-23.5 / 20)).astype(dtype)
    y, g, st = host(x)
    assert np.array_equal(y.view(np.uint8), x.view(np.uint8)) and np.all(g == 1.0) and np.all(st == 0.0)


def test_two_halves_with_a_carried_state_equal_one_piece():
    x = R.bursty(np.random.default_rng(2), (2, 4000))
    ref = R.compress_ref(x, FS)
    ya, ga, sa = host(x[:, :1777])
    yb, gb, sb = host(x[:, 1777:], state=torch.from_numpy(sa))
    within((np.concatenate([ya, yb], -1), np.concatenate([ga, gb], -1), sb), ref, np.float64)


def test_return_forms_and_empty_signal():
    x = torch.zeros(2, 100)
    assert isinstance(fx().compress(x, FS), torch.Tensor)
    assert len(fx().compress(x, FS, return_gain=True)) == 2 and len(fx().compress(x, FS, return_state=True)) == 2
    y, g, st = fx().compress(torch.zeros(2, 0), FS, return_gain=True, return_state=True, state=torch.ones(1, 2))
    assert y.shape == (2, 0) and g.shape == (1, 0) and torch.equal(st, torch.ones(1, 2, dtype=torch.float64))


def test_argument_errors():
    x = torch.zeros(2, 64)
    c = fx().compress
    for kw in ({"ratio": 0.5}, {"ratio": math.nan}, {"ratio": True}, {"attack": -1e-3}, {"attack": math.inf}, {"release": -1.0},
               {"release": math.nan}, {"knee_db": -1.0}, {"knee_db": math.inf}, {"threshold_db": math.inf}, {"threshold_db": math.nan},
               {"makeup_db": math.inf}, {"state": torch.zeros(2, 2)}, {"state": torch.zeros(2)}):
        with pytest.raises(ValueError):
            c(x, FS, **kw)
        if "state" not in kw:
            with pytest.raises(ValueError):
                fx().Compressor(**kw)
    with pytest.raises(ValueError):
        c(x, 100)
    with pytest.raises(TypeError):
        c(x.to(torch.int16), FS)
    with pytest.raises(TypeError):
        c(x.to(torch.float16), FS)
    with pytest.raises(TypeError):
        c(x.numpy(), FS)
    with pytest.raises(TypeError):
        c(x, FS, state=np.zeros((1, 2)))
    with pytest.raises(ValueError):
        c(torch.zeros(1, 1, 2, 8), FS)
    with pytest.raises(ValueError, match="sample rate"):
        fx().Compressor()(x)


# ---- the boundary ----------------------------------------------------------------------------------------------------------

def test_plan_info_without_a_device():
    from torchfx_amd import torchfx_ext as E

    info = E.compressor_plan_info(3 * 2048 + 17, 1, 2)
    assert info["tile"] == 2048 and info["tiles"] == 4 and 1 <= info["segments"] <= 4
    assert E.compressor_plan_info(3 * 2048 + 17, 1, 2, 3) == {"tile": 2048, "tiles": 4, "segments": 3, "seg_tiles": 2, "scratch_bytes": 72}
    assert E.compressor_plan_info(3 * 2048 + 17, 1, 2, 100)["segments"] == 4
    one = E.compressor_plan_info(48000, 4096, 2)                       # the groups alone fill the chip
    assert one["segments"] == 1 and one["scratch_bytes"] == 0 and one["seg_tiles"] == one["tiles"]
    long_row = E.compressor_plan_info(28_800_000, 1, 2)
    assert long_row["segments"] > 1 and long_row["scratch_bytes"] == long_row["segments"] * 24
    assert E.compressor_plan_info(0, 1, 1)["tiles"] == 0
    with pytest.raises(RuntimeError, match="segments"):
        E.compressor_plan_info(100, 1, 1, -1)
    with pytest.raises(RuntimeError, match="channels"):
        E.compressor_plan_info(100, 1, 0)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from torchfx_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(x=p, y=p, gain=None, dtype=0, groups=1, channels=1, T=32, th=-20.0, s=0.75, w=6.0, aa=0.9, ar=0.99, mk=0.0, sin=None,
              sout=None, seg=0, scratch=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tfx_compressor_forward(a["x"], a["y"], a["gain"], a["dtype"], a["groups"], a["channels"], a["T"], a["th"], a["s"],
                                          a["w"], a["aa"], a["ar"], a["mk"], a["sin"], a["sout"], a["seg"], a["scratch"], None)
    bad = [dict(x=None), dict(y=None), dict(dtype=7), dict(groups=-1), dict(T=-1), dict(channels=0), dict(th=math.inf), dict(s=1.5),
           dict(s=-0.1), dict(s=math.nan), dict(w=-1.0), dict(w=math.nan), dict(aa=1.5), dict(aa=-0.5), dict(ar=math.nan),
           dict(mk=math.inf), dict(seg=-1), dict(T=3 * 2048, seg=2), dict(sin=p, sout=p)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"compressor_forward" in lib.tfx_last_error(), kw
    assert b"scratch" in (call(T=3 * 2048, seg=2), lib.tfx_last_error())[1]
    assert call(groups=0) == 0 and call(T=0) == 0                     # empty work is fine and touches nothing
    i64 = ctypes.c_int64
    outs = [i64() for _ in range(5)]
    assert lib.tfx_compressor_plan_info(1, 1, 100, 0, *[ctypes.byref(o) for o in outs]) == 0
    assert lib.tfx_compressor_plan_info(1, 1, 100, 0, None, *[ctypes.byref(o) for o in outs[1:]]) != 0
    assert lib.tfx_compressor_plan_info(-1, 1, 100, 0, *[ctypes.byref(o) for o in outs]) != 0


def test_dynamics_namespace_census():
    """Exactly the ops of ``torchfx_dynamics``, each with a device kernel, the CPU refusal and shape inference."""
    from torchfx_amd import native

    ns = native.dynamics_ops()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_dynamics::")}
    assert names == {"torchfx_dynamics::compressor_forward"}
    for name in names:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CPU"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "Meta"), name
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.compressor_forward(torch.zeros(2, 8), -20.0, 0.75, 6.0, 0.9, 0.99, 0.0, 2, None, False)
    from torchfx_amd import torchfx_ext as E
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.compressor_forward(torch.zeros(2, 8), -20.0, 0.75, 6.0, 0.9, 0.99)
    y, g, st = ns.compressor_forward(torch.empty(3, 2, 50, device="meta"), -20.0, 0.75, 6.0, 0.9, 0.99, 0.0, 2, None, True, 0)
    assert y.shape == (3, 2, 50) and g.shape == (3, 50) and st.shape == (3, 2) and st.dtype == torch.float64


# ---- planner, effects, streams ----------------------------------------------------------------------------------------------

def test_planner_keeps_the_compressor_as_a_step_of_its_own():
    f = fx()
    x = torch.from_numpy(R.bursty(np.random.default_rng(3), (2, 3000), dtype=np.float32))
    comp = f.Compressor(-18, 3)
    w = f.Wave(x, FS) | f.filter.HiButterworth(100, order=2) | f.Gain(0.9) | comp | f.Gain(1.1)
    plan = w.plan()
    assert sum(m is comp for m in plan) == 1 and comp.fs == FS
    k = plan.index(comp)
    assert 0 < k < len(plan) - 1
    lines = w.explain()
    assert lines[k].startswith("Compressor: numpy on host")
    y = (f.Wave(x, FS) | f.Compressor(-18, 3)).ys
    within((y.numpy(),) + host(x.numpy(), threshold_db=-18, ratio=3)[1:], R.compress_ref(x.numpy(), FS, -18, 3), np.float32)
    assert "threshold_db=-18.0" in repr(comp)


def test_stream_processors_refuse_the_stateless_compressor():
    from torchfx_amd import realtime as RT

    f = fx()
    with pytest.raises(TypeError, match="StatefulCompressor"):
        RT.StreamProcessor([f.Compressor()], chunk_size=256, device="cpu")
    with pytest.raises(TypeError, match="StatefulCompressor"):
        RT.StreamProcessor([f.Gain(0.5), f.Compressor(-18, 3), f.Gain(2.0)], chunk_size=256, device="cpu")
    RT.StreamProcessor([RT.StatefulCompressor()], chunk_size=256, device="cpu")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stateful_compressor_chunks_equal_the_one_shot_call(dtype):
    from torchfx_amd.realtime import StatefulCompressor

    x = R.bursty(np.random.default_rng(4), (2, 5000), dtype=dtype)
    ref = R.compress_ref(x, FS, -18.0, 3.0)
    c = StatefulCompressor(-18.0, 3.0, fs=FS)
    cuts = [0, 1, 8, 700, 701, 2300, 2301, 4999, 5000]
    y = np.concatenate([c(torch.from_numpy(x[:, a:b].copy())).numpy() for a, b in zip(cuts, cuts[1:])], -1)
    top = np.abs(ref[0]).max()
    tol = (2.0 ** -23 * np.abs(ref[0]) if dtype == np.float32 else 0.0) + 1e-11 * top
    assert np.all(np.abs(y.astype(np.float64) - ref[0]) <= tol)
    assert np.abs(c._hist.numpy() - ref[2]).max() <= 1e-10
    c.reset_state()
    assert c._hist is None
    first = c(torch.from_numpy(x[:, :700].copy())).numpy()
    assert np.array_equal(first, fx().compress(torch.from_numpy(x[:, :700].copy()), FS, -18.0, 3.0).numpy())      # from silence again
    c(torch.from_numpy(x[:1, :10].copy()))                            # another row count: a new stream
    assert c._hist.shape == (1, 2)


def test_stream_processor_runs_stateful_compressor_over_cpu_chunks():
    from torchfx_amd import realtime as RT

    x = R.bursty(np.random.default_rng(6), (2, 4000), dtype=np.float32)
    sp = RT.StreamProcessor([RT.StatefulCompressor(-18.0, 3.0)], chunk_size=512, device="cpu")
    y = sp.process_tensor(torch.from_numpy(x), FS).numpy()
    ref = R.compress_ref(x, FS, -18.0, 3.0)[0]
    assert np.all(np.abs(y.astype(np.float64) - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-11 * np.abs(ref).max())
