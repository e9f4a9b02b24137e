"""The phaser without a device: the NumPy host path of torchfx_amd.phaser.phase_shift against tests/phaser_reference.py (the
coefficient track within delta_a, the recursion within 16 E_REF of the long-double loop fed the path's own coefficient bits),
argument errors, the state round trip, Phaser in a Wave, the planner and explain(), the torchfx_phaser namespace, the plan query
and the C ABI's refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import phaser_reference as R

FS = 48000


def fx():
    import torchfx_amd
    return torchfx_amd


def signal(shape, seed=0, dtype=np.float32):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(dtype)


def host(x, **kw):
    out = fx().phase_shift(torch.from_numpy(np.ascontiguousarray(x)), FS, return_coef=True, return_state=True, **kw)
    return [t.numpy() for t in out]


def both_checks(what, x, dry=0.5, wet=0.5, state=None, **kw):
    p = dict(dict(stages=4, min_freq=200.0, max_freq=2000.0, rate=3.0, phase=0.0, spread=0.0, shape="sine", position=0), **kw)
    y, coef, st = host(x, dry=dry, wet=wet, state=None if state is None else torch.from_numpy(state), **p)
    C = x.shape[-2] if x.ndim >= 2 else 1
    assert y.shape == x.shape and y.dtype == x.dtype and coef.shape == ((C if p["spread"] != 0.0 and C > 1 else 1), x.shape[-1])
    R.check_coef(coef, FS, p["min_freq"], p["max_freq"], p["rate"], p["phase"], p["spread"], p["shape"], p["position"], what)
    rows = x.reshape(-1, x.shape[-1])
    yld, sld, e_ref = R.reference(rows, coef, p["stages"], dry, wet, C, state)
    R.check(y.reshape(rows.shape), yld, e_ref, what)
    gap = np.abs(yld.astype(np.float64) - dry * rows.astype(np.float64)).max(-1)
    assert np.all(gap > 100.0 * (16.0 * e_ref + 2.0 ** -24 * np.abs(yld).max(-1).astype(np.float64))), f"{what}: the wet part is not at work"
    return y, coef, st, sld


# ---- the host path against the loop -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("stages,lo,hi", [(4, 200.0, 2000.0), (12, 200.0, 2000.0), (4, 20.0, 8000.0), (12, 20.0, 8000.0)])
def test_host_path_on_the_measured_cases(stages, lo, hi):
    """30 000 samples of uniform noise at 48 kHz, rate 3 Hz: longer than the host path's block, so the carry between blocks is in."""
    both_checks(f"host N={stages} {lo:g}-{hi:g}", signal((30000,), stages, np.float64), stages=stages, min_freq=lo, max_freq=hi)


@pytest.mark.parametrize("position", [0, 2 ** 40], ids=["p0", "p2^40"])
@pytest.mark.parametrize("shape", [(700,), (2, 700), (3, 2, 700)], ids=["T", "CT", "BCT"])
@pytest.mark.parametrize("lfo", ["sine", "triangle"])
def test_host_path_against_the_definition(lfo, shape, position):
    dtype = np.float32 if len(shape) == 2 else np.float64
    both_checks(f"host {lfo} {shape}", signal(shape, len(shape), dtype), dry=0.6, stages=2 + len(shape), rate=30.0, phase=0.1,
                spread=0.25, shape=lfo, position=position)


def test_lengths_one_two_and_a_block_seam():
    from torchfx_amd import phaser

    for T in (1, 2, 7, phaser._HOST_BLOCK - 1, phaser._HOST_BLOCK, phaser._HOST_BLOCK + 1):
        x = signal((2, T), T % 11, np.float64)
        y, coef, st = host(x, rate=30.0, spread=0.25)
        yld, sld, e_ref = R.reference(x, coef, 4, 0.5, 0.5, 2)
        R.check(y, yld, e_ref, f"host T={T}")


def test_state_round_trip_and_the_dry_path():
    x = signal((3, 2, 900), 3, np.float64)
    state = np.random.default_rng(4).uniform(-1.0, 1.0, (6, 5))
    y, coef, st, sld = both_checks("host state", x, state=state, rate=30.0, spread=0.25)
    assert st.shape == (6, 5) and st.dtype == np.float64 and np.array_equal(st[:, 0], x.reshape(6, -1)[:, -1])
    assert np.abs(st - sld.astype(np.float64)).max() < 1e-13
    t = torch.from_numpy(x)
    f = fx()
    ya, sa = f.phase_shift(t[..., :411], FS, rate=30.0, spread=0.25, state=torch.from_numpy(state), return_state=True)
    yb, cb = f.phase_shift(t[..., 411:], FS, rate=30.0, spread=0.25, state=sa, position=411, return_coef=True)
    assert np.array_equal(cb.numpy(), coef[:, 411:])                   # the coefficient track does not depend on the cut
    assert np.abs(torch.cat([ya, yb], -1).numpy() - y).max() < 1e-13
    # wet = 0, dry = 1: the input comes back bit for bit; None is silence
    assert torch.equal(f.phase_shift(t, FS, dry=1.0, wet=0.0), t)
    assert torch.equal(f.phase_shift(t, FS, state=torch.zeros(6, 5)), f.phase_shift(t, FS))
    empty, st0 = f.phase_shift(t[..., :0], FS, state=torch.from_numpy(state), return_state=True)
    assert empty.shape == (3, 2, 0) and np.array_equal(st0.numpy(), state)


def test_equal_rows_and_a_planted_nan():
    x = signal((2, 2, 600), 6, np.float64)
    x[1] = x[0]
    f = fx()
    y = f.phase_shift(torch.from_numpy(x), FS, rate=30.0, spread=0.25).numpy()
    assert np.array_equal(y[0], y[1]) and not np.array_equal(y[0, 0], y[0, 1])
    bad = x.copy()
    bad[0, 1, 300] = np.nan
    z, st = f.phase_shift(torch.from_numpy(bad), FS, rate=30.0, spread=0.25, return_state=True)
    z = z.numpy()
    assert np.isnan(z[0, 1, 300:]).all() and np.isfinite(z[0, 1, :300]).all()
    assert np.array_equal(z[0, 0], y[0, 0]) and np.array_equal(z[1], y[1])
    assert np.isnan(st.numpy()[1, 1:]).all() and np.isfinite(st.numpy()[[0, 2, 3]]).all()


# ---- arguments --------------------------------------------------------------------------------------------------------------

def test_argument_errors():
    f = fx()
    x = torch.zeros(2, 64)
    bad = [dict(stages=0), dict(stages=13), dict(stages=2.0), dict(stages=True), dict(min_freq=9.9), dict(min_freq=3000.0),
           dict(max_freq=0.46 * FS), dict(max_freq=math.inf), dict(min_freq=math.nan), dict(rate=0.0), dict(rate=FS / 2), dict(rate=-1.0),
           dict(rate=math.nan), dict(position=-1), dict(position=2 ** 52 + 1), dict(position=1.5), dict(dry=math.inf), dict(wet=math.nan),
           dict(phase=math.inf), dict(spread=math.nan), dict(shape="square"), dict(state=torch.zeros(2, 4))]
    for kw in bad:
        with pytest.raises(ValueError, match="phase_shift"):
            f.phase_shift(x, FS, **kw)
    with pytest.raises(TypeError, match="phase_shift"):
        f.phase_shift(x.to(torch.int32), FS)
    with pytest.raises(TypeError, match="phase_shift"):
        f.phase_shift(x, FS, state=np.zeros((2, 5)))
    with pytest.raises(TypeError, match="phase_shift"):
        f.phase_shift(np.zeros((2, 64)), FS)
    with pytest.raises(ValueError):
        f.phase_shift(torch.zeros(1, 1, 1, 8), FS)
    with pytest.raises(ValueError):
        f.phase_shift(x, 4000)
    f.phase_shift(x, FS, stages=12, min_freq=10.0, max_freq=0.45 * FS, rate=FS / 2 - 1, position=2 ** 52)       # the edges are allowed
    for kw in (dict(stages=0), dict(mix=math.nan), dict(max_freq=100.0), dict(shape="saw")):
        with pytest.raises(ValueError, match="phase_shift"):
            f.Phaser(**kw)
    with pytest.raises(ValueError, match="sample rate"):
        f.Phaser()(x)


# ---- effect, planner ----------------------------------------------------------------------------------------------------------

def test_phaser_in_a_wave_the_planner_step_and_explain():
    f = fx()
    x = torch.from_numpy(signal((2, 3000), 12))
    ph = f.Phaser(rate=30.0, invert=True, mix=0.4, spread=0.25)
    w = f.Wave(x, FS) | f.filter.HiButterworth(100, order=2) | f.Gain(0.9) | ph | f.Gain(1.1)
    assert ph.fs == FS
    plan = w.plan()
    assert sum(m is ph for m in plan) == 1
    k = plan.index(ph)
    assert 0 < k < len(plan) - 1
    assert w.explain()[k] == "Phaser: numpy on host -- cpu tensor"
    P = ph.params(torch.float32)
    assert (P.dry, P.wet, P.stages, P.rate, P.spread) == (0.6, -0.4, 4, 30.0, 0.25)
    y = (f.Wave(x, FS) | f.Phaser(rate=30.0, invert=True, mix=0.4, spread=0.25)).ys
    assert torch.equal(y, f.phase_shift(x, FS, rate=30.0, dry=0.6, wet=-0.4, spread=0.25))
    # every parameter is in the plan key: a changed one is another plan
    for kw in (dict(rate=31.0), dict(min_freq=210.0), dict(max_freq=2100.0), dict(stages=5), dict(mix=0.41), dict(invert=False),
               dict(spread=0.3), dict(shape="triangle")):
        other = dict(dict(rate=30.0, invert=True, mix=0.4, spread=0.25), **kw)
        assert (f.Wave(x, FS) | f.Phaser(**other)).ys.ne(y).any(), kw
    assert "rate=30.0" in repr(ph) and "stages=4" in repr(ph) and "invert=True" in repr(ph)
    assert {"Phaser", "phase_shift"} <= set(f.__all__)
    assert ph.route(x) == "numpy on host -- cpu tensor"


def test_phaser_namespace_census():
    """Exactly one op in ``torchfx_phaser``, with a device kernel, the CPU refusal and shape inference."""
    from torchfx_amd import native
    from torchfx_amd import torchfx_ext as E

    ns = native.phaser_ops()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_phaser::")}
    assert names == {"torchfx_phaser::phaser_forward"}
    for key in ("CUDA", "CPU", "Meta"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key("torchfx_phaser::phaser_forward", key), key
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.phaser_forward(torch.zeros(2, 8), 4, 48000.0, 0.5, 200.0, 2000.0, 0.0, 0.0, 0.5, 0.5, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.phaser_forward(torch.zeros(2, 8), 4, FS, 0.5, 200.0, 2000.0)
    meta = torch.empty(3, 2, 50, device="meta")
    y, coef, st, pos = ns.phaser_forward(meta, 6, 48000.0, 0.5, 200.0, 2000.0, 0.0, 0.25, 0.5, 0.5, 0, 0, None, None, True, 0)
    assert y.shape == (3, 2, 50) and coef.shape == (2, 50) and coef.dtype == torch.float64 and st.shape == (6, 7) and pos.shape == (0,)
    y, coef, st, pos = ns.phaser_forward(meta, 6, 48000.0, 0.5, 200.0, 2000.0, 0.0, 0.0, 0.5, 0.5, 0, 0,
                                         torch.empty(1, dtype=torch.int64, device="meta"), None, True, 0)
    assert coef.shape == (1, 50) and pos.shape == (1,) and pos.dtype == torch.int64 and st.dtype == torch.float64
    assert ns.phaser_forward(meta, 6, 48000.0, 0.5, 200.0, 2000.0, 0.0, 0.0, 0.5, 0.5, 0)[1].shape == (0,)
    assert {"phaser_forward", "phaser_plan_info"} <= set(E.__all__)


def test_plan_info_geometry():
    from torchfx_amd import torchfx_ext as E

    info = E.phaser_plan_info(3 * 2048 + 17, rows=2, channels=2, stages=4)
    assert info == dict(tile=2048, tiles=4, segments=4, seg_tiles=1, scratch_bytes=2 * 4 * 2 * 4 * 8)
    assert E.phaser_plan_info(3 * 2048 + 17, rows=2, channels=2, stages=12, segments=3) == dict(
        tile=2048, tiles=4, segments=3, seg_tiles=2, scratch_bytes=2 * 3 * 2 * 12 * 8)
    one = E.phaser_plan_info(2_880_000, rows=256, channels=2)
    assert one["segments"] == 1 and one["scratch_bytes"] == 0 and one["tiles"] == 1407 and one["seg_tiles"] == 1407
    many = E.phaser_plan_info(28_800_000, rows=2, channels=2)
    assert many["segments"] == 256 and many["tiles"] == 14063 and many["seg_tiles"] == 55
    assert E.phaser_plan_info(100, segments=9)["segments"] == 1 and E.phaser_plan_info(0)["tiles"] == 0
    for kw in (dict(stages=0), dict(stages=13), dict(channels=0), dict(rows=3, channels=2), dict(segments=-1), dict(length=-1)):
        with pytest.raises(RuntimeError, match="phaser_plan_info"):
            E.phaser_plan_info(**dict(dict(length=100), **kw))


def test_c_abi_refuses_bad_arguments_before_the_device():
    from torchfx_amd import _lib

    lib = _lib.load()
    buf, out = [(ctypes.c_float * 256)() for _ in range(2)]
    st = [(ctypes.c_double * 16)() for _ in range(2)]
    pos = [(ctypes.c_int64 * 1)() for _ in range(2)]
    vp = lambda b: None if b is None else ctypes.cast(b, ctypes.c_void_p)      # noqa: E731
    ok = dict(x=buf, y=out, coef=None, dtype=0, rows=2, channels=2, T=32, stages=4, fs=48000.0, rate=0.5, lo=200.0, hi=2000.0, phase=0.0,
              spread=0.0, dry=0.5, wet=0.5, shape=0, position=0, pin=None, pout=None, sin=None, sout=None, segments=0, scratch=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tfx_phaser_forward(vp(a["x"]), vp(a["y"]), vp(a["coef"]), a["dtype"], a["rows"], a["channels"], a["T"], a["stages"],
                                      a["fs"], a["rate"], a["lo"], a["hi"], a["phase"], a["spread"], a["dry"], a["wet"], a["shape"],
                                      a["position"], vp(a["pin"]), vp(a["pout"]), vp(a["sin"]), vp(a["sout"]), a["segments"],
                                      vp(a["scratch"]), None)
    bad = [dict(x=None), dict(y=None), dict(y=buf), dict(dtype=7), dict(rows=-1), dict(T=-1), dict(channels=0), dict(rows=3), dict(stages=0),
           dict(stages=13), dict(shape=2), dict(fs=0.0), dict(fs=math.nan), dict(lo=9.0), dict(lo=3000.0), dict(hi=0.46 * 48000.0),
           dict(rate=0.0), dict(rate=24000.0), dict(rate=math.nan), dict(phase=math.inf), dict(spread=math.nan), dict(dry=math.inf),
           dict(wet=math.nan), dict(position=-1), dict(position=2 ** 52 + 1), dict(segments=-1), dict(sin=st[0], sout=st[0]),
           dict(pin=pos[0], pout=pos[0]), dict(T=3 * 2048, segments=2, x=None)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"phaser_forward" in lib.tfx_last_error(), kw
    assert call(T=3 * 2048, segments=2) != 0 and b"scratch" in lib.tfx_last_error()      # two segments need the summaries' buffer
    assert call(rows=0) == 0                                            # empty work is fine and touches nothing
    i64 = ctypes.c_int64
    outs = [i64() for _ in range(5)]
    refs = [ctypes.byref(o) for o in outs]
    assert lib.tfx_phaser_plan_info(2, 2, 5000, 4, 0, *refs) == 0
    assert [o.value for o in outs] == [2048, 3, 3, 1, 2 * 3 * 2 * 4 * 8]
    assert lib.tfx_phaser_plan_info(2, 2, 5000, 4, 0, None, *refs[1:]) != 0 and b"null output" in lib.tfx_last_error()
    assert lib.tfx_phaser_plan_info(2, 2, -5, 4, 0, *refs) != 0
    assert lib.tfx_phaser_plan_info(2, 2, 5000, 13, 0, *refs) != 0
