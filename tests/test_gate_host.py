"""The gate without a device: the host path (torchfx_amd.gate over NumPy) against the per-sample loop of tests/gate_reference.py
-- open track and the (open, c) of the state exact, gain within the derived bound against the long-double twin -- the exact
consequences of the definition, parameter errors, the state round trip, poison containment, empty signals, planning and
explain(), and the C ABI's argument checks.

The bounds are ``gate_reference.within``'s.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gate_reference as R

FS = 48000
CORNERS = {
    "defaults": {},
    "hold0": {"hold": 0.0},
    "hard": {"attack": 0.0, "release": 0.0},
    "range20": {"range_db": 20.0, "hold": 2e-3},
    "no_hysteresis": {"hysteresis_db": 0.0, "hold": 1e-3},
}


def fx():
    import torchfx_amd
    return torchfx_amd


def run(x, link=True, state=None, **kw):
    """``gate`` on the host -> NumPy ``dict(y, g, open, state)``."""
    st = None if state is None else torch.from_numpy(np.asarray(state, dtype=np.float64))
    y, g, o, s = fx().gate(torch.from_numpy(x), FS, link=link, return_gain=True, return_open=True, state=st, return_state=True, **kw)
    return dict(y=y.numpy(), g=g.numpy(), open=o.numpy(), state=s.numpy())


def material(K, lead, seed, dtype, T=0):
    """``[*lead, T']`` with ``T' = max(T, 6 H + 400)``: phrases with quiet stretches of H - 1, H, H + 1 and 3 H + 7 samples one
    after the other (40 loud samples between them), a quiet lead-in and, near the end, a stretch between the two levels."""
    rng = np.random.default_rng(seed)
    H = K["H"]
    T = max(T, 6 * H + 400)
    runs, at = [], 60
    for n in (H - 1, H, H + 1, 3 * H + 7):
        runs.append((at, n))
        at += max(n, 0) + 40
    x = R.phrases(rng, tuple(lead) + (T,), K, runs, dtype)
    x[..., :20] = (x[..., :20] * (0.1 * K["p_close"] / K["p_open"])).astype(dtype)
    x[..., T - 60:T - 30] = 0.5 * (K["p_open"] + K["p_close"])         # between the levels: holds an open gate, opens no closed one
    return x


within = R.within


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("corner", list(CORNERS))
def test_host_path_against_the_loop(corner, dtype):
    kw = CORNERS[corner]
    K = R.constants(FS, **kw)
    x = material(K, (2, 2), 1, dtype)
    for link in (True, False):
        ref = R.gate_ref(x, K, link)
        assert 0.05 < ref["open"].mean() < 0.999 and ref["open"][:, -1].all()
        frac = within(run(x, link, **kw), ref, x, K, x.shape[-1], f"{corner} link={link}")
        print(f"{corner} {np.dtype(dtype).name} link={link}: gain error {frac:.3f} of the bound")


def test_host_block_seam_carries_the_counter_and_the_gain(monkeypatch):
    import importlib

    G = importlib.import_module("torchfx_amd.gate")                    # the package's attribute of that name is the function
    K = R.constants(FS, hold=5e-3)
    x = material(K, (1, 2), 2, np.float64, 3000)
    ref = R.gate_ref(x, K)
    for blk in (1, 7, 239, 240, 241, 4096):                            # H = 240: the quiet stretches straddle the block seams
        monkeypatch.setattr(G, "_HOST_BLOCK", blk)
        within(run(x, hold=5e-3), ref, x, K, x.shape[-1], f"block {blk}")


def test_hard_gate_is_exact():
    for range_db, r in ((math.inf, 0.0), (20.0, 10.0 ** (-20.0 / 20.0))):
        kw = dict(attack=0.0, release=0.0, range_db=range_db, hold=1e-3)
        K = R.constants(FS, **kw)
        assert K["r"] == r
        for dtype in (np.float32, np.float64):
            x = material(K, (2,), 3, dtype, 3000)
            got = run(x, **kw)
            op = got["open"][0].astype(bool)
            assert 0.05 < op.mean() < 0.99
            assert np.array_equal(got["g"][0], np.where(op, 1.0, r).astype(dtype))
            assert np.array_equal(got["y"][:, op], x[:, op])
            assert np.array_equal(got["y"][:, ~op], (r * x[:, ~op].astype(np.float64)).astype(dtype))


def test_always_open_group_comes_back_bit_identical():
    K = R.constants(FS)
    rng = np.random.default_rng(4)
    for dtype in (np.float32, np.float64):
        x = R.phrases(rng, (2, 2, 5000), K, [(1000, K["H"])], dtype)   # a stretch of exactly H samples does not close
        got = run(x, attack=0.0)
        assert got["open"].all() and np.array_equal(got["y"], x)
        assert np.array_equal(got["state"], np.array([[1.0, 1.0, 0.0]] * 2))


def test_levels_compare_at_exactly_the_host_doubles():
    K = R.constants(FS, hold=0.0, attack=0.0, release=0.0)
    po, pc = K["p_open"], K["p_close"]
    below = lambda v: np.nextafter(v, 0.0)                             # noqa: E731
    # closed: only p >= P_open opens; open (hold 0): p >= P_close holds, below it closes at once
    x = np.array([below(po), po, pc, below(pc), pc, below(po), po, below(pc), -po, -pc, -below(pc)])
    got = run(x, hold=0.0, attack=0.0, release=0.0)
    assert got["open"][0].tolist() == [0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 0]
    assert np.array_equal(got["open"], R.gate_ref(x, K)["open"])


@pytest.mark.parametrize("chunk", [1, 7, 2048, 2049])
def test_state_round_trip_equals_one_piece(chunk):
    kw = dict(hold=3e-3, range_db=30.0)
    K = R.constants(FS, **kw)
    T = 1500 if chunk == 1 else 6200
    x = material(K, (2, 2), 5, np.float32, T)
    ref = R.gate_ref(x, K)
    st, parts = None, {"y": [], "g": [], "open": []}
    for n0 in range(0, T, chunk):
        got = run(np.ascontiguousarray(x[..., n0:n0 + chunk]), state=st, **kw)
        st = got["state"]
        for k in parts:
            parts[k].append(got[k])
    whole = {k: np.concatenate(v, -1) for k, v in parts.items()}
    whole["state"] = st
    within(whole, ref, x, K, T, f"chunks of {chunk}")
    one = run(x, **kw)
    assert np.array_equal(whole["open"], one["open"]) and np.array_equal(st[:, 1:], one["state"][:, 1:])


def test_state_is_independent_of_the_cut_and_has_c_zero_when_closed():
    K = R.constants(FS, hold=2e-3)
    x = material(K, (1,), 6, np.float64, 4000)
    x[..., -500:] = 0.0                                                # ends closed
    got = run(x, hold=2e-3)
    assert got["state"][0, 1:].tolist() == [0.0, 0.0]
    x[..., -50:] = 2 * K["p_open"]
    x[..., -7:] = 0.0                                                  # ends open, 7 samples into the hold
    assert run(x, hold=2e-3)["state"][0, 1:].tolist() == [1.0, 7.0]


def test_poison_is_contained():
    K = R.constants(FS)
    x = material(K, (3, 2), 7, np.float64)
    T = x.shape[-1]
    clean = run(x)
    for bad in (np.nan, np.inf, -np.inf):
        z = x.copy()
        z[1, 1, 2047] = bad
        got = run(z)
        ref = R.gate_ref(z, K)
        within(got, ref, z, K, T, f"poison {bad}")
        for k in ("y", "g", "open"):
            assert np.array_equal(got[k][[0, 2]], clean[k][[0, 2]]) and np.array_equal(got[k][1][..., :2047], clean[k][1][..., :2047])
        assert np.isnan(got["y"][1][..., 2047:]).all() and np.isnan(got["g"][1, 2047:]).all() and not got["open"][1, 2047:].any()
        assert np.isnan(got["state"][1]).all() and np.array_equal(got["state"][[0, 2]], clean["state"][[0, 2]])
        again = run(x[1:2], state=got["state"][1:2])                   # a poisoned state stays poisoned
        assert np.isnan(again["y"]).all() and not again["open"].any() and np.isnan(again["state"]).all()


def test_empty_signal_returns_empty_tensors_and_the_state_unchanged():
    f = fx()
    x = torch.zeros(2, 2, 0)
    y, g, o, st = f.gate(x, FS, range_db=20.0, return_gain=True, return_open=True, return_state=True)
    assert y.shape == (2, 2, 0) and g.shape == (2, 0) and o.shape == (2, 0) and o.dtype == torch.uint8
    assert torch.equal(st, torch.tensor([[0.1, 0.0, 0.0]] * 2, dtype=torch.float64))
    s0 = torch.tensor([[0.5, 1.0, 17.0], [0.25, 0.0, 0.0]], dtype=torch.float64)
    assert torch.equal(f.gate(x, FS, state=s0, return_state=True)[1], s0)
    assert f.gate(torch.zeros(0), FS).shape == (0,)


def test_return_order_and_shapes():
    f = fx()
    x = torch.rand(3, 2, 100)
    assert isinstance(f.gate(x, FS), torch.Tensor)
    y, o = f.gate(x, FS, return_open=True)
    assert o.dtype == torch.uint8 and o.shape == (3, 100)
    y, g, o, st = f.gate(x, FS, link=False, return_gain=True, return_open=True, return_state=True)
    assert g.shape == (6, 100) and g.dtype == x.dtype and o.shape == (6, 100) and st.shape == (6, 3) and st.dtype == torch.float64
    assert f.gate(x[0, 0], FS, return_gain=True)[1].shape == (1, 100)


def test_parameter_errors():
    f = fx()
    x = torch.zeros(2, 64)
    g = f.gate
    for kw in (dict(threshold_db=math.inf), dict(threshold_db=math.nan), dict(threshold_db="x"), dict(threshold_db=True)):
        with pytest.raises(ValueError, match="threshold_db must be a finite level"):
            g(x, FS, **kw)
    for kw in (dict(hysteresis_db=-1.0), dict(hysteresis_db=math.inf), dict(hysteresis_db=math.nan)):
        with pytest.raises(ValueError, match="hysteresis_db must be a finite width >= 0"):
            g(x, FS, **kw)
    for kw in (dict(range_db=-1.0), dict(range_db=math.nan)):
        with pytest.raises(ValueError, match="range_db must be >= 0"):
            g(x, FS, **kw)
    g(x, FS, range_db=math.inf)
    for name in ("attack", "hold", "release"):
        for v in (-1e-3, math.inf, math.nan):
            with pytest.raises(ValueError, match=f"{name} must be a finite time >= 0"):
                g(x, FS, **{name: v})
    with pytest.raises(ValueError, match="exceeds the limit of 2\\^31 - 1"):
        g(x, FS, hold=2 ** 31 / FS)
    g(x, FS, hold=(2 ** 31 - 1) / FS)
    with pytest.raises(ValueError, match="not a positive finite linear level"):
        g(x, FS, threshold_db=-8000.0)
    with pytest.raises(TypeError, match="float32 or float64"):
        g(torch.zeros(2, 64, dtype=torch.float16), FS)
    with pytest.raises(TypeError):
        g(torch.zeros(2, 64, dtype=torch.int32), FS)
    with pytest.raises(ValueError, match=r"state must have shape \[groups, 3\] = \[1, 3\]"):
        g(x, FS, state=torch.zeros(1, 2))
    with pytest.raises(ValueError, match=r"\[2, 3\]"):
        g(x, FS, link=False, state=torch.zeros(1, 3))
    with pytest.raises(TypeError, match="state must be a torch.Tensor"):
        g(x, FS, state=np.zeros((1, 3)))
    with pytest.raises(ValueError):
        g(torch.zeros(1, 1, 2, 8), FS)
    with pytest.raises(ValueError, match="sample rate"):
        f.Gate()(x)
    with pytest.raises(ValueError, match="hysteresis_db"):
        f.Gate(hysteresis_db=-3)


def test_params_hold_the_definitions_constants():
    from torchfx_amd.gate import GateParams

    P = GateParams(FS, torch.float32, -37.5, 4.5, 26.0, 2e-3, 33e-3, 0.25)
    K = R.constants(FS, -37.5, 4.5, 26.0, 2e-3, 33e-3, 0.25)
    assert (P.p_open, P.p_close, P.r, P.H, P.aA, P.aR, P.bA, P.bR) == tuple(K[k] for k in ("p_open", "p_close", "r", "H", "aA", "aR", "bA", "bR"))
    assert P.H == 1584 and GateParams(FS, torch.float64, range_db=math.inf).r == 0.0
    assert GateParams(FS, torch.float32, attack=0.0, release=0.0).key()[-2:] == (0.0, 0.0)
    assert P.key() != GateParams(FS, torch.float32).key()


# ---- the boundary ----------------------------------------------------------------------------------------------------------

def test_plan_info_without_a_device():
    from torchfx_amd import torchfx_ext as E

    info = E.gate_plan_info(3 * 2048 + 5, 1, 2)
    assert info["tile"] == 2048 and info["tiles"] == 4 and info["segments"] == 4
    assert E.gate_plan_info(3 * 2048 + 5, 1, 2, 3) == {"tile": 2048, "tiles": 4, "segments": 3, "seg_tiles": 2, "scratch_bytes": 96}
    assert E.gate_plan_info(3 * 2048 + 5, 1, 2, 100)["segments"] == 4
    one = E.gate_plan_info(48000, 4096, 2)                             # the groups alone fill the chip
    assert one["segments"] == 1 and one["scratch_bytes"] == 0 and one["seg_tiles"] == one["tiles"]
    assert E.gate_plan_info(48000, 512, 1)["segments"] == 1 and E.gate_plan_info(48000, 511, 1)["segments"] == 3
    long_row = E.gate_plan_info(28_800_000, 2, 2)
    assert long_row["segments"] == 512 and long_row["scratch_bytes"] == 2 * 512 * 32
    assert E.gate_plan_info(0, 1, 1)["tiles"] == 0
    with pytest.raises(RuntimeError, match="segments"):
        E.gate_plan_info(100, 1, 1, -1)
    with pytest.raises(RuntimeError, match="channels"):
        E.gate_plan_info(100, 1, 0)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from torchfx_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(x=p, y=p, gain=None, open=None, dtype=0, groups=1, channels=1, T=32, po=0.01, pc=0.005, r=0.0, H=2400, aa=0.9, ar=0.99,
              sin=None, sout=None, seg=0, scratch=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tfx_gate_forward(a["x"], a["y"], a["gain"], a["open"], a["dtype"], a["groups"], a["channels"], a["T"], a["po"],
                                    a["pc"], a["r"], a["H"], a["aa"], a["ar"], a["sin"], a["sout"], a["seg"], a["scratch"], None)
    bad = [dict(x=None), dict(y=None), dict(dtype=7), dict(groups=-1), dict(T=-1), dict(channels=0), dict(po=math.inf), dict(po=0.0),
           dict(po=math.nan), dict(pc=0.02), dict(pc=-1.0), dict(pc=math.nan), dict(r=1.5), dict(r=-0.1), dict(r=math.nan),
           dict(H=-1), dict(H=2 ** 31), dict(aa=1.5), dict(aa=-0.5), dict(ar=math.nan), dict(seg=-1), dict(T=3 * 2048, seg=2),
           dict(sin=p, sout=p)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"gate_forward" in lib.tfx_last_error(), kw
    assert b"scratch" in (call(T=3 * 2048, seg=2), lib.tfx_last_error())[1]
    assert call(groups=0) == 0 and call(T=0) == 0                      # empty work is fine and touches nothing
    assert call(H=2 ** 31 - 1, T=0) == 0 and call(pc=0.01, T=0) == 0
    i64 = ctypes.c_int64
    outs = [i64() for _ in range(5)]
    assert lib.tfx_gate_plan_info(1, 1, 100, 0, *[ctypes.byref(o) for o in outs]) == 0
    assert [o.value for o in outs] == [2048, 1, 1, 1, 0]
    assert lib.tfx_gate_plan_info(1, 1, 100, 0, None, *[ctypes.byref(o) for o in outs[1:]]) != 0
    assert lib.tfx_gate_plan_info(-1, 1, 100, 0, *[ctypes.byref(o) for o in outs]) != 0


def test_gate_namespace_census():
    """Exactly the op of ``torchfx_gate``, with a device kernel, the CPU refusal and shape inference."""
    from torchfx_amd import native

    ns = native.gate_ops()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_gate::")}
    assert names == {"torchfx_gate::gate_forward"}
    for name in names:
        for key in ("CUDA", "CPU", "Meta"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(name, key), (name, key)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.gate_forward(torch.zeros(2, 8), 0.01, 0.005, 0.0, 10, 0.9, 0.99, 2, None, False, False)
    from torchfx_amd import torchfx_ext as E
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.gate_forward(torch.zeros(2, 8), 0.01, 0.005, 0.0, 10, 0.9, 0.99)
    y, g, o, st = ns.gate_forward(torch.empty(3, 2, 50, device="meta"), 0.01, 0.005, 0.0, 10, 0.9, 0.99, 2, None, True, True, 0)
    assert y.shape == (3, 2, 50) and g.shape == (3, 50) and o.shape == (3, 50) and o.dtype == torch.uint8
    assert st.shape == (3, 3) and st.dtype == torch.float64


# ---- planner and effect ------------------------------------------------------------------------------------------------------

def test_planner_keeps_the_gate_as_a_step_of_its_own():
    f = fx()
    K = R.constants(FS, -30.0)
    x = torch.from_numpy(material(K, (2,), 8, np.float32))
    gt, comp = f.Gate(-30.0), f.Compressor(-18, 3)
    w = f.Wave(x, FS) | f.filter.HiButterworth(100, order=2) | f.Gain(0.9) | gt | f.Gain(1.1) | comp
    plan = w.plan()
    assert sum(m is gt for m in plan) == 1 and gt.fs == FS
    k = plan.index(gt)
    assert 0 < k < plan.index(comp)
    lines = w.explain()
    assert lines[k] == "Gate: numpy on host -- cpu tensor" and lines[plan.index(comp)].startswith("Compressor: numpy on host")
    y = (f.Wave(x, FS) | f.Gate(-30.0)).ys
    assert torch.equal(y, f.gate(x, FS, -30.0))
    assert "threshold_db=-30.0" in repr(gt) and "range_db=inf" in repr(gt)
    from torchfx_amd.gate import GateParams
    assert gt.params(torch.float32).key() == GateParams(FS, torch.float32, -30.0).key()


def test_plan_cache_sees_a_changed_gate_parameter():
    f = fx()
    K = R.constants(FS, -30.0)
    x = torch.from_numpy(material(K, (2,), 9, np.float32))
    gt = f.Gate(-30.0, fs=FS)
    w = f.Wave(x, FS) | gt
    a = w.ys.clone()
    gt.range_db = 6.0
    b = (f.Wave(x, FS) | gt).ys
    assert not torch.equal(a, b) and torch.equal(b, f.gate(x, FS, -30.0, range_db=6.0))
