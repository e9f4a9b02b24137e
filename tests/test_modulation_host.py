"""The modulated delay line without a device: the NumPy host path of torchfx_amd.modulation.modulated_delay against the
per-sample loop of tests/modulation_reference.py within the derived bound, the exact cases of the definition, argument errors,
the plan query and the C ABI's refusals, Chorus / Flanger / Vibrato in a Wave, the planner, the torchfx_modulation namespace and
the stateful classes over CPU chunks."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import modulation_reference as R

FS = 48000
# (delay, depth, rate, phase, gain), delay and depth in samples: a read next to the sample, one a few hundred samples back with
# a deep sweep, one past the end of the short signals
VOICES = [(1.5, 0.4, 3.0, 0.0, 0.5), (300.25, 200.5, 0.7, 0.3, -0.4), (640.0, 0.0, 1.0, 0.6, 0.3)]


def fx():
    import torchfx_amd
    return torchfx_amd


def signal(shape, seed=0, dtype=np.float64):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(dtype)


def host(x, voices=VOICES, **kw):
    return fx().modulated_delay(torch.from_numpy(np.ascontiguousarray(x)), FS, voices, **kw).numpy()


# ---- the host path against the loop -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("position", [0, 2 ** 40], ids=["p0", "p2^40"])
@pytest.mark.parametrize("shape", [(700,), (2, 700), (3, 2, 700)], ids=["T", "CT", "BCT"])
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
@pytest.mark.parametrize("lfo", ["sine", "triangle"])
def test_host_path_against_the_definition(lfo, interpolation, shape, position):
    dtype = np.float32 if len(shape) == 2 else np.float64
    x = signal(shape, len(shape), dtype)
    kw = dict(dry=0.7, spread=0.25, shape=lfo, interpolation=interpolation, position=position)
    ref = R.modulated_delay_ref(x, FS, VOICES, **kw)
    R.at_work(ref, x, FS, VOICES, 0.7)
    got = host(x, **kw)
    assert got.dtype == x.dtype
    R.check(got, ref, x, FS, VOICES, 0.7, what=f"{lfo} {interpolation} {shape} at {position}")


def test_spread_moves_the_channels_apart_and_position_moves_the_lfo():
    x = np.tile(signal((1, 900), 5), (2, 1))
    same = host(x, spread=0.0, dry=0.0)
    apart = host(x, spread=0.25, dry=0.0)
    assert np.array_equal(same[0], same[1]) and np.array_equal(apart[0], same[0]) and not np.array_equal(apart[0], apart[1])
    assert not np.array_equal(host(x, dry=0.0, position=12345), same)


def test_host_path_crosses_its_block_seam(monkeypatch):
    from torchfx_amd import modulation

    x = signal((2, 1000), 6)
    whole = host(x, interpolation="cubic", spread=0.1)
    monkeypatch.setattr(modulation, "_HOST_BLOCK", 333)
    assert np.array_equal(host(x, interpolation="cubic", spread=0.1), whole)


# ---- the exact cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("interpolation,lfo", [("linear", "sine"), ("cubic", "triangle")])
def test_integer_delay_is_an_exact_copy(interpolation, lfo, dtype):
    x = signal((2, 500), 7, dtype)
    for D in (1, 37, 499, 500, 1200):
        y = host(x, [(float(D), 0.0, 2.0, 0.3, 1.0)], dry=0.0, interpolation=interpolation, shape=lfo, position=3)
        want = np.zeros_like(x)
        want[:, D:] = x[:, :max(0, 500 - D)]
        assert np.array_equal(y, want), D
    assert np.array_equal(host(x, [(0.0, 0.0, 2.0, 0.0, 1.0)], dry=0.0), x)          # a linear delay of 0 is the signal itself


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_silent_voices_return_the_input(dtype):
    x = signal((3, 2, 400), 8, dtype)
    silent = [(b, d, r, p, 0.0) for b, d, r, p, _ in VOICES]
    for interpolation in ("linear", "cubic"):
        assert np.array_equal(host(x, silent, dry=1.0, spread=0.3, interpolation=interpolation), x)


def test_equal_batch_items_give_equal_rows_and_a_row_does_not_see_its_batch():
    one = signal((2, 600), 9, np.float32)
    x = np.stack([one, signal((2, 600), 10, np.float32), one])
    y = host(x, spread=0.25, interpolation="cubic")
    assert np.array_equal(y[0], y[2]) and not np.array_equal(y[0], y[1])
    assert np.array_equal(y[0], host(one, spread=0.25, interpolation="cubic"))


def test_a_non_finite_sample_stays_in_its_window():
    x = signal((2, 900), 11)
    clean = host(x, interpolation="cubic")
    reach = math.floor(max(b + d for b, d, *_ in VOICES)) + 2
    for m in (0, 450, 899):
        for bad in (np.nan, np.inf):
            xb = x.copy()
            xb[1, m] = bad
            y = host(xb, interpolation="cubic")
            keep = np.ones(900, bool)
            keep[m:m + reach + 1] = False
            assert np.array_equal(y[0], clean[0]) and np.array_equal(y[1, keep], clean[1, keep])
            assert not np.isfinite(y[1, m])


def test_empty_signal_and_return_form():
    y = fx().modulated_delay(torch.zeros(2, 0), FS, VOICES)
    assert y.shape == (2, 0) and y.dtype == torch.float32


# ---- argument errors --------------------------------------------------------------------------------------------------------

def test_argument_errors():
    f = fx()
    x = torch.zeros(2, 64)
    ok = (10.0, 2.0, 1.0, 0.0, 0.5)
    bad_values = [
        (dict(voices=[]), "number of voices"),
        (dict(voices=[ok] * 9), "number of voices"),
        (dict(voices=[(10.0, 2.0, 1.0, 0.0)]), "must be \\(delay, depth, rate, phase, gain\\)"),
        (dict(voices=[(-1.0, 0.0, 1.0, 0.0, 0.5)]), ">= 0 samples"),
        (dict(voices=[(10.0, -2.0, 1.0, 0.0, 0.5)]), ">= 0 samples"),
        (dict(voices=[(1.0, 2.0, 1.0, 0.0, 0.5)]), "delay - depth must be >= 0"),
        (dict(voices=[(2.5, 2.0, 1.0, 0.0, 0.5)], interpolation="cubic"), "delay - depth must be >= 1"),
        (dict(voices=[(2.0 ** 24 - 2.0, 0.0, 1.0, 0.0, 0.5)]), "below 2\\^24 - 3"),
        (dict(voices=[(10.0, 2.0, 0.0, 0.0, 0.5)]), "rate must be in"),
        (dict(voices=[(10.0, 2.0, 24000.0, 0.0, 0.5)]), "rate must be in"),
        (dict(voices=[(10.0, 2.0, math.nan, 0.0, 0.5)]), "finite rate"),
        (dict(voices=[(10.0, 2.0, 1.0, math.inf, 0.5)]), "finite phase"),
        (dict(voices=[(10.0, 2.0, 1.0, 0.0, math.nan)]), "finite gain"),
        (dict(voices=[(math.inf, 2.0, 1.0, 0.0, 0.5)]), "finite number of samples"),
        (dict(voices=[(True, 2.0, 1.0, 0.0, 0.5)]), "finite number of samples"),
        (dict(dry=math.nan), "dry must be"),
        (dict(spread=math.inf), "spread must be"),
        (dict(shape="square"), "shape must be one of"),
        (dict(interpolation="sinc"), "interpolation must be one of"),
        (dict(position=-1), "position must be"),
        (dict(position=2 ** 52 + 1), "position must be"),
        (dict(position=1.5), "position must be"),
        (dict(fs=100), "fs must be"),
    ]
    for kw, match in bad_values:
        a = dict(dict(fs=FS, voices=[ok]), **kw)
        with pytest.raises(ValueError, match=match):
            f.modulated_delay(x, a.pop("fs"), a.pop("voices"), **a)
    with pytest.raises(TypeError, match="float32 or float64"):
        f.modulated_delay(torch.zeros(2, 64, dtype=torch.float16), FS, [ok])
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        f.modulated_delay(np.zeros(8), FS, [ok])
    with pytest.raises(TypeError, match="sequence of"):
        f.modulated_delay(x, FS, 3)
    with pytest.raises(ValueError, match="shape"):
        f.modulated_delay(torch.zeros(2, 2, 2, 8), FS, [ok])
    # the effects check their arguments when they are built
    with pytest.raises(ValueError, match="number of voices"):
        f.Chorus(voices=9)
    with pytest.raises(ValueError, match="delay - depth"):
        f.Chorus(depth=30e-3, delay=20e-3)
    with pytest.raises(ValueError, match="rate must be in"):
        f.Vibrato(rate=0.0)
    with pytest.raises(ValueError, match="finite time"):
        f.Flanger(depth=-1e-3)
    with pytest.raises(ValueError, match="interpolation must be one of"):
        f.Flanger(interpolation="nearest")
    with pytest.raises(ValueError, match="needs the sample rate"):
        f.Chorus()(x)


def test_plan_info_without_a_device():
    from torchfx_amd import torchfx_ext as E

    q = E.modulated_delay_plan_info(3 * 1024 + 17, [(960.0, 512.0, 5.0 / FS, 0.0, 0.5), (3.5, 1.0, 1.0 / FS, 0.0, 0.5)], batch=5, channels=2)
    assert q == dict(tile=1024, tiles=4, history=1474, batch_items=4, batch_groups=2)
    assert E.modulated_delay_plan_info(0, [(1.0, 0.0, 0.1, 0.0, 1.0)])["tiles"] == 0
    with pytest.raises(RuntimeError, match="voices"):
        E.modulated_delay_plan_info(100, np.zeros((9, 5)) + 0.1)
    with pytest.raises(RuntimeError, match="cubic"):
        E.modulated_delay_plan_info(100, [(0.5, 0.0, 0.1, 0.0, 1.0)], interpolation="cubic")
    with pytest.raises(RuntimeError, match="channels"):
        E.modulated_delay_plan_info(100, [(1.0, 0.0, 0.1, 0.0, 1.0)], channels=0)


def test_c_abi_refuses_bad_arguments_before_the_device():
    from torchfx_amd import _lib

    lib = _lib.load()
    buf, out, hin, hout = [(ctypes.c_float * 256)() for _ in range(4)]
    pos = [(ctypes.c_int64 * 1)() for _ in range(2)]
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)                     # noqa: E731
    table = lambda *rows: (ctypes.c_double * (5 * len(rows)))(*[t for r in rows for t in r])      # noqa: E731
    good = (4.0, 1.0, 1e-4, 0.0, 0.5)
    ok = dict(x=vp(buf), y=vp(out), dtype=0, batch=1, channels=2, T=32, voices=table(good), V=1, spread=0.0, dry=1.0, shape=0, interp=0,
              position=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tfx_modulated_delay_forward(a["x"], a["y"], a["dtype"], a["batch"], a["channels"], a["T"], vp(a["voices"]), a["V"],
                                               a["spread"], a["dry"], a["shape"], a["interp"], a["position"], None)
    bad = [dict(x=None), dict(y=None), dict(y=vp(buf)), dict(dtype=7), dict(batch=-1), dict(T=-1), dict(channels=0), dict(voices=None),
           dict(V=0), dict(V=9), dict(shape=2), dict(interp=-1), dict(spread=math.nan), dict(dry=math.inf), dict(position=-1),
           dict(position=2 ** 52 + 1), dict(voices=table((1.0, 2.0, 1e-4, 0.0, 0.5))), dict(voices=table((1.5, 1.0, 1e-4, 0.0, 0.5)), interp=1),
           dict(voices=table((4.0, 1.0, 0.5, 0.0, 0.5))), dict(voices=table((4.0, 1.0, 0.0, 0.0, 0.5))),
           dict(voices=table((2.0 ** 24, 0.0, 1e-4, 0.0, 0.5))), dict(voices=table((4.0, 1.0, 1e-4, math.nan, 0.5))),
           dict(voices=table((4.0, 1.0, 1e-4, 0.0, math.inf))), dict(voices=table((-1.0, 0.0, 1e-4, 0.0, 0.5)))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"modulated_delay_forward" in lib.tfx_last_error(), kw
    assert call(batch=0) == 0 and call(T=0) == 0                       # empty work is fine and touches nothing

    def stream(**kw):
        a = dict(dict(ok, hin=vp(hin), hout=vp(hout), pin=vp(pos[0]), pout=vp(pos[1])), **kw)
        return lib.tfx_modulated_delay_stream_forward(a["x"], a["y"], a["dtype"], a["batch"], a["channels"], a["T"], vp(a["voices"]),
                                                      a["V"], a["spread"], a["dry"], a["shape"], a["interp"], a["hin"], a["hout"],
                                                      a["pin"], a["pout"], None)
    for kw in [dict(hout=None), dict(hout=vp(hin)), dict(hout=vp(buf)), dict(y=vp(hin)), dict(y=vp(buf)), dict(pout=vp(pos[0])), dict(V=9),
               dict(interp=3), dict(x=None)]:
        assert stream(**kw) != 0, kw
        assert b"modulated_delay_stream_forward" in lib.tfx_last_error(), kw
    assert stream(batch=0, pout=None) == 0
    i64 = ctypes.c_int64
    outs = [i64() for _ in range(5)]
    assert lib.tfx_modulated_delay_plan_info(1, 1, 100, vp(table(good)), 1, 0, *[ctypes.byref(o) for o in outs]) == 0
    assert [o.value for o in outs] == [1024, 1, 7, 4, 1]
    assert lib.tfx_modulated_delay_plan_info(1, 1, 100, vp(table(good)), 1, 0, None, *[ctypes.byref(o) for o in outs[1:]]) != 0
    assert lib.tfx_modulated_delay_plan_info(-1, 1, 100, vp(table(good)), 1, 0, *[ctypes.byref(o) for o in outs]) != 0


def test_modulation_namespace_census():
    """Exactly the two ops of ``torchfx_modulation``, each with a device kernel, the CPU refusal and shape inference."""
    from torchfx_amd import native
    from torchfx_amd import torchfx_ext as E

    ns = native.modulation_ops()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_modulation::")}
    assert names == {"torchfx_modulation::modulated_delay_forward", "torchfx_modulation::modulated_delay_stream_forward"}
    for name in names:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CPU"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "Meta"), name
    table = torch.tensor([[960.0, 512.0, 1e-4, 0.0, 0.5]], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.modulated_delay_forward(torch.zeros(2, 8), table, 0.0, 1.0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.modulated_delay_stream_forward(torch.zeros(2, 8), None, None, table, 0.0, 1.0, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.modulated_delay_forward(torch.zeros(2, 8), table)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.modulated_delay_stream_forward(torch.zeros(2, 8), None, None, table)
    meta = torch.empty(3, 2, 50, device="meta")
    assert ns.modulated_delay_forward(meta, table, 0.0, 1.0, 0, 0, 0).shape == (3, 2, 50)
    y, h, p = ns.modulated_delay_stream_forward(meta, None, None, table, 0.0, 1.0, 0, 0)
    assert y.shape == (3, 2, 50) and h.shape == (6, 1474) and p.shape == (1,) and p.dtype == torch.int64
    assert {"modulated_delay_forward", "modulated_delay_stream_forward", "modulated_delay_plan_info"} <= set(E.__all__)
    assert {"Chorus", "Flanger", "Vibrato", "ModulatedDelay", "modulated_delay"} <= set(fx().__all__)


# ---- effects, planner, streams ----------------------------------------------------------------------------------------------

def test_the_three_effects_fill_the_voice_table():
    f = fx()
    ch = f.Chorus(fs=FS)
    P = ch.params(torch.float32)
    assert P.table.shape == (3, 5) and P.interpolation == "cubic" and P.dry == 0.5 and P.spread == 0.25
    assert np.array_equal(P.table[:, 0], [960.0] * 3) and np.array_equal(P.table[:, 1], [144.0] * 3)
    assert np.array_equal(P.table[:, 3], [0.0, 1 / 3, 2 / 3]) and np.array_equal(P.table[:, 4], [0.5 / 3] * 3)
    assert np.array_equal(P.table[:, 2], [1.5 / FS] * 3) and P.history == 1106
    vb = f.Vibrato(fs=FS).params(torch.float64)
    assert vb.table.tolist() == [[49.0, 48.0, 5.0 / FS, 0.0, 1.0]] and vb.dry == 0.0
    assert f.Vibrato(fs=FS, interpolation="linear").params(torch.float64).table[0, 0] == 48.0
    fl = f.Flanger(fs=FS, invert=True).params(torch.float32)
    assert fl.table.tolist() == [[144.0, 96.0, 0.25 / FS, 0.0, -0.5]] and fl.dry == 1.0
    assert "feed-forward" in f.Flanger.__doc__
    assert "rate=1.5" in repr(ch) and "interpolation='cubic'" in repr(ch) and "voices=3" in repr(ch)


def test_wave_gives_the_effect_its_rate_and_the_planner_keeps_it_as_one_step():
    f = fx()
    x = torch.from_numpy(signal((2, 3000), 12, np.float32))
    ch = f.Chorus()
    w = f.Wave(x, FS) | f.filter.HiButterworth(100, order=2) | f.Gain(0.9) | ch | f.Gain(1.1)
    assert ch.fs == FS
    plan = w.plan()
    assert sum(m is ch for m in plan) == 1
    k = plan.index(ch)
    assert 0 < k < len(plan) - 1
    assert w.explain()[k] == "Chorus: numpy on host -- cpu tensor"
    y = (f.Wave(x, FS) | f.Chorus()).ys
    P = ch.params(torch.float32)
    voices = [(b, d, 1.5, p, g) for b, d, _, p, g in P.table.tolist()]
    ref = R.modulated_delay_ref(x.numpy(), FS, voices, dry=0.5, spread=0.25, interpolation="cubic")
    R.at_work(ref, x.numpy(), FS, voices, 0.5)
    R.check(y.numpy(), ref, x.numpy(), FS, voices, 0.5, what="Wave | Chorus()")
    # a changed parameter is another plan
    assert (f.Wave(x, FS) | f.Chorus(rate=2.0)).ys.ne(y).any()


def test_stream_processors_refuse_the_plain_effects():
    from torchfx_amd import realtime as RT

    f = fx()

    class NoBackend(RT.AudioBackend):
        def open_stream(self, config, callback=None):
            raise AssertionError("the refusal comes before a stream is opened")

        def start(self):
            pass

        def stop(self):
            pass

        def close(self):
            pass

    for plain, stateful in ((f.Chorus, "StatefulChorus"), (f.Flanger, "StatefulFlanger"), (f.Vibrato, "StatefulVibrato")):
        with pytest.raises(TypeError, match=stateful):
            RT.StreamProcessor([plain()], chunk_size=256, device="cpu")
        with pytest.raises(TypeError, match=stateful):
            RT.StreamProcessor([f.Gain(0.5), plain(), f.Gain(2.0)], chunk_size=256, device="cpu")
        with pytest.raises(TypeError, match=stateful):
            RT.RealtimeProcessor([plain()], NoBackend(), RT.StreamConfig(), device="cpu")
        RT.StreamProcessor([getattr(RT, stateful)()], chunk_size=256, device="cpu")
    with pytest.raises(TypeError, match="StatefulChorus, StatefulFlanger, StatefulVibrato"):
        RT.StreamProcessor([f.ModulatedDelay([(1e-3, 0.0, 1.0, 0.0, 1.0)])], chunk_size=256, device="cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["Chorus", "Flanger", "Vibrato"])
def test_stateful_chunks_equal_the_one_shot_call(name, dtype):
    from torchfx_amd import realtime as RT

    x = torch.from_numpy(signal((2, 2600), 13)).to(dtype)
    whole = getattr(fx(), name)(fs=FS)(x)
    assert not torch.equal(whole, x)
    eff = getattr(RT, "Stateful" + name)(fs=FS)
    H = eff.params(dtype).history
    for size in (1, 7, 512):                                            # 1 and 7 are far below H; the last chunk is ragged
        eff.reset_state()
        n = 2600 if size > 1 else 300
        cuts = list(range(0, n, size)) + [n]
        y = torch.cat([eff(x[:, a:b].contiguous()) for a, b in zip(cuts, cuts[1:])], -1)
        assert y.dtype == dtype and torch.equal(y, whole[:, :n]), size
        assert eff._hist.shape == (2, H) and int(eff._pos) == n
        hist = torch.cat([torch.zeros(2, H, dtype=dtype), x[:, :n]], -1)[:, n:]
        assert torch.equal(eff._hist, hist)
    eff(x[:1, :10].contiguous())                                        # another row count: a new stream from position 0
    assert eff._hist.shape == (1, H) and int(eff._pos) == 10
    eff.reset_state()
    assert eff._hist is None and eff._pos is None


def test_stream_processor_runs_the_stateful_effects_over_cpu_chunks():
    from torchfx_amd import realtime as RT

    x = torch.from_numpy(signal((2, 4000), 14, np.float32))
    sp = RT.StreamProcessor([RT.StatefulFlanger(), RT.StatefulChorus()], chunk_size=512, device="cpu")
    y = sp.process_tensor(x, FS)
    f = fx()
    assert torch.equal(y, f.Chorus(fs=FS)(f.Flanger(fs=FS)(x)))
