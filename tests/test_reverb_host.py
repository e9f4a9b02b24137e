"""Freeverb without a device: the block-wise host path (torchfx_amd/reverb.py) against the per-sample loops of
tests/reverb_reference.py within its measured bound over the shared grid, the exact cases of the definition, every argument
error, the tunings' rounding rule, the effect, the planner, the stream classes on CPU chunks, the plan query and the C entry
points' argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from tests import reverb_reference as R

FS = 44100


def bank(x, comb, allpass, dtype=None, **kw):
    from torchfx_amd import freeverb_bank

    t = torch.from_numpy(np.array(x))
    return freeverb_bank(t.to(dtype or t.dtype), comb, allpass, **kw)


@pytest.mark.parametrize("case", R.BANK_GRID, ids=R.bank_id)
def test_host_path_matches_the_reference_over_the_grid(case):
    x, comb, allpass, kw, ref, ref_state = R.bank_case(case)
    for dt, nd in ((torch.float64, np.float64), (torch.float32, np.float32)):
        y, st = bank(x, comb, allpass, dt, return_state=True, **kw)
        assert y.dtype == dt and tuple(y.shape) == x.shape and st.dtype == torch.float64
        R.check(y.numpy(), ref, f"host {R.bank_id(case)} {nd.__name__}", nd)
        R.check(st.numpy(), ref_state, f"host state {R.bank_id(case)} {nd.__name__}")


@pytest.mark.parametrize("shape,fs", R.FREEVERB_CASES)
def test_freeverb_effect_matches_the_reference(shape, fs):
    from torchfx_amd import Freeverb, freeverb

    x, ref, _ = R.freeverb_case(shape, fs)
    for dt, nd in ((torch.float64, np.float64), (torch.float32, np.float32)):
        t = torch.from_numpy(np.array(x)).to(dt)
        y = Freeverb(fs=fs)(t)
        assert y.dtype == dt and y.shape == t.shape
        R.check(y.numpy(), ref, f"Freeverb {shape} {fs} {nd.__name__}", nd)
        assert torch.equal(y, freeverb(t, fs))


def test_width_and_tail_match_the_reference():
    from torchfx_amd import freeverb

    x, ref, _ = R.freeverb_case((2, 5000), FS, width=0.3, tail=300)
    t = torch.from_numpy(np.array(x)).double()
    y = freeverb(t, FS, width=0.3, tail=300 / FS)
    assert y.shape == (2, 5300)
    R.check(y.numpy(), ref, "width 0.3, tail 300")
    assert torch.equal(y, freeverb(torch.nn.functional.pad(t, (0, 300)), FS, width=0.3))


def impulse(shape, dtype=torch.float64):
    x = torch.zeros(shape, dtype=dtype)
    x[..., 0] = 1.0
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_exact_comb_echoes(dtype):
    """One comb, D = 37, fb = 0.5, damp = 0, no all-pass, input_gain = 1, a unit impulse on channel 0 of [2, T] (the feed is
    input_gain (2 / C) (x_0 + x_1) = 1 at n = 0): r[kD] = 0.5^(k-1) for k >= 1 and zero elsewhere, in both banks.  A mono
    signal feeds L = R, so there the same holds with input_gain = 0.5."""
    from torchfx_amd import freeverb_bank

    T = 400
    want = torch.zeros(T, dtype=dtype)
    for k in range(1, T // 37 + 1):
        want[37 * k] = 0.5 ** (k - 1)
    x = impulse((2, T), dtype)
    x[1] = 0.0
    y = freeverb_bank(x, [[37], [37]], (), 0.5, 0.0, input_gain=1.0, dry_gain=0.0, wet1=1.0)
    assert torch.equal(y[0], want) and torch.equal(y[1], want)
    assert torch.equal(freeverb_bank(impulse((T,), dtype), (37,), (), 0.5, 0.0, input_gain=0.5, dry_gain=0.0), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_exact_allpass_echoes(dtype):
    """A one-sample comb (D = 1, fb = 0) into one all-pass with D = 5, g = 0.5: r[1] = -1, r[1 + 5k] = 0.5^(k-1), zero elsewhere."""
    from torchfx_amd import freeverb_bank

    T = 200
    want = torch.zeros(T, dtype=dtype)
    want[1] = -1.0
    for k in range(1, (T - 2) // 5 + 1):
        want[1 + 5 * k] = 0.5 ** (k - 1)
    assert torch.equal(freeverb_bank(impulse((T,), dtype), (1,), (5,), 0.0, 0.0, 0.5, input_gain=0.5, dry_gain=0.0), want)


def test_dry_only_returns_the_input_bit_for_bit():
    from torchfx_amd import Freeverb

    for shape in ((3000,), (2, 3000), (2, 2, 3000)):
        x = torch.from_numpy(np.array(R.signal(shape, 5)))
        assert torch.equal(Freeverb(wet=0.0, dry=0.5, fs=FS)(x), x)


def test_batch_items_are_independent():
    from torchfx_amd import freeverb

    x = torch.from_numpy(np.array(R.signal((5, 2, 2500), 6)))
    y = freeverb(x, FS, width=0.5)
    for i in range(5):
        assert torch.equal(y[i], freeverb(x[i], FS, width=0.5))


@pytest.mark.parametrize("chunk", [1, 7, 64, 1000, 62, 63, 65, 66])
def test_chunked_calls_continue_the_network(chunk):
    """Chunks of 1, 7, 64, 1000 and D - 1, D, D + 1 around the comb delays 63 .. 65 (and the second channel's 65 .. 67), with a
    remainder, against the one-shot reference: outputs and the final state."""
    from torchfx_amd import freeverb_bank

    case = ("wave", "four", 0.9, 0.98, 4097, 2)
    x, comb, allpass, kw, ref, ref_state = R.bank_case(case)
    T = 1500 if chunk < 64 else 4097
    if T != 4097:
        ref, ref_state = R.freeverb_ref(x[..., :T], comb, allpass, **R._ref_kw(kw))
    t = torch.from_numpy(np.array(x[..., :T])).double()
    st, out = None, []
    for n0 in range(0, T, chunk):
        y, st = freeverb_bank(t[..., n0:n0 + chunk], comb, allpass, state=st, return_state=True, **kw)
        out.append(y)
    R.check(torch.cat(out, -1).numpy(), ref, f"host chunks of {chunk}")
    R.check(st.numpy(), ref_state, f"host state after chunks of {chunk}")


def test_argument_errors():
    from torchfx_amd import Freeverb, freeverb, freeverb_bank

    x = torch.zeros(2, 100)
    ok = dict(comb_delays=[[10, 11], [12, 13]], allpass_delays=[[3], [4]], feedback=0.5, damp=0.2)

    def call(x=x, **kw):
        return freeverb_bank(x, **{**ok, **kw})

    call()
    bad_value = [
        dict(x=torch.zeros(3, 100)), dict(x=torch.zeros(2, 3, 100)), dict(x=torch.zeros(1, 2, 2, 100)),
        dict(comb_delays=[[10, 11]]), dict(comb_delays=[[], []]), dict(comb_delays=[list(range(1, 10))] * 2),
        dict(allpass_delays=[[1, 2, 3, 4, 5]] * 2), dict(allpass_delays=[[3]]), dict(comb_delays=[[0, 5], [5, 5]]),
        dict(comb_delays=[[5, 65537], [5, 5]]), dict(allpass_delays=[[0], [1]]), dict(feedback=1.0), dict(feedback=-1.0),
        dict(feedback=float("nan")), dict(damp=-0.1), dict(damp=1.0), dict(damp=float("inf")), dict(allpass_gain=1.0),
        dict(allpass_gain=-1.5), dict(input_gain=float("inf")), dict(dry_gain=float("nan")), dict(wet1=float("inf")),
        dict(wet2=float("nan")), dict(tail_samples=-1), dict(tail_samples=1.5), dict(state=torch.zeros(2, 5)),
        dict(feedback=True),
    ]
    for kw in bad_value:
        with pytest.raises(ValueError, match="freeverb|Input must be"):
            call(**kw)
    bad_type = [dict(x=np.zeros((2, 100))), dict(x=torch.zeros(2, 100, dtype=torch.int32)), dict(x=torch.zeros(2, 100, dtype=torch.float16)),
                dict(comb_delays=[[10.0, 11.0], [12.0, 13.0]]), dict(allpass_delays=[[True], [False]]), dict(state=np.zeros((2, 32)))]
    for kw in bad_type:
        with pytest.raises(TypeError, match="freeverb"):
            call(**kw)
    for kw in (dict(room_size=1.1), dict(damping=-0.1), dict(wet=2.0), dict(dry=float("nan")), dict(width=1.5), dict(tail=-1.0),
               dict(tail=float("inf")), dict(fs=100), dict(room_size="big")):
        with pytest.raises(ValueError):
            Freeverb(**kw)
        if "fs" not in kw:
            with pytest.raises(ValueError):
                freeverb(x, FS, **kw)
    with pytest.raises(ValueError, match="needs the sample rate"):
        Freeverb()(x)
    with pytest.raises(ValueError, match="1 or 2 channels"):
        Freeverb(fs=FS)(torch.zeros(3, 100))
    # empty signals: nothing in, the tail out; the state moves on unchanged
    st = torch.arange(2.0 * 31).reshape(2, 31).double()
    y, so = call(x=torch.zeros(2, 0), state=st, return_state=True)
    assert y.shape == (2, 0) and torch.equal(so, st)
    assert call(x=torch.zeros(2, 0), tail_samples=7).shape == (2, 7)


def test_tunings_follow_the_rounding_rule():
    from torchfx_amd.reverb import tunings

    for fs in (44100, 48000, 96000, 8000, 192000):
        comb, allpass = tunings(fs, 2)
        rc, ra = R.tunings(fs, 2)
        assert comb.tolist() == rc and allpass.tolist() == ra
    comb, allpass = tunings(44100, 2)
    assert comb[0].tolist() == list(R.COMB_TUNING) and comb[1].tolist() == [t + 23 for t in R.COMB_TUNING]
    assert allpass[0].tolist() == list(R.ALLPASS_TUNING) and allpass[1].tolist() == [t + 23 for t in R.ALLPASS_TUNING]
    assert tunings(48000, 1)[0].tolist() == [[1215, 1293, 1390, 1476, 1548, 1623, 1695, 1760]]
    assert tunings(96000, 2)[1][1].tolist() == [1260, 1010, 792, 540]


def test_freeverb_piped_from_a_wave_takes_its_rate_and_is_a_step_of_its_own():
    from torchfx_amd import Freeverb, Gain, Wave, freeverb

    x = torch.from_numpy(np.array(R.signal((2, 3000), 8)))
    fx = Freeverb(room_size=0.7, tail=0.01)
    w = Wave(x, fs=48000) | Gain(0.5) | fx | Gain(2.0)
    assert fx.fs == 48000
    plan = w.plan()
    assert [type(m).__name__ for m in plan] == ["Gain", "Freeverb", "Gain"]
    lines = w.explain()
    assert len(lines) == 3 and lines[1].startswith("Freeverb: numpy on host -- cpu tensor")
    alone = Wave(x, fs=48000) | Freeverb(room_size=0.7, tail=0.01)          # Gain has no host path: the values without it
    assert alone.ys.shape == (2, 3480) and torch.equal(alone.ys, freeverb(x, 48000, room_size=0.7, tail=0.01))
    assert "room_size=0.7" in repr(fx)


def test_route_names_the_kernel_the_placement_and_the_launches():
    """route() on a meta-free host: a CPU tensor names the host path; the native wording is built from the plan query, checked
    here through the query itself (tests/test_gpu_reverb.py checks route() on device tensors)."""
    from torchfx_amd import Freeverb

    assert Freeverb(fs=FS).route(torch.zeros(2, 100)) == "numpy on host -- cpu tensor"


def test_plan_info_without_a_device():
    from torchfx_amd import torchfx_ext as E
    from torchfx_amd.reverb import tunings

    comb, allpass = tunings(44100, 2)
    S = int((comb.sum(1) + 8 + allpass.sum(1)).max())
    assert E.freeverb_plan_info(5000, comb, allpass, batch=3, channels=2) == dict(
        block=1024, placement="lds", state_len=S, launches=1, workspace_bytes=0)
    assert E.freeverb_plan_info(5000, comb, allpass, batch=3, channels=2, wet2=0.1, tail=10) == dict(
        block=1024, placement="lds", state_len=S, launches=2, workspace_bytes=6 * 5010 * 8)
    assert E.freeverb_plan_info(5000, comb[:1], allpass[:1], channels=1, wet2=0.1)["launches"] == 1
    assert E.freeverb_plan_info(100, *tunings(48000, 2), channels=2)["placement"] == "lds"
    q = E.freeverb_plan_info(100, *tunings(96000, 2), batch=2, channels=2)
    words = int(max(tunings(96000, 2)[0][c].sum() + tunings(96000, 2)[1][c].sum() for c in range(2)))
    assert q["placement"] == "global" and q["workspace_bytes"] == 4 * words * 8 and q["launches"] == 1
    assert E.freeverb_plan_info(6000, [[2500 + 7 * k for k in range(8)]], (), channels=1)["placement"] == "global"
    assert E.freeverb_plan_info(10, [[70, 83, 1, 200]], [[5]], channels=1) == dict(
        block=1, placement="lds", state_len=70 + 83 + 1 + 200 + 4 + 5, launches=1, workspace_bytes=0)
    assert E.freeverb_plan_info(10, [[63, 64, 65]], (), channels=1)["block"] == 63
    for bad in (dict(channels=3, comb_delays=[[5]] * 3), dict(comb_delays=[[0]]), dict(comb_delays=[[70000]]),
                dict(comb_delays=[list(range(1, 10))]), dict(allpass_delays=[[1, 2, 3, 4, 5]]), dict(length=-1), dict(tail=-1)):
        kw = dict(length=10, comb_delays=[[5]], allpass_delays=(), channels=1)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="freeverb_plan_info"):
            E.freeverb_plan_info(**kw)


def test_c_entry_points_check_their_arguments_before_the_device():
    from torchfx_amd import _lib
    lib = _lib.load()
    comb = (ctypes.c_int64 * 2)(10, 11)
    ap = (ctypes.c_int64 * 1)(3)
    outs = [ctypes.c_int64(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()]
    ptrs = [ctypes.byref(o) for o in outs]

    def fwd(x=None, y=None, dtype=0, batch=1, channels=1, T=100, tail=0, comb=comb, NC=2, ap=ap, NA=1, fb=0.5, damp=0.2, g=0.5,
            gin=0.015, dry=1.0, wet1=1.0, wet2=0.0):
        return lib.tfx_freeverb_forward(x, y, dtype, batch, channels, T, tail, comb, NC, ap, NA, fb, damp, g, gin, dry, wet1, wet2,
                                        None, None, None, None)

    assert fwd() != 0 and b"null pointer" in lib.tfx_last_error()
    for kw in (dict(T=-1), dict(batch=-1), dict(tail=-1), dict(channels=3), dict(channels=0), dict(NC=0), dict(NC=9), dict(NA=5),
               dict(NA=-1), dict(comb=None), dict(ap=None), dict(dtype=7), dict(fb=1.0), dict(damp=1.0), dict(damp=-0.5), dict(g=1.0),
               dict(gin=float("inf")), dict(dry=float("nan")), dict(wet1=float("inf")), dict(wet2=float("nan"))):
        assert fwd(**kw) != 0, kw
        assert b"freeverb_forward" in lib.tfx_last_error(), kw
    bad = (ctypes.c_int64 * 2)(10, 0)
    assert fwd(comb=bad) != 0 and b"comb delays must be in [1, 65536]" in lib.tfx_last_error()
    # empty work is fine and touches nothing
    assert fwd(T=0) == 0 and fwd(batch=0) == 0
    assert lib.tfx_freeverb_plan_info(1, 1, 100, 0, comb, 2, ap, 1, 0.0, *ptrs) == 0
    assert [o.value for o in outs] == [10, 0, 10 + 11 + 2 + 3, 1, 0]
    assert lib.tfx_freeverb_plan_info(1, 1, 100, 0, comb, 2, ap, 1, 0.0, None, *ptrs[1:]) != 0
    assert b"null output" in lib.tfx_last_error()
    assert lib.tfx_freeverb_plan_info(1, 1, -5, 0, comb, 2, ap, 1, 0.0, *ptrs) != 0
    assert lib.tfx_freeverb_plan_info(1, 1, 100, 0, None, 2, ap, 1, 0.0, *ptrs) != 0


def test_the_ops_live_in_a_namespace_of_their_own():
    from torchfx_amd import native

    ops = native.reverb_ops()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_reverb::")}
    assert names == {"torchfx_reverb::freeverb_forward"}
    assert torch._C._dispatch_has_kernel_for_dispatch_key("torchfx_reverb::freeverb_forward", "CUDA")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.freeverb_forward(torch.zeros(2, 8), [5, 6], [], 0.5, 0.2, 0.5, 0.015, 1.0, 1.0, 0.0)
    y, st = ops.freeverb_forward(torch.empty(3, 2, 100, device="meta"), [5, 6, 7, 8], [3, 4], 0.5, 0.2, 0.5, 0.015, 1.0, 1.0, 0.5, 20)
    assert y.shape == (3, 2, 120) and st.shape == (6, 7 + 8 + 2 + 4) and st.dtype == torch.float64


def test_stream_processors_refuse_the_plain_effect():
    from torchfx_amd import Freeverb
    from torchfx_amd import realtime as RT

    class NoBackend(RT.AudioBackend):
        def open_stream(self, config, callback=None):
            raise AssertionError("the refusal comes before a stream is opened")

        def start(self):
            pass

        def stop(self):
            pass

        def close(self):
            pass

    with pytest.raises(TypeError, match="StatefulFreeverb"):
        RT.StreamProcessor([Freeverb()], chunk_size=512, device="cpu")
    with pytest.raises(TypeError, match="StatefulFreeverb"):
        RT.StreamProcessor([RT.StatefulFreeverb(), Freeverb(fs=FS)], chunk_size=512, device="cpu")
    with pytest.raises(TypeError, match="StatefulFreeverb"):
        RT.RealtimeProcessor([Freeverb()], NoBackend(), RT.StreamConfig(), device="cpu")
    RT.StreamProcessor([RT.StatefulFreeverb()], chunk_size=512, device="cpu")
    RT.RealtimeProcessor([RT.StatefulFreeverb()], NoBackend(), RT.StreamConfig(), device="cpu")


@pytest.mark.parametrize("chunk", [512, 100])
def test_stateful_freeverb_chunks_on_cpu(chunk):
    from torchfx_amd.realtime import StatefulFreeverb, StreamProcessor

    x, ref, _ = R.freeverb_case((2, 5000), FS, tail=300)
    t = torch.from_numpy(np.array(x)).double()
    fx = StatefulFreeverb(tail=300 / FS)
    sp = StreamProcessor([fx], chunk_size=chunk, device="cpu")
    y = sp.process_tensor(t, FS)
    assert y.shape == t.shape and fx.fs == FS
    R.check(y.numpy(), ref[:, :5000], f"StatefulFreeverb chunks of {chunk}")
    ring = fx.flush()
    assert ring.shape == (2, 300)
    R.check(ring.numpy(), ref[:, 5000:], "StatefulFreeverb ring-out")
    assert fx._hist is None and fx.flush().numel() == 0
    # reset_state: the next chunk starts from silence again
    a = fx(t[:, :700])
    fx.reset_state()
    assert torch.equal(fx(t[:, :700]), a)
    assert StatefulFreeverb(fs=FS).flush().numel() == 0


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2e-19, reason="np.longdouble is not wider than float64 here")
def test_e_ref_is_what_the_reference_measures():
    e, where = R.measure_e_ref()
    print(f"E_REF measured {e:.4e} at {where}; recorded {R.E_REF:.4e}")
    assert 0.5 * R.E_REF <= e <= R.E_REF
