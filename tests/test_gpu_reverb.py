"""Freeverb on the device (csrc/reverb.hip) against the per-sample loops of tests/reverb_reference.py within its measured
bound: Freeverb() on every shape at 44.1 and 48 kHz, freeverb_bank over the seams of the kernel (blocks of 1, 2 and 63 samples,
a comb per wave up to eight, delays shorter and longer than the signal, sub-blocks of the all-passes, T around the block size),
both launch counts, both placements of the delay lines, chunked calls and the state, and the exact cases of the definition
with torch.equal: echoes of an impulse, the dry path, batch independence, the tail, items next to a non-finite one."""
import numpy as np
import pytest
import torch

from tests import reverb_reference as R
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 44100
DTYPES = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}


def on_device(x, dtype=None):
    t = torch.from_numpy(np.array(x))
    return t.to(DEV, dtype or t.dtype)


def bank(x, comb, allpass, dtype=None, **kw):
    from torchfx_amd import freeverb_bank

    return freeverb_bank(on_device(x, dtype), comb, allpass, **kw)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape,fs", R.FREEVERB_CASES)
def test_freeverb_matches_the_reference(shape, fs, dt):
    from torchfx_amd import Freeverb

    x, ref, _ = R.freeverb_case(shape, fs)
    tdt, ndt = DTYPES[dt]
    t = on_device(x, tdt)
    fx = Freeverb(fs=fs)
    y = fx(t)
    assert y.dtype == tdt and y.shape == t.shape and y.device.type == "cuda"
    assert np.abs(ref - x).max() > 0.05                                    # the wet part is at work
    R.check(y.cpu().numpy(), ref, f"Freeverb {shape} {fs} {dt}", ndt)
    route = fx.route(t)
    assert route.startswith("native (freeverb_kernel") and "blocks of 1024 samples" in route and "LDS" in route and "one launch" in route


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("case", R.BANK_GRID, ids=R.bank_id)
def test_bank_matches_the_reference_over_the_seams(case, dt):
    x, comb, allpass, kw, ref, ref_state = R.bank_case(case)
    tdt, ndt = DTYPES[dt]
    C = case[5]
    q = ext().freeverb_plan_info(case[4], comb, allpass, channels=C, wet2=kw["wet2"])
    assert q["block"] == min(min(min(r) for r in comb), 1024) and q["launches"] == C and q["placement"] == "lds"
    y, st = bank(x, comb, allpass, tdt, return_state=True, **kw)
    assert y.dtype == tdt and tuple(y.shape) == x.shape and st.dtype == torch.float64 and tuple(st.shape) == ref_state.shape
    R.check(y.cpu().numpy(), ref, f"bank {R.bank_id(case)} {dt}", ndt)
    R.check(st.cpu().numpy(), ref_state, f"bank state {R.bank_id(case)} {dt}")


def impulse(shape, dtype):
    x = torch.zeros(shape, dtype=dtype, device=DEV)
    x[..., 0] = 1.0
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
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
    y = freeverb_bank(x, [[37], [37]], (), 0.5, 0.0, input_gain=1.0, dry_gain=0.0, wet1=1.0).cpu()
    assert torch.equal(y[0], want) and torch.equal(y[1], want)
    assert torch.equal(freeverb_bank(impulse((T,), dtype), (37,), (), 0.5, 0.0, input_gain=0.5, dry_gain=0.0).cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_exact_allpass_echoes(dtype):
    """A one-sample comb (D = 1, fb = 0) into one all-pass with D = 5, g = 0.5: r[1] = -1, r[1 + 5k] = 0.5^(k-1), zero elsewhere."""
    from torchfx_amd import freeverb_bank

    T = 200
    want = torch.zeros(T, dtype=dtype)
    want[1] = -1.0
    for k in range(1, (T - 2) // 5 + 1):
        want[1 + 5 * k] = 0.5 ** (k - 1)
    y = freeverb_bank(impulse((T,), dtype), (1,), (5,), 0.0, 0.0, 0.5, input_gain=0.5, dry_gain=0.0)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("shape", [(3000,), (2, 3000), (2, 2, 3000)])
def test_dry_only_returns_the_input_bit_for_bit(shape):
    from torchfx_amd import Freeverb

    for tdt in (torch.float32, torch.float64):
        x = on_device(R.signal(shape, 5), tdt)
        assert torch.equal(Freeverb(wet=0.0, dry=0.5, fs=FS)(x), x)


@pytest.mark.parametrize("width", [1.0, 0.5])
def test_each_item_of_a_batch_equals_its_result_alone(width):
    from torchfx_amd import freeverb

    x = on_device(R.signal((5, 2, 2500), 6))
    y = freeverb(x, FS, width=width)
    assert not torch.equal(y[0], y[1])
    for i in range(5):
        assert torch.equal(y[i], freeverb(x[i].contiguous(), FS, width=width))
    assert torch.equal(y[1:3], freeverb(x[1:3].contiguous(), FS, width=width))


@pytest.mark.parametrize("width", [1.0, 0.3])
def test_tail_equals_the_zero_padded_call(width):
    from torchfx_amd import freeverb_bank
    from torchfx_amd.reverb import FreeverbParams

    P = FreeverbParams(FS, width=width).bank(2)
    x = on_device(R.signal((2, 2, 3000), 7))
    args = (P.comb, P.allpass, P.fb, P.d1, P.g, P.input_gain, P.dry, P.wet1, P.wet2)
    y, st = freeverb_bank(x, *args, tail_samples=300, return_state=True)
    z, sz = freeverb_bank(torch.nn.functional.pad(x, (0, 300)), *args, return_state=True)
    assert y.shape == (2, 2, 3300) and torch.equal(y, z) and torch.equal(st, sz)
    assert float(y[..., 3000:].abs().max()) > 1e-3                          # the room rings on


def test_width_one_and_narrower_are_both_within_the_bound_and_differ_in_launches():
    from torchfx_amd import Freeverb, freeverb

    comb, allpass = R.tunings(FS, 2)
    one = ext().freeverb_plan_info(5000, comb, allpass, channels=2, wet2=0.0)
    two = ext().freeverb_plan_info(5000, comb, allpass, channels=2, wet2=R.freeverb_constants(width=0.3)[6])
    assert one["launches"] == 1 and one["workspace_bytes"] == 0
    assert two["launches"] == 2 and two["workspace_bytes"] == 2 * 5000 * 8
    for width in (1.0, 0.3):
        x, ref, _ = R.freeverb_case((2, 5000), FS, width=width)
        for dt, (tdt, ndt) in DTYPES.items():
            R.check(freeverb(on_device(x, tdt), FS, width=width).cpu().numpy(), ref, f"width {width} {dt}", ndt)
    assert "two launches" in Freeverb(width=0.3, fs=FS).route(on_device(R.signal((2, 100), 1)))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_lines_in_the_global_workspace(dt):
    """Eight combs of about 2500 samples and T = 6000: 160 KB of lines do not fit the LDS, the rings live in the workspace.
    Two channels with a cross-feed, so the workspace holds the lines and the wet signal; and a 96 kHz Freeverb()."""
    from torchfx_amd import Freeverb

    tdt, ndt = DTYPES[dt]
    comb = [[2500 + 7 * k + 3 * c for k in range(8)] for c in range(2)]
    allpass = [[556 + c, 441 + c] for c in range(2)]
    q = ext().freeverb_plan_info(6000, comb, allpass, channels=2, wet2=0.25)
    assert q["placement"] == "global" and q["block"] == 1024 and q["launches"] == 2
    assert q["workspace_bytes"] == 2 * (sum(comb[1]) + sum(allpass[1])) * 8 + 2 * 6000 * 8
    x = R.signal((2, 6000), 11)
    kw = dict(fb=0.84, d1=0.2, g=0.5, input_gain=0.1, dry=0.75, wet1=0.5, wet2=0.25)
    ref, ref_state = R.freeverb_ref(x, comb, allpass, **kw)
    y, st = bank(x, comb, allpass, tdt, feedback=0.84, damp=0.2, input_gain=0.1, dry_gain=0.75, wet1=0.5, wet2=0.25, return_state=True)
    R.check(y.cpu().numpy(), ref, f"global lines {dt}", ndt)
    R.check(st.cpu().numpy(), ref_state, f"global lines state {dt}")
    # the same bank with the lines in LDS: fewer combs
    assert ext().freeverb_plan_info(6000, [r[:4] for r in comb], allpass, channels=2)["placement"] == "lds"
    if dt == "f64":
        x96 = R.signal((2, 3000), 12)
        c96, a96 = R.tunings(96000, 2)
        fb, d1, g, gin, dry, wet1, wet2 = R.freeverb_constants()
        ref96, _ = R.freeverb_ref(x96, c96, a96, fb, d1, g, gin, dry, wet1, wet2)
        fx = Freeverb(fs=96000)
        assert "global workspace" in fx.route(on_device(x96))
        R.check(fx(on_device(x96, tdt)).cpu().numpy(), ref96, "Freeverb at 96 kHz", ndt)


CHUNK_CASE = ("wave", "four", 0.9, 0.98, 4097, 2)


@pytest.mark.parametrize("chunk", [1, 7, 64, 1000, 62, 63, 65, 66])
def test_chunked_calls_and_the_state_match_the_one_shot_reference(chunk):
    """Chunks of 1, 7, 64, 1000 and D - 1, D, D + 1 around the comb delays 63 .. 65 (the second channel's 65 .. 67), with a
    remainder, against the one-shot reference: outputs and the final state (the reference's lines in time order)."""
    from torchfx_amd import freeverb_bank

    x, comb, allpass, kw, ref, ref_state = R.bank_case(CHUNK_CASE)
    T = 600 if chunk < 64 else 4097
    if T != 4097:
        ref, ref_state = R.freeverb_ref(x[..., :T], comb, allpass, **R._ref_kw(kw))
    t = on_device(x[..., :T], torch.float64)
    st, out = None, []
    for n0 in range(0, T, chunk):
        y, st = freeverb_bank(t[..., n0:n0 + chunk], comb, allpass, state=st, return_state=True, **kw)
        assert y.shape[-1] == min(chunk, T - n0)
        out.append(y)
    R.check(torch.cat(out, -1).cpu().numpy(), ref, f"chunks of {chunk}")
    R.check(st.cpu().numpy(), ref_state, f"state after chunks of {chunk}")
    empty, same = freeverb_bank(t[..., :0], comb, allpass, state=st, return_state=True, **kw)        # an empty chunk moves nothing
    assert empty.shape == (2, 0) and torch.equal(same, st)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("width", [1.0, 0.3])
def test_a_non_finite_sample_stays_in_its_item_and_behind_itself(bad, width):
    from torchfx_amd import freeverb

    n0 = 2500
    x = np.array(R.signal((3, 2, 5000), 13))
    planted = x.copy()
    planted[1, 0, n0] = bad
    zeroed = x[1].copy()
    zeroed[:, n0:] = 0.0
    comb, allpass = R.tunings(FS, 2)
    fb, d1, g, gin, dry, wet1, wet2 = R.freeverb_constants(width=width)
    ref, _ = R.freeverb_ref(zeroed, comb, allpass, fb, d1, g, gin, dry, wet1, wet2)
    for dt, (tdt, ndt) in DTYPES.items():
        y = freeverb(on_device(planted, tdt), FS, width=width)
        for i in (0, 2):
            assert torch.equal(y[i], freeverb(on_device(x[i], tdt), FS, width=width)), (dt, i)
        R.check(y[1, :, :n0].cpu().numpy(), ref[:, :n0], f"before the {bad} {dt} width {width}", ndt)
        assert not torch.isfinite(y[1, 0, n0])


def test_freeverb_in_a_wave_pipeline_is_a_step_of_its_own_and_names_its_route():
    from torchfx_amd import Freeverb, Gain, Wave, freeverb

    x = on_device(R.signal((2, 3000), 8))
    w = Wave(x, 48000, device=DEV) | Gain(0.5) | Freeverb(room_size=0.7, width=0.5, tail=0.01) | Gain(2.0)
    assert [type(m).__name__ for m in w.plan()] == ["Gain", "Freeverb", "Gain"]
    line = w.explain()[1]
    assert line.startswith("Freeverb: native (freeverb_kernel") and "blocks of 1024 samples" in line and "LDS" in line
    assert "two launches" in line
    want = ext().gain_forward(freeverb(ext().gain_forward(x, 0.5, False), 48000, room_size=0.7, width=0.5, tail=0.01), 2.0, False)
    assert w.ys.shape == (2, 3480) and torch.equal(w.ys, want)
