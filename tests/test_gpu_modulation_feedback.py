"""Feedback (regeneration) of the modulated delay line on the device (csrc/modulation.hip, modulated_delay_feedback_kernel)
against the per-sample float64 loop of tests/modulation_feedback_reference.py within its derived bound, every case after the plan
it was built for (modulated_delay_feedback_plan_info): blocks of 1 (64 rows per wave), 5 (12 rows per wave, a remainder), 16 (a
second packed wave, a last wave of one row), 32 (the last packed size) and 33 (the first unpacked one), 47 (idle lanes), 64 (one
full sub-block), 128 and 129 (two full sub-blocks and a third of one lane), 150 (the last sub-block short), packing cut by LDS
(B5long: 7 of 12 rows per wave), the rows_per_wave == 1 fallback with the full 64 KiB launch (B1long), two, three and eight
voices, rings that wrap many times, lengths around a block, inside a long block and around the pipeline depth -- and the exact
cases with torch.equal: integer echoes across block, sub-block and wave seams, a row alone and inside batches that pack it into
the first wave and into a later, partly filled one, a NaN and an Inf that stay in their row.  Flanger, Chorus and ModulatedDelay
with feedback run on the device against the same loop and name the kernel in explain()."""
import numpy as np
import pytest
import torch

from tests import modulation_feedback_reference as F
from tests.gpu_common import DEV

pytestmark = pytest.mark.gpu


def run(x, table, dtype=torch.float32, device=DEV, **kw):
    from torchfx_amd import modulated_delay

    return modulated_delay(torch.from_numpy(np.array(x)).to(device, dtype), F.FS, table, **kw).cpu()


def kw_of(name, interpolation, lfo):
    return dict(dry=F.DRY, spread=F.SPREAD, shape=lfo, interpolation=interpolation, position=F.POSITION, feedback=F.table(name)[1])


@pytest.mark.parametrize("name", list(F.TABLES))
@pytest.mark.parametrize("lfo", ["sine", "triangle"])
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_against_the_reference(dt, interpolation, lfo, name):
    """Every row of the case table (B16 .. V3 close the packing, seam and voice gaps named beside them in the reference)."""
    F.assert_plan(name, interpolation)
    y = run(F.case(name, interpolation, lfo)[0], F.voices(name, interpolation), dt, **kw_of(name, interpolation, lfo))
    assert y.dtype == dt
    F.check(y.numpy(), name, interpolation, lfo, f"device {name} {interpolation} {lfo} {dt}")


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_the_longest_ring_in_the_full_lds_launch(dt):
    """B1long: rows_per_wave == 1 with B <= 32 (the stride is the ring alone, one active lane), a ring of 8192 samples that wraps,
    the 64 KiB dynamic-LDS launch."""
    interpolation, lfo = F.LONG_PAIR
    F.assert_plan("B1long", interpolation)
    y = run(F.case("B1long", interpolation, lfo)[0], F.voices("B1long", interpolation), dt, **kw_of("B1long", interpolation, lfo))
    F.check(y.numpy(), "B1long", interpolation, lfo, f"device B1long {interpolation} {lfo} {dt}")


@pytest.mark.parametrize("n", [0, 1, 4, 5, 6])
def test_lengths_around_a_block(n):
    y = run(F.case("B5", "cubic", "sine")[0][..., :n], F.voices("B5", "cubic"), torch.float64, **kw_of("B5", "cubic", "sine"))
    F.check(y.numpy(), "B5", "cubic", "sine", f"device B5 T = {n}", length=n)


# B150: a row that ends inside a block of more than 64, in sub-block 0, at the seam of sub-blocks 0 / 1, one past it and one
# short of the block (9 * 150 + 10, + 64, + 65, + 149): the skip of the sub-blocks past the end, the pipeline draining mid-block.
# B129: rows shorter than the first block and its sub-blocks.  B16: around the block and around 4 B, the depth of the pipeline.
@pytest.mark.parametrize("name,n", [("B150", n) for n in (1360, 1414, 1415, 1499)] + [("B129", n) for n in (1, 63, 64, 65, 129, 130)]
                         + [("B16", n) for n in (0, 1, 15, 16, 17, 4 * 16 - 1, 4 * 16, 4 * 16 + 1)])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_row_that_ends_inside_a_block(dt, name, n):
    """The loop is causal: the prefix of the full case's reference is what the shorter call must give."""
    assert F.plan(name, "cubic", length=n)["block"] == F.table(name)[2]
    y = run(F.case(name, "cubic", "sine")[0][..., :n], F.voices(name, "cubic"), dt, **kw_of(name, "cubic", "sine"))
    F.check(y.numpy(), name, "cubic", "sine", f"device {name} T = {n} {dt}", length=n)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [1, 7, 64, 65, 16, 32, 33, 128, 129])
def test_integer_echoes_are_exact(D, dt):
    """y is x delayed by D = B plus its echoes at 2 D, 3 D, .. with factors 1, 1/2, 1/4, ..: exact for 3-bit integers, <= 40 echoes.
    Six batch items: D = 16 fills waves of 4 + 2 and D = 32 waves of 2 + 2 + 2."""
    n = max(40, 4 * D + 3)
    g = np.random.default_rng(D)
    x = (g.integers(-7, 8, (6, 2, n)) * (g.random((6, 2, n)) < 0.25)).astype(np.float64)
    want = np.zeros_like(x)
    for k in range(1, n // D + 1):
        want[..., k * D:] += 0.5 ** (k - 1) * x[..., :n - k * D]
    y = run(x, [(float(D), 0.0, 100.0, 0.3, 1.0)], dt, dry=0.0, feedback=0.5, position=7)
    assert torch.equal(y, torch.from_numpy(want).to(dt))


@pytest.mark.parametrize("name,interpolation", [("B1", "linear"), ("B5", "cubic"), ("two", "cubic"), ("B150", "linear")])
def test_a_row_does_not_see_its_batch_and_the_device_agrees_with_the_host(name, interpolation):
    x, table, kw = F.case(name, interpolation, "sine")[0], F.voices(name, interpolation), kw_of(name, interpolation, "sine")
    alone, pair, five = (run(x[a:b], table, **kw) for a, b in ((1, 2), (0, 2), (0, 5)))
    assert torch.equal(alone[0], pair[1]) and torch.equal(alone[0], five[1])          # rows 2 and 3 of [5, 2, T]
    host = run(x, table, torch.float64, "cpu", **kw)                # float64: two float32 roundings may differ by a whole ulp
    F.check(run(x, table, torch.float64, **kw).numpy(), name, interpolation, "sine", f"device against the host, {name}", ref=host.numpy())


@pytest.mark.parametrize("name,interpolation", [("B16", "cubic"), ("B32", "linear"), ("B5long", "cubic"), ("V8", "linear")])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_rows_bits_do_not_depend_on_its_wave(dt, name, interpolation):
    """Packed waves beyond the first: a row alone, as slot 1 of the first wave, as slot 0 of the second wave and as the last row of
    that partly filled wave has the same bits (the row index of a later packed wave, the stride between a wave's rings)."""
    rpw = F.assert_plan(name, interpolation)["rows_per_wave"]
    n = rpw + (rpw + 1) // 2                                           # a full wave and a partly filled one
    assert rpw > 1 and F.plan(name, interpolation, batch=n)["workgroups"] == 2 * 2
    x, table, kw = F.case(name, interpolation, "sine")[0], F.voices(name, interpolation), kw_of(name, interpolation, "sine")
    batch = np.array(x[np.arange(n) % x.shape[0]])
    at = sorted({1, rpw, n - 1})
    batch[at] = x[1]
    alone, whole = run(x[1:2], table, dt, **kw), run(batch, table, dt, **kw)
    for i in at:
        assert torch.equal(whole[i], alone[0]), f"row {i} of {n}, {rpw} rows per wave"
    for i in sorted(set(range(n)) - set(at)):                           # and its wave-mates are the case's rows
        F.check(whole[i:i + 1].numpy(), name, interpolation, "sine", f"device {name} {dt}: row {i} of {n}", rows=slice(i % x.shape[0], i % x.shape[0] + 1))
    if dt == torch.float64:
        host = run(x, table, torch.float64, "cpu", **kw)
        F.check(run(x, table, torch.float64, **kw).numpy(), name, interpolation, "sine", f"device against the host, {name}", ref=host.numpy())


def test_a_nan_stays_in_its_row_and_behind_its_sample():
    x = np.array(F.case("B5", "linear", "sine")[0][..., :200])
    table, n0, D, kw = [(5.0, 0.0, 100.0, 0.0, 1.0)], 37, 5, dict(dry=F.DRY, spread=F.SPREAD, feedback=0.5, position=3)
    clean = run(x, table, **kw)
    x[1, 1, n0] = np.nan
    y = run(x, table, **kw)
    keep = torch.ones(5, 2, 200, dtype=torch.bool)
    keep[1, 1, n0:] = False
    assert torch.equal(y[keep], clean[keep]) and bool(torch.isfinite(clean).all()) and bool(torch.isnan(y[1, 1, [n0 + D, n0 + 2 * D]]).all())


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_value_in_the_second_wave_leaves_its_wave_mates_alone(bad):
    """B = 16, four rows per wave, seven batch items: the value is planted in row 5, slot 1 of the second wave; rows 4 and 6
    share its wave and its LDS, rows 0 .. 3 are the first wave.  Everything but the planted row from its sample on keeps its bits."""
    c = F.case("B16", "linear", "sine")[0]
    x = np.array(c[np.arange(7) % 5][..., :200])
    table, n0, D, kw = [(16.0, 0.0, 100.0, 0.0, 1.0)], 37, 16, dict(dry=F.DRY, spread=F.SPREAD, feedback=0.5, position=3)
    from torchfx_amd import torchfx_ext as E

    q = E.modulated_delay_feedback_plan_info(200, [(16.0, 0.0, 100.0 / F.FS, 0.0, 1.0)], 0.5, batch=7, channels=2)
    assert (q["block"], q["rows_per_wave"], q["workgroups"]) == (16, 4, 2 * 2)
    clean = run(x, table, **kw)
    x[5, 1, n0] = bad
    y = run(x, table, **kw)
    keep = torch.ones(7, 2, 200, dtype=torch.bool)
    keep[5, 1, n0:] = False
    assert torch.equal(y[keep], clean[keep]) and bool(torch.isfinite(clean).all())
    assert not bool(torch.isfinite(y[5, 1, [n0, n0 + D, n0 + 2 * D]]).any())


def test_a_nan_in_sub_block_1_reaches_only_what_can_read_it():
    """B150 cubic: the NaN sits in sub-block 1 of block 3.  The earliest sample whose taps can reach w[n0] is n0 + B, B =
    floor(min(delay - depth)) - 1 for the cubic interpolant (its newest tap is w[n - i + 1], i >= B + 1), and by n0 + H, H =
    floor(delay + depth) + 2, every tap has passed it: the row keeps its bits in between and is NaN somewhere in that window."""
    name, ip = "B150", "cubic"
    B = F.assert_plan(name, ip)["block"]
    (delay, depth, *_), = F.voices(name, ip)
    assert B == int(np.floor(delay - depth)) - 1 == 150
    H, n0 = int(np.floor(delay + depth)) + 2, 3 * B + 64 + 10
    x = np.array(F.case(name, ip, "sine")[0])
    clean = run(x, F.voices(name, ip), **kw_of(name, ip, "sine"))
    x[2, 0, n0] = np.nan
    y = run(x, F.voices(name, ip), **kw_of(name, ip, "sine"))
    keep = torch.ones(y.shape, dtype=torch.bool)
    keep[2, 0, n0] = False
    keep[2, 0, n0 + B:] = False
    assert torch.equal(y[keep], clean[keep]) and bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(y[2, 0, n0])) and bool(torch.isnan(y[2, 0, n0 + B:n0 + H + 1]).any())


def effects():
    import torchfx_amd as f

    return {
        "Flanger": (f.Flanger(fs=48000, feedback=0.7), 1500,
                    "Flanger: native (modulated_delay_feedback_kernel, 1 voice(s), sine LFO, cubic interpolation, feedback 1.4: block 47, "
                    "1 row(s) per wave, ring 512, 2 workgroup(s) of 32 step(s); one launch)"),
        # the chorus' first echo comes back after 2 * 816 samples
        "Chorus": (f.Chorus(fs=48000, feedback=0.4), 3000,
                   "Chorus: native (modulated_delay_feedback_kernel, 3 voice(s), sine LFO, cubic interpolation, feedback 0.8: block 815, "
                   "1 row(s) per wave, ring 2048, 2 workgroup(s) of 4 step(s); one launch)"),
        "ModulatedDelay": (f.ModulatedDelay([(2e-3, 0.5e-3, 1.0, 0.0, 0.5), (5e-3, 1e-3, 0.7, 0.25, -0.3)], dry=0.8, spread=0.25,
                                            shape="triangle", fs=48000, feedback=0.9), 1500,
                           "ModulatedDelay: native (modulated_delay_feedback_kernel, 2 voice(s), triangle LFO, linear interpolation, "
                           "feedback 0.9: block 72, 1 row(s) per wave, ring 512, 2 workgroup(s) of 21 step(s); one launch)"),
    }


@pytest.mark.parametrize("which", ["Flanger", "Chorus", "ModulatedDelay"])
def test_the_effect_classes_on_the_device(which):
    """The classes reach the kernel: against the loop fed the table and the raw feedback that params() reports, within the same
    bound, and explain() names the kernel and its plan."""
    import torchfx_amd as f

    eff, n, line = effects()[which]
    x = np.random.default_rng(n).uniform(-1.0, 1.0, (2, n)).astype(np.float32)
    assert (f.Wave(torch.from_numpy(x).to(DEV), 48000, device=DEV) | eff).explain()[-1] == line
    P = eff.params(torch.float64)
    rows = [tuple(float(v) for v in r) for r in P.table]                # (base, depth, inc, phase, gain): inc is a rate at fs = 1
    y_ref, w_ref = F.feedback_ref(x[None], 1, rows, P.feedback, P.dry, P.spread, P.shape, P.interpolation)
    assert np.abs(y_ref - F.feedback_ref(x[None], 1, rows, 0.0, P.dry, P.spread, P.shape, P.interpolation)[0]).max() > 1e-3
    for dt in (torch.float32, torch.float64):
        assert np.array_equal(np.asarray(eff.params(dt).table), np.asarray(P.table))
        y = eff(torch.from_numpy(x).to(DEV, dt))
        assert y.dtype == dt and y.is_cuda
        F.check_bound(y.cpu().numpy(), y_ref[0], w_ref[0], 1, rows, P.dry, P.feedback, P.interpolation, f"device {which} {dt}")


def test_zz_report():
    for name, share in sorted(F.SHARES.items()):
        print(f"modulated delay feedback on the device, {name}: largest share of the bound {share:.3f}")
    assert all(s <= 1.0 for s in F.SHARES.values())
