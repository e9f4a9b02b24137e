"""Feedback (regeneration) of the modulated delay line on the device (csrc/modulation.hip, modulated_delay_feedback_kernel)
against the per-sample float64 loop of tests/modulation_feedback_reference.py within its derived bound -- blocks of 1 (64 rows
per wave), 5 (12 rows per wave, a remainder), 47 (idle lanes), 150 (sub-blocks, the last one short), two voices of opposite sign,
rings that wrap many times, lengths around a block -- and the exact cases with torch.equal: integer echoes across block and
sub-block seams, a row alone and inside batches that pack it differently, a NaN that stays in its row."""
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
    return dict(dry=F.DRY, spread=F.SPREAD, shape=lfo, interpolation=interpolation, position=F.POSITION, feedback=F.TABLES[name][1])


@pytest.mark.parametrize("name", list(F.TABLES))
@pytest.mark.parametrize("lfo", ["sine", "triangle"])
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_against_the_reference(dt, interpolation, lfo, name):
    y = run(F.case(name, interpolation, lfo)[0], F.voices(name, interpolation), dt, **kw_of(name, interpolation, lfo))
    assert y.dtype == dt
    F.check(y.numpy(), name, interpolation, lfo, f"device {name} {interpolation} {lfo} {dt}")


@pytest.mark.parametrize("n", [0, 1, 4, 5, 6])
def test_lengths_around_a_block(n):
    y = run(F.case("B5", "cubic", "sine")[0][..., :n], F.voices("B5", "cubic"), torch.float64, **kw_of("B5", "cubic", "sine"))
    F.check(y.numpy(), "B5", "cubic", "sine", f"device B5 T = {n}", length=n)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [1, 7, 64, 65])
def test_integer_echoes_are_exact(D, dt):
    """y is x delayed by D = B plus its echoes at 2 D, 3 D, .. with factors 1, 1/2, 1/4, ..: exact for 3-bit integers, <= 40 echoes."""
    n = max(40, 4 * D + 3)
    g = np.random.default_rng(D)
    x = (g.integers(-7, 8, (3, 2, n)) * (g.random((3, 2, n)) < 0.25)).astype(np.float64)
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


def test_a_nan_stays_in_its_row_and_behind_its_sample():
    x = np.array(F.case("B5", "linear", "sine")[0][..., :200])
    table, n0, D, kw = [(5.0, 0.0, 100.0, 0.0, 1.0)], 37, 5, dict(dry=F.DRY, spread=F.SPREAD, feedback=0.5, position=3)
    clean = run(x, table, **kw)
    x[1, 1, n0] = np.nan
    y = run(x, table, **kw)
    keep = torch.ones(5, 2, 200, dtype=torch.bool)
    keep[1, 1, n0:] = False
    assert torch.equal(y[keep], clean[keep]) and bool(torch.isfinite(clean).all()) and bool(torch.isnan(y[1, 1, [n0 + D, n0 + 2 * D]]).all())
