"""The modulated delay line on the device (csrc/modulation.hip) against the per-sample float64 loop of
tests/modulation_reference.py within its derived bound -- every length class of the tiling, row counts 1, 2, 3 and a batch
that splits, 1 / 3 / 8 voices, both LFO shapes, both interpolants, delays shorter than a lane's span, longer than a tile and
longer than the signal, position 2^40 -- and the exact cases of the definition with torch.equal: integer delays, silent voices,
batch independence, prefixes, the non-finite window.  Signals hold float32-representable values so that one reference serves
both dtypes."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import modulation_reference as R
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 48000
TILE = 1024
DTYPES = {"f32": torch.float32, "f64": torch.float64}
# (delay, depth, rate, phase, gain) with delay and depth in samples, every depth <= 512
SHORT = (1.5, 0.4, 3.0, 0.0, 0.5)                   # smaller than a lane's span
ACROSS = (1500.5, 400.25, 0.7, 0.3, -0.4)            # larger than a tile: reads cross tiles
BEYOND = (5000.0, 512.0, 1.1, 0.6, 0.3)              # larger than every T here: that voice's wet part is all zeros
VOICES = {
    1: [SHORT],
    3: [SHORT, ACROSS, BEYOND],
    8: [SHORT, ACROSS, BEYOND, (37.0, 36.0, 5.0, 0.11, 0.2), (700.75, 512.0, 0.25, 0.9, 0.15), (2.0, 1.0, 11.0, 0.5, -0.3),
        (1024.0, 0.0, 1.0, 0.0, 0.1), (260.5, 3.25, 2.0, 0.77, 0.25)],
}
DRY = 0.7
WORST = {}


def signal(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, seed, V, lfo, interpolation, position=0, spread=0.25):
    """(x float32 array, unrounded float64 reference), computed once per case and shared."""
    x = signal(shape, seed)
    x.setflags(write=False)
    ref = R.modulated_delay_ref(x, FS, VOICES[V], dry=DRY, spread=spread, shape=lfo, interpolation=interpolation, position=position)
    ref.setflags(write=False)
    return x, ref


def run(x, voices, dtype=None, **kw):
    from torchfx_amd import modulated_delay

    t = torch.from_numpy(np.array(x))
    return modulated_delay(t.to(DEV, dtype or t.dtype), FS, voices, **kw)


def parity(what, shape, seed, V, lfo, interpolation, dt, position=0):
    x, ref = case(shape, seed, V, lfo, interpolation, position)
    R.at_work(ref, x, FS, VOICES[V], DRY, what)
    y = run(x, VOICES[V], DTYPES[dt], dry=DRY, spread=0.25, shape=lfo, interpolation=interpolation, position=position)
    assert y.dtype == DTYPES[dt] and y.shape == x.shape and y.device.type == "cuda"
    worst, excess = R.check(y.cpu().numpy(), ref, x, FS, VOICES[V], DRY, what=f"{what} {dt}")
    k = (dt, interpolation)
    seen = WORST.get(k, (0.0, -math.inf))
    WORST[k] = (max(seen[0], worst), max(seen[1], excess))


def test_plan_info_gives_the_tile_the_tests_assume():
    q = ext().modulated_delay_plan_info(3 * TILE + 17, [(b, d, r / FS, p, g) for b, d, r, p, g in VOICES[3]], batch=5, channels=2)
    assert q == dict(tile=TILE, tiles=4, history=5514, batch_items=4, batch_groups=2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_lengths_against_the_definition(T, dt):
    parity(f"T={T}", (2, T), T, 3, "sine", "cubic", dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("V", [1, 3, 8])
@pytest.mark.parametrize("shape", [(TILE + 1,), (2, TILE + 1), (3, TILE + 1), (5, 2, TILE + 1)], ids=["T", "2T", "3T", "52T"])
def test_shapes_and_voice_counts_against_the_definition(shape, V, dt):
    lfo, interpolation = [("sine", "linear"), ("triangle", "cubic"), ("sine", "cubic"), ("triangle", "linear")][(len(shape) + V) % 4]
    parity(f"{shape} V={V} {lfo} {interpolation}", shape, 100 + V, V, lfo, interpolation, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
@pytest.mark.parametrize("lfo", ["sine", "triangle"])
def test_shapes_of_the_lfo_and_interpolants(lfo, interpolation, dt):
    parity(f"{lfo} {interpolation}", (2, 2 * TILE + 5), 7, 8, lfo, interpolation, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
def test_position_2_to_the_40(interpolation, dt):
    parity(f"position 2^40 {interpolation}", (2, TILE + 1), 9, 3, "sine", interpolation, dt, position=2 ** 40)
    x, ref = case((2, TILE + 1), 9, 3, "sine", interpolation, 2 ** 40)
    assert np.abs(ref - case((2, TILE + 1), 9, 3, "sine", interpolation, 0)[1]).max() > 1e-3       # the position moved the LFO


def test_spread_makes_the_channels_differ():
    one = signal((1, TILE + 1), 11)
    x = np.concatenate([one, one])
    y = run(x, VOICES[3], dry=DRY, spread=0.25, interpolation="cubic")
    y0 = run(x, VOICES[3], dry=DRY, spread=0.0, interpolation="cubic")
    assert torch.equal(y0[0], y0[1]) and torch.equal(y[0], y0[0]) and not torch.equal(y[0], y[1])


# ---- the exact cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("interpolation,lfo", [("linear", "sine"), ("cubic", "triangle")])
def test_integer_delay_is_an_exact_copy(interpolation, lfo, dt):
    T = 2 * TILE + 5
    x = torch.from_numpy(signal((3, T), 12)).to(DEV, DTYPES[dt])
    for D in (1, 37, TILE - 1, TILE + 3, T - 1, T, T + 100):
        y = run(x.cpu().numpy(), [(float(D), 0.0, 2.0, 0.3, 1.0)], dry=0.0, interpolation=interpolation, shape=lfo, position=3)
        want = torch.zeros_like(x)
        want[:, D:] = x[:, :max(0, T - D)]
        assert torch.equal(y, want), D


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
def test_silent_voices_return_the_input(interpolation, dt):
    x = torch.from_numpy(signal((5, 2, TILE + 1), 13)).to(DEV, DTYPES[dt])
    silent = [(b, d, r, p, 0.0) for b, d, r, p, _ in VOICES[8]]
    assert torch.equal(run(x.cpu().numpy(), silent, dry=1.0, spread=0.3, interpolation=interpolation), x)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_rows_bits_depend_on_neither_the_batch_nor_the_length(dt):
    T = 3 * TILE + 17
    items = signal((5, 2, T), 14)
    items[4] = items[1]                                                 # equal batch items, in different batch groups
    kw = dict(dry=DRY, spread=0.25, interpolation="cubic")
    y = run(items, VOICES[3], DTYPES[dt], **kw)
    assert torch.equal(y[4], y[1]) and not torch.equal(y[0], y[1])
    for b in (0, 3, 4):                                                 # a batch item run alone, as [C, T] and as [1, C, T]
        assert torch.equal(run(items[b], VOICES[3], DTYPES[dt], **kw), y[b]), b
        assert torch.equal(run(items[b:b + 1], VOICES[3], DTYPES[dt], **kw)[0], y[b]), b
    for n in (1, TILE - 1, TILE, 2 * TILE + 1):                         # the effect is causal: a prefix is the prefix's result
        assert torch.equal(run(items[..., :n], VOICES[3], DTYPES[dt], **kw), y[..., :n]), n


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
def test_a_non_finite_sample_stays_in_its_window(interpolation, dt, bad):
    T = 2 * TILE + 5
    voices = [SHORT, (700.75, 512.0, 0.25, 0.9, 0.15)]
    reach = math.floor(700.75 + 512.0) + 2
    x = signal((3, T), 15)
    kw = dict(dry=DRY, spread=0.1, interpolation=interpolation)
    clean = run(x, voices, DTYPES[dt], **kw)
    for m in (0, TILE - 1, TILE, T - 1):
        xb = x.copy()
        xb[1, m] = bad
        y = run(xb, voices, DTYPES[dt], **kw)
        keep = torch.ones(T, dtype=torch.bool, device=DEV)
        keep[m:m + reach + 1] = False
        assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2]), m
        assert torch.equal(y[1, keep], clean[1, keep]), m
        assert not torch.isfinite(y[1, m]), m


# ---- the effects and the boundary -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["Chorus", "Flanger", "Vibrato"])
def test_effects_at_their_defaults_against_the_definition(name):
    import torchfx_amd as fx

    eff = getattr(fx, name)()
    x = signal((2, 2 * TILE + 5), 16)
    y = (fx.Wave(torch.from_numpy(x), FS, device=DEV) | eff).ys
    P = eff.params(torch.float32)
    voices = eff.voice_table(FS)
    ref = R.modulated_delay_ref(x, FS, voices, dry=P.dry, spread=P.spread, shape=P.shape, interpolation=P.interpolation)
    R.at_work(ref, x, FS, voices, P.dry, name)
    R.check(y.cpu().numpy(), ref, x, FS, voices, P.dry, what=name)


def test_explain_and_route_name_the_native_kernel():
    from torchfx_amd import Chorus, Wave

    x = torch.zeros(5, 2, 3 * TILE + 17)
    lines = (Wave(x, FS, device=DEV) | Chorus()).explain()
    assert lines == [f"Chorus: native (modulated_delay_kernel, 3 voice(s), sine LFO, cubic interpolation, 4 tile(s) of {TILE} per row, "
                     "2 batch group(s) of up to 4; one launch)"]


def test_cpu_tensor_is_refused_by_the_op_and_served_by_the_function():
    from torchfx_amd import modulated_delay

    x = torch.from_numpy(signal((2, 300), 17))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext().modulated_delay_forward(x, [(b, d, r / FS, p, g) for b, d, r, p, g in VOICES[1]])
    assert modulated_delay(x.to(DEV), FS, VOICES[1]).device.type == "cuda" and modulated_delay(x, FS, VOICES[1]).device.type == "cpu"


def test_zz_report_largest_deviations():
    """Not a check of its own: prints what the parity tests above saw, per dtype and interpolant."""
    for (dt, interpolation), (worst, excess) in sorted(WORST.items()):
        print(f"{dt} {interpolation}: largest deviation from the definition {worst:.3e}, largest excess over the bound {excess:.3e}")
    assert all(excess <= 0.0 for _, excess in WORST.values())
