"""The compressor on the device (csrc/compressor.hip through torchfx_ext.compressor_forward) against the per-sample float64
definition (tests/compressor_reference.py).  Shapes come from compressor_plan_info (tile and segment seams), never from the
workload.  The bounds (float64 detector for both signal dtypes):
  float64   |20 log10 g - 20 log10 g_ref| <= 1e-10 dB   and   |y - y_ref| <= 1e-11 max|y_ref|
  float32   |y - y_ref| <= 2^-23 |y_ref| + 1e-11 max|y_ref|   (y_ref in float64 from the float32 input: one rounding of the product)
            the returned gain is g rounded once: |g - g_ref| <= (2^-24 + 2e-11) g_ref   (1e-10 dB is 1.2e-11 relative)
  state     1e-10 (it is in dB)
The same bounds hold between different `segments` and between chunked and one-shot runs."""
import math

import numpy as np
import pytest
import torch

from tests import compressor_reference as R
from tests.gpu_common import DEV, dev, ext

pytestmark = pytest.mark.gpu

FS = 48000
TILE = 2048
T_SEAMS = 3 * TILE + 17
DTYPES = {"f32": np.float32, "f64": np.float64}
CORNERS = {
    "defaults": {},
    "attack0": {"attack": 0.0},
    "release0": {"release": 0.0},
    "ratio_inf": {"ratio": math.inf},
    "hard_knee": {"knee_db": 0.0},
    "makeup": {"makeup_db": 4.5},
}
_REF: dict = {}
WORST: dict = {}


def reduced(kw):
    from torchfx_amd.dynamics import CompressorParams

    P = CompressorParams(FS, torch.float32, **kw)
    return P.th, P.s, P.w, P.alpha_a, P.alpha_r, P.makeup


def run(x, kw=None, channels=1, state=None, segments=0, gain=True):
    """The low-level op on a device copy of ``x`` -> NumPy ``(y, g, state)``."""
    st = None if state is None else dev(np.asarray(state, dtype=np.float64))
    y, g, s = ext().compressor_forward(dev(x), *reduced(kw or {}), channels, st, gain, segments)
    return y.cpu().numpy(), (g.cpu().numpy() if gain else None), s.cpu().numpy()


def signal(seed, groups, channels, T, dtype):
    """Bursty noise: the loud bursts end 5 samples before every tile seam (the release tail is the seam's carry), and a stretch
    of exact zeros lies across the first seam."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((groups, channels, T)) * 0.01
    for k in range(1, T // TILE + 1):
        lo, hi = max(0, k * TILE - 300), k * TILE - 5
        x[..., lo:hi] *= 60.0 * (1.0 + 0.1 * k)
    if T > TILE + 50:
        x[..., TILE - 2:TILE + 50] = 0.0
    if T < TILE:
        x[..., T // 3:] *= 50.0
    return np.clip(x, -2.0, 2.0).astype(dtype)


def reference(name, x, channels, kw=None, state=None):
    """``compress_ref`` on ``x [groups, channels, T]``, computed once per ``name``."""
    if name not in _REF:
        _REF[name] = R.compress_ref(x.reshape(-1, channels, x.shape[-1]), FS, link=True, state=state, **(kw or {}))
    return _REF[name]


def check(what, got, ref, dtype):
    """The module's bounds for ``got = (y, g, state)`` against ``ref``; the largest deviations go to WORST (printed at the end)."""
    (y, g, st), (yr, gr, sr) = got, ref
    yr = yr.reshape(y.shape)
    top = np.abs(yr).max() if yr.size else 0.0
    if dtype == np.float64:
        dy = np.abs(y - yr).max() / max(top, 1e-300)
        dg = np.abs(20 * np.log10(g) - 20 * np.log10(gr)).max()
        ok = dy <= 1e-11 and dg <= 1e-10
    else:
        err = np.abs(y.astype(np.float64) - yr)
        dy = (err - 2.0 ** -23 * np.abs(yr)).max() / max(top, 1e-300)
        dg = (np.abs(g.astype(np.float64) - gr) / gr).max()
        ok = dy <= 1e-11 and dg <= 2.0 ** -24 + 2e-11
    ds = np.abs(st - sr).max()
    key = np.dtype(dtype).name
    w = WORST.setdefault(key, [-np.inf, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], dy), max(w[1], dg), max(w[2], ds)
    print(f"{what} [{key}]: dy {dy:.3e}  dg {dg:.3e}  dstate {ds:.3e}")
    assert ok and ds <= 1e-10, (what, dy, dg, ds)


def between(what, a, b, dtype):
    """The same bounds between two device results (two float32 outputs are two roundings of products 1e-11 apart: one ulp)."""
    (ya, ga, sa), (yb, gb, sb) = a, b
    ya, yb, ga, gb = (v.astype(np.float64) for v in (ya, yb, ga, gb))
    dy = (np.abs(ya - yb) - (2.0 ** -23 * np.abs(yb) if dtype == np.float32 else 0.0)).max() / np.abs(yb).max()
    dg = np.abs(20 * np.log10(ga) - 20 * np.log10(gb)).max() if dtype == np.float64 else (np.abs(ga - gb) / gb).max()
    ds = np.abs(sa - sb).max()
    print(f"{what}: dy {dy:.3e}  dg {dg:.3e}  dstate {ds:.3e}")
    assert dy <= 1e-11 and dg <= (1e-10 if dtype == np.float64 else 2.0 ** -23 + 2e-11) and ds <= 1e-10, (what, dy, dg, ds)


def test_plan_info_gives_the_tile_the_tests_assume():
    info = ext().compressor_plan_info(T_SEAMS, 1, 2)
    assert info["tile"] == TILE and info["tiles"] == 4
    assert ext().compressor_plan_info(T_SEAMS, 1, 2, 3)["segments"] == 3
    assert ext().compressor_plan_info(T_SEAMS, 1, 2, 9)["segments"] == 4           # clamped to the tile count
    assert ext().compressor_plan_info(T_SEAMS, 1, 2, 1)["scratch_bytes"] == 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, T_SEAMS])
def test_lengths_against_the_definition(T, dt):
    x = signal(T, 1, 2, T, DTYPES[dt])
    check(f"T={T}", run(x, channels=2), reference(("len", T, dt), x, 2), DTYPES[dt])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("link", [True, False])
@pytest.mark.parametrize("gc", [(1, 1), (1, 2), (3, 2)])
def test_every_segment_count_against_the_definition_and_each_other(gc, link, dt):
    groups, channels = gc
    x = signal(11 * groups + channels, groups, channels, T_SEAMS, DTYPES[dt])
    ch = channels if link else 1
    ref = reference(("seg", gc, link, dt), x, ch)
    outs = {}
    for segments in (0, 1, 2, 3, 9):
        outs[segments] = run(x, channels=ch, segments=segments)
        check(f"{gc} link={link} segments={segments}", outs[segments], ref, DTYPES[dt])
    for segments in (0, 2, 3, 9):
        between(f"{gc} link={link} segments={segments} vs 1", outs[segments], outs[1], DTYPES[dt])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("corner", CORNERS)
def test_parameter_corners(corner, dt):
    x = signal(5, 1, 2, T_SEAMS, DTYPES[dt])
    ref = reference(("corner", corner, dt), x, 2, CORNERS[corner])
    for segments in (1, 3):
        check(f"{corner} segments={segments}", run(x, CORNERS[corner], 2, segments=segments), ref, DTYPES[dt])


@pytest.mark.parametrize("dt", DTYPES)
def test_transparent_bit_for_bit_at_every_segment_count(dt):
    rng = np.random.default_rng(3)
    x = (rng.uniform(-1, 1, (2, 2, T_SEAMS)) * 10 ** (-23.5 / 20)).astype(DTYPES[dt])     # under Th - W/2 = -23 dB
    x[0, 0, 100] = -0.0
    for segments in (0, 1, 2, 3, 9):
        y, g, st = run(x, channels=2, segments=segments)
        assert np.array_equal(y.view(np.uint8), x.view(np.uint8)), segments
        assert np.all(g == 1.0) and np.all(st == 0.0)


def test_carried_state_across_two_calls_and_determinism():
    x = signal(9, 2, 2, T_SEAMS, np.float64)
    ref = reference(("state", 0), x, 2)
    cut = TILE + 333
    ya, ga, sa = run(x[..., :cut], channels=2, segments=2)
    yb, gb, sb = run(x[..., cut:], channels=2, state=sa, segments=2)
    check("two calls", (np.concatenate([ya, yb], -1), np.concatenate([ga, gb], -1), sb), ref, np.float64)
    again = run(x[..., cut:], channels=2, state=sa, segments=2)
    assert all(np.array_equal(a, b) for a, b in zip((yb, gb, sb), again))          # two identical calls: bit-equal
    st0 = np.array([[3.0, 1.0], [0.5, 2.5]])
    check("given state", run(x, channels=2, state=st0, segments=3), reference(("state", 1), x, 2, state=st0), np.float64)


def test_without_gain_the_second_output_is_none_and_y_is_the_same():
    x = signal(2, 1, 2, TILE + 1, np.float32)
    y, g, st = run(x, channels=2, gain=False)
    y2, g2, st2 = run(x, channels=2, gain=True)
    assert g is None and g2.shape == (1, TILE + 1) and np.array_equal(y, y2) and np.array_equal(st, st2)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_groups_bits_do_not_depend_on_the_other_groups(dt):
    x = signal(21, 3, 2, T_SEAMS, DTYPES[dt])
    y, g, st = run(x, channels=2, segments=3)
    for k in range(3):
        yk, gk, sk = run(x[k:k + 1], channels=2, segments=3)
        assert np.array_equal(y[k:k + 1], yk) and np.array_equal(g[k:k + 1], gk) and np.array_equal(st[k:k + 1], sk)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dt", DTYPES)
def test_non_finite_from_its_sample_to_the_end_of_its_group(dt, bad):
    x = signal(31, 3, 2, T_SEAMS, DTYPES[dt])
    clean = run(x, channels=2, segments=3)
    n0 = 2 * TILE + 777                              # segments = 3 over 4 tiles: the second segment is tile 2; mid-tile
    xb = x.copy()
    xb[1, 1, n0] = bad
    y, g, st = run(xb, channels=2, segments=3)
    for k in (0, 2):
        assert np.array_equal(y[k], clean[0][k]) and np.array_equal(g[k], clean[1][k]) and np.array_equal(st[k], clean[2][k])
    assert np.array_equal(y[1][:, :n0], clean[0][1][:, :n0]) and np.array_equal(g[1][:n0], clean[1][1][:n0])
    assert np.isnan(y[1][:, n0:]).all() and np.isnan(g[1][n0:]).all() and np.isnan(st[1]).all()


def test_public_function_on_the_device_matches_the_definition():
    import torchfx_amd as fx

    x = signal(41, 3, 2, T_SEAMS, np.float32)
    for link in (True, False):
        y, g, st = fx.compress(dev(x), FS, -18.0, 3.0, link=link, return_gain=True, return_state=True)
        ref = R.compress_ref(x, FS, -18.0, 3.0, link=link)
        check(f"compress link={link}", (y.cpu().numpy(), g.cpu().numpy(), st.cpu().numpy()), ref, np.float32)
    w = fx.Wave(torch.from_numpy(x[0]), FS, device=DEV) | fx.LoudnessNormalize(-14) | fx.Compressor(-18, 3) | fx.Limiter(-1)
    assert any(line.startswith("Compressor: native (compressor_kernel") for line in w.explain())
    assert w.ys.shape == (2, T_SEAMS) and bool(torch.isfinite(w.ys).all())


def test_launch_count_is_one_for_one_segment_and_three_otherwise():
    from torchfx_amd import _lib

    lib = _lib.load()
    x = dev(signal(1, 1, 2, T_SEAMS, np.float32))
    import json

    for segments, names in ((1, ["compressor_pass_c"]), (3, ["compressor_pass_a", "compressor_pass_b", "compressor_pass_c"])):
        lib.tfx_prof_enable(1)
        try:
            ext().compressor_forward(x, *reduced({}), 2, None, False, segments)
            prof = json.loads(lib.tfx_prof_collect().decode())
        finally:
            lib.tfx_prof_enable(0)
        assert sorted(prof) == names and all(v["calls"] == 1 for v in prof.values()), prof


def test_cpu_tensor_is_refused():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext().compressor_forward(torch.zeros(2, 64), *reduced({}), 2, None, False, 0)


def test_zz_report_largest_deviations():
    """Not a check: prints the largest deviation the tests above saw per dtype (DESIGN.md section 4.12 records them)."""
    for k, (dy, dg, ds) in sorted(WORST.items()):
        print(f"compressor worst [{k}]: y excess over the float32 rounding / max|y| {dy:.3e}, gain {dg:.3e}, state {ds:.3e}")
