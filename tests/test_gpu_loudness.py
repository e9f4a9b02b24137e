"""BS.1770 loudness on the device (csrc/sos.hip, the measuring pass of the cascade kernel) against the NumPy / SciPy oracle
of tests/loudness_reference.py -- never against the code under test.

Bars, all derived from the project's float64 cascade bar and the number formats:

* energy of a block of n samples: with delta = TOL_IIR_F64OUT * max(1, max|y_ref| of the row) the bound on every filtered
  sample (y is never rounded to float32, so it holds for both input dtypes),
      |S - S_ref| <= 2 delta sqrt(n S_ref) + n delta^2 + n 2^-52 S_ref
  (Cauchy-Schwarz on sum 2 y e, the squares of the errors, and the round-off of a sum of n non-negative terms);
* loudness: the energy bounds of the windows that pass both gates give a relative bound rho on their mean, and
  |L - L_ref| <= -10 log10(1 - rho).  The test asserts on the oracle that no window lies within 0.1 LU of either gate, so
  the gated sets are equal;
* normalised signal against float64 x * 10^((target - L_ref) / 20): (4 u + 0.1152 bar_L) max|expected|, u the unit
  round-off of the signal dtype (four roundings at most: the two scalars, a quotient and the product), ln(10) / 20 =
  0.1152 per LU.
"""
import math

import numpy as np
import pytest
import torch

from tests import loudness_reference as R
from tests.gpu_common import DEV, TOL_IIR_F64OUT, allpass_sos, rnd

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def fx():
    import torchfx_amd
    return torchfx_amd


def ext():
    from torchfx_amd import torchfx_ext
    return torchfx_ext


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared references are read-only arrays


class Ref:
    """A signal [C, T] and what the oracle says about it, with the bars; read-only."""

    def __init__(self, fs, x, weights=None, gating=False):
        self.fs, self.T, self.x = fs, x.shape[-1], x
        self.weights = [1.0] * x.shape[0] if weights is None else weights
        self.sos = R.kweighting_sos(fs)
        self.y = R.filtered(self.x, self.sos)
        self.e = R.edges(self.T, fs, 10)
        self.s = R.block_energy(self.x, self.sos, fs, 10, y=self.y)
        self.bar_s = energy_bar(self.y, self.s, self.e)
        self.p = R.window_power(self.s, fs, self.weights)
        self.L, self.above, self.both, self.thr = R.gate(self.p)
        self.bar_L = 0.0
        if len(self.p) and self.both.any():
            lj = R.lufs(self.p)
            # no window is near a gate: the gated sets of any measurement inside the energy bars are the oracle's
            assert np.abs(lj + 70.0).min() > 0.1 and np.abs(lj - self.thr).min() > 0.1
            self.bar_L = loudness_bar(self.bar_s, self.p, self.both, self.e, self.weights)
        if gating:                       # both gates reject something
            assert 0 < self.both.sum() < self.above.sum() < len(self.p)
        for a in (self.x, self.y, self.s, self.bar_s, self.p):
            a.setflags(write=False)

    def window_bars(self, width):
        """(loudness of every window of `width` sub-blocks, the bound on its error from the energy bars)."""
        w = np.asarray(self.weights, dtype=np.float64)
        p = R.window_power(self.s, self.fs, self.weights, width)
        dp = np.array([np.sum(w * np.sum(self.bar_s[:, j:j + width], axis=-1)) / float(self.e[j + width] - self.e[j])
                       for j in range(len(p))])
        return R.lufs(p), -10 * np.log10(1 - dp / p)


def energy_bar(y, s, e):
    n = np.diff(e).astype(np.float64)
    delta = TOL_IIR_F64OUT * np.maximum(1.0, np.abs(y).max(axis=-1, keepdims=True))
    return 2 * delta * np.sqrt(n * s) + n * delta ** 2 + n * 2.0 ** -52 * s


def loudness_bar(bar_s, p, both, e, weights):
    """bar_s [C, nblk] -> the bound on |L - L_ref| when the windows `both` are averaged."""
    w = np.asarray(weights, dtype=np.float64)
    dp = np.array([np.sum(w * np.sum(bar_s[:, j:j + 4], axis=-1)) / float(e[j + 4] - e[j]) for j in range(len(p))])
    rho = float(dp[both].sum() / p[both].sum())
    assert 0 < rho < 1e-6
    return -10 * math.log10(1 - rho)


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(fs, T, dtype):
        key = (fs, T, np.dtype(dtype).name)
        if key not in cache:
            cache[key] = Ref(fs, R.gating_signal(fs, T, dtype), R.GATING_WEIGHTS, gating=True)
        return cache[key]

    return get


def check_energy(got, s_ref, bar, what):
    got = got.cpu().numpy()
    assert got.shape == s_ref.shape and got.dtype == np.float64, (what, got.shape, s_ref.shape)
    if got.size == 0:
        return
    err = np.abs(got - s_ref)
    worst = float((err / bar).max())
    print(f"{what}: max |S - S_ref| {float(err.max()):.3e}, largest err / bar {worst:.3e}")
    assert np.isfinite(err).all() and (err <= bar).all(), f"{what}: err / bar up to {worst:.3e}"


def check_loudness(got, ref, what):
    got = float(got)
    print(f"{what}: L {got:.12f} LUFS, |L - L_ref| {abs(got - ref.L):.3e} LU (bar {ref.bar_L:.3e})")
    assert abs(got - ref.L) <= ref.bar_L, what


def nseg_in_force(ref, rows=3):
    return ext().sos_block_energy_plan_info(ref.sos, rows, ref.T, ref.fs, 10)["nseg"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", R.GATING_CASES, ids=lambda c: f"{c[0]}Hz")
def test_gating_signals_at_the_launchs_own_segmentation(refs, case, dtype):
    ref = refs(*case, dtype)
    x = dev(ref.x)
    s = fx().block_energy(x, ref.fs)
    assert s.is_cuda and s.dtype == torch.float64
    check_energy(s, ref.s, ref.bar_s, f"{case} {dtype.__name__} nseg {nseg_in_force(ref)}")
    il = fx().integrated_loudness(x, ref.fs, R.GATING_WEIGHTS)
    assert il.is_cuda and il.dtype == torch.float64 and il.dim() == 0
    check_loudness(il, ref, f"{case} {dtype.__name__}")
    for width, fn in ((4, fx().momentary_loudness), (30, fx().short_term_loudness)):
        got = fn(x, ref.fs, R.GATING_WEIGHTS).cpu().numpy()
        exp, bars = ref.window_bars(width)
        assert got.shape == exp.shape == (len(ref.e) - width,)
        print(f"windows of {width}: largest err / bar {float((np.abs(got - exp) / bars).max()):.3e}")
        assert (np.abs(got - exp) <= bars).all(), width


@pytest.mark.parametrize("nseg", [2, 3, 7])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", R.GATING_CASES, ids=lambda c: f"{c[0]}Hz")
def test_gating_signals_in_forced_segments(refs, case, dtype, nseg, monkeypatch):
    """The high-pass forgets its state in about 1400 samples at 8 kHz and 7700 at 44.1 kHz: every row is long enough for
    several segments that start from zero state that far in front of a block edge."""
    monkeypatch.setenv("TFX_SOS_NSEG", str(nseg))
    ref = refs(*case, dtype)
    used = nseg_in_force(ref)
    assert 1 < used <= nseg, (used, nseg)
    x = dev(ref.x)
    check_energy(fx().block_energy(x, ref.fs), ref.s, ref.bar_s, f"{case} {dtype.__name__} forced {nseg} -> {used} segments")
    check_loudness(fx().integrated_loudness(x, ref.fs, R.GATING_WEIGHTS), ref, f"{case} {dtype.__name__} forced {nseg}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_mono_and_batched_inputs(refs, dtype):
    ref = refs(8000, 48123, dtype)
    mono = dev(ref.x[1])
    s = fx().block_energy(mono, ref.fs)
    check_energy(s, ref.s[1], ref.bar_s[1], "[T]")
    ref1 = Ref(ref.fs, ref.x[1:2])
    got = fx().integrated_loudness(mono, ref.fs)
    assert got.dim() == 0
    check_loudness(got, ref1, "[T]")
    other = Ref(ref.fs, ref.x[::-1] * dtype(0.5), R.GATING_WEIGHTS)
    xb = np.stack([ref.x, other.x])
    sb = fx().block_energy(dev(xb), ref.fs)
    check_energy(sb, np.stack([ref.s, other.s]), np.stack([ref.bar_s, other.bar_s]), "[B, C, T]")
    ilb = fx().integrated_loudness(dev(xb), ref.fs, R.GATING_WEIGHTS)
    assert ilb.shape == (2,) and ilb.is_cuda
    check_loudness(ilb[0], ref, "[B, C, T] item 0")
    check_loudness(ilb[1], other, "[B, C, T] item 1")


@pytest.mark.parametrize("T", [799, 2399, 2400, 2401, 3199, 3200, 3201])
def test_rows_of_few_blocks(T):
    """Shorter than one block, and exactly 3 and 4 blocks of 800 samples -1 / +0 / +1 sample: 0, 2, 3, 3, 3, 4, 4 blocks;
    integrated loudness needs four."""
    fs = 8000
    x = np.random.default_rng(T).uniform(-1, 1, (2, T)).astype(np.float32)
    nblk = T // 800
    ref = Ref(fs, x)
    s = fx().block_energy(dev(x), fs)
    assert s.shape == (2, nblk) and s.is_cuda
    check_energy(s, ref.s, ref.bar_s, f"T {T}")
    got = fx().integrated_loudness(dev(x), fs)
    assert fx().momentary_loudness(dev(x), fs).shape == (max(0, nblk - 3),)
    assert fx().short_term_loudness(dev(x), fs).shape == (0,)
    if nblk < 4:
        assert float(got) == -math.inf and ref.L == -math.inf
    else:
        check_loudness(got, ref, f"T {T}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_general_cascade_and_block_length(refs, dtype, monkeypatch):
    """The op is not K-weighting-specific: a 4-section Butterworth low-pass, blocks of 1000 / 3 samples (edges 333, 666,
    1000, ...), at the launch's own segmentation and in forced segments."""
    from torchfx_amd import filter as F
    ref = refs(8000, 48123, dtype)
    f = F.LoButterworth(1200, order=8, fs=8000)
    if f._sos is None:
        f.compute_coefficients()
    sos = np.ascontiguousarray(f._sos.detach().cpu().numpy(), dtype=np.float64)
    assert sos.shape == (4, 6)
    y = R.filtered(ref.x, sos)
    e = R.edges(ref.T, 1000, 3)
    assert list(e[:4]) == [0, 333, 666, 1000] and len(e) - 1 == (ref.T * 3) // 1000
    s_ref = R.block_energy(ref.x, sos, 1000, 3, y=y)
    bar = energy_bar(y, s_ref, e)
    check_energy(ext().sos_block_energy(dev(ref.x), sos, 1000, 3), s_ref, bar, "butter8, 1000/3")
    monkeypatch.setenv("TFX_SOS_NSEG", "7")
    assert ext().sos_block_energy_plan_info(sos, 3, ref.T, 1000, 3)["nseg"] > 1
    check_energy(ext().sos_block_energy(dev(ref.x), sos, 1000, 3), s_ref, bar, "butter8, 1000/3, forced segments")
    with pytest.raises(RuntimeError, match="shorter than 64"):
        ext().sos_block_energy(dev(ref.x), sos, 191, 3)


def test_a_cascade_whose_carry_needs_more_than_64_kb_of_lds():
    """256 all-pass sections on a float32 signal, blocks of 1000 / 3 samples: from 209 sections on the launch asks for more
    dynamic LDS than a kernel gets without raising its limit first."""
    sos = allpass_sos(256)
    x = rnd((2, 20_000), 9, np.float32)
    assert ext().sos_block_energy_plan_info(sos, 2, x.shape[-1], 1000, 3)["nseg"] == 1          # nothing decays: no segments
    y = R.filtered(x, sos)
    e = R.edges(x.shape[-1], 1000, 3)
    s_ref = R.block_energy(x, sos, 1000, 3, y=y)
    assert s_ref.shape == (2, 60) and np.isfinite(s_ref).all()
    check_energy(ext().sos_block_energy(dev(x), sos, 1000, 3), s_ref, energy_bar(y, s_ref, e), "256 all-pass sections, 1000/3")


def test_deterministic_and_independent_of_the_other_rows(refs, monkeypatch):
    ref = refs(44100, 132377, np.float32)
    g = np.random.default_rng(9).uniform(-1, 1, (2, ref.T)).astype(np.float32)
    x5 = dev(np.concatenate([ref.x, g]))
    for force in (None, "3"):
        if force:
            monkeypatch.setenv("TFX_SOS_NSEG", force)
        a, b = fx().block_energy(x5, ref.fs), fx().block_energy(x5, ref.fs)
        assert torch.equal(a, b)                                            # two runs agree
        for r in range(5):
            assert torch.equal(fx().block_energy(x5[r:r + 1], ref.fs)[0], a[r]), (force, r)      # row r alone
            assert torch.equal(fx().block_energy(x5[r], ref.fs), a[r]), (force, r)
        xb = torch.stack([x5[:3], x5[2:5]])
        sb = fx().block_energy(xb, ref.fs)
        assert torch.equal(sb[0], a[:3]) and torch.equal(sb[1], a[2:5])        # [B, C, T] equals its items
        il = fx().integrated_loudness(xb, ref.fs, R.GATING_WEIGHTS)
        assert torch.equal(il[0], fx().integrated_loudness(xb[0], ref.fs, R.GATING_WEIGHTS))
        assert torch.equal(il[1], fx().integrated_loudness(xb[1], ref.fs, R.GATING_WEIGHTS))


@pytest.mark.parametrize("nseg", [1, 7])
@pytest.mark.parametrize("bad", [math.nan, math.inf], ids=["nan", "inf"])
def test_non_finite_samples_behave_as_in_the_sequential_recursion(refs, bad, nseg, monkeypatch):
    monkeypatch.setenv("TFX_SOS_NSEG", str(nseg))
    ref = refs(8000, 48123, np.float32)
    assert (nseg_in_force(ref) > 1) == (nseg > 1)
    clean = fx().block_energy(dev(ref.x), ref.fs)
    for p in (20000, 21599, 21600, 43300):           # inside a block, its last sample, its first sample, in the last segment
        x = ref.x.copy()
        x[1, p] = bad
        s = fx().block_energy(dev(x), ref.fs)
        first = p // 800
        assert torch.equal(s[0], clean[0]) and torch.equal(s[2], clean[2]), p                # the other rows keep their bits
        assert torch.equal(s[1, :first], clean[1, :first]) and bool(torch.isfinite(s[1, :first]).all()), p
        assert not bool(torch.isfinite(s[1, first:]).any()), (p, s[1, first:])
        exp = R.signal_block_energy(x, ref.fs)
        assert np.array_equal(np.isfinite(exp), np.isfinite(s.cpu().numpy()))
        xb = torch.stack([dev(x), dev(ref.x)])
        il = fx().integrated_loudness(xb, ref.fs, R.GATING_WEIGHTS)
        assert math.isnan(float(il[0])) and abs(float(il[1]) - ref.L) <= ref.bar_L
        y = fx().LoudnessNormalize(-16.0, R.GATING_WEIGHTS, fs=ref.fs)(xb)
        assert bool(torch.isnan(y[0]).all()) and bool(torch.isfinite(y[1]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_loudness_normalize_and_the_wave_pipeline(refs, dtype):
    """The gain against the oracle's, for the effect on a tensor, on a batch and behind a Wave.  The loudness of the
    normalised signal is measured on the float64 signal: a float32 product carries a gain rounded to 2^-24, 5e-7 LU,
    which is not what the loudness bar is about."""
    ref = refs(44100, 132377, dtype)
    target = -16.0
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53

    def check(y, r, what):
        exp = r.x.astype(np.float64) * 10 ** ((target - r.L) / 20)
        bar = (4 * u + 0.1152 * r.bar_L) * np.abs(exp).max()
        assert y.is_cuda and y.shape == r.x.shape and y.dtype == dev(r.x).dtype
        err = float(np.abs(y.cpu().numpy().astype(np.float64) - exp).max())
        print(f"{what} {dtype.__name__}: max err {err:.3e} (bar {bar:.3e})")
        assert err <= bar, what

    L = fx()
    check(L.LoudnessNormalize(target, R.GATING_WEIGHTS, fs=ref.fs)(dev(ref.x)), ref, "effect")
    quiet = Ref(ref.fs, ref.x * dtype(0.125), R.GATING_WEIGHTS)
    yb = L.LoudnessNormalize(target, R.GATING_WEIGHTS, fs=ref.fs)(torch.stack([dev(ref.x), dev(quiet.x)]))
    check(yb[0], ref, "batch item 0")
    check(yb[1], quiet, "batch item 1 (its own measurement)")
    w = L.Wave(dev(ref.x), ref.fs, device=DEV) | L.LoudnessNormalize(target, R.GATING_WEIGHTS)
    lines = w.explain()
    assert any("sos_block_energy_kernel" in ln and "segment" in ln for ln in lines), lines
    check(w.ys, ref, "wave")
    if dtype == np.float64:
        got = w.loudness(R.GATING_WEIGHTS)
        print(f"loudness of the normalised wave: {got:.12f} (bar {ref.bar_L:.3e})")
        assert isinstance(got, float) and abs(got - target) <= ref.bar_L
    silent = torch.zeros(2, 3, 40000, device=DEV, dtype=dev(ref.x).dtype)
    assert torch.equal(L.LoudnessNormalize(target, fs=8000)(silent), silent)
