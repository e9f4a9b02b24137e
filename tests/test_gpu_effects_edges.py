"""GPU: csrc/effects.hip and csrc/select.hip at every seam of their own geometry, against the plain definitions of
tests/effects_reference.py.  Shapes come from `effects_plan_info` (vector, tile, reduce group, finish threads, stream tile), never
from a workload.  What is exact is compared exactly:

  gain, normalize apply     one / two correctly rounded operations in the signal dtype: bit for bit (NaN where the definition has one)
  abs-max                   a planted +-1.5 (NaN, inf) in an otherwise small signal must come back from every position class
  RMS of integer data       the sum of squares is an integer below 2^53: exact in any order, so sqrt(S / n) bit for bit
  branch sum                torch.equal with zeros_like + in-place adds
  delay line                exact impulses / NaN reach / zero coefficient; noise within eps (|c v[n - D]| + |y*|) per sample
  percentile select         == torch.quantile on the CPU

Misalignment that reaches the kernel: every op of the extension makes its input contiguous first, so a strided view arrives as
a fresh aligned copy.  `at_offset` builds a CONTIGUOUS tensor k elements into a larger buffer (what a slice of a longer
recording is) and asserts that its pointer is not 16-byte aligned -- the scalar branches are entered, not assumed."""
import numpy as np
import pytest
import torch

from tests import effects_reference as R
from tests.gpu_common import DEV, dev, ext

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}
TDT = {"f32": torch.float32, "f64": torch.float64}
IDT = {"f32": torch.int32, "f64": torch.int64}
OFFSETS = {"f32": (0, 1, 2, 3), "f64": (0, 1)}          # elements: every residue of a 16-byte vector
BOTH = pytest.mark.parametrize("dt", ["f32", "f64"])
WORST = {}


def plan(dt, T=0):
    return ext().effects_plan_info(T, TDT[dt])


def lengths(dt):
    p = plan(dt)
    vec, tile, G = p["vec"], p["tile"], p["group"]
    return sorted({1, 2, vec - 1, vec, vec + 1, tile - 1, tile, tile + 1, G - 1, G, G + 1, 2 * G + tile + 3})


def at_offset(src, k):
    """A contiguous device tensor with the shape and bits of `src` (numpy array or tensor) whose first element lies k elements
    into a 16-byte aligned allocation; asserts that it is misaligned exactly when k is no multiple of the vector."""
    s = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src))
    n = s.numel()
    buf = torch.empty(n + k + 8, dtype=s.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[k:k + n].view(s.shape)
    t.copy_(s)
    assert t.is_contiguous() and t.shape == s.shape
    assert (t.data_ptr() % 16 != 0) == ((k * s.element_size()) % 16 != 0)
    if k:
        assert t.data_ptr() % 16 != 0
    return t


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same(got, ref, what):
    """Bit for bit outside NaNs (so the sign of a zero counts), NaN exactly where the definition has one."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, got.dtype, ref.shape, ref.dtype)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs at {np.flatnonzero(np.isnan(got) != nan)[:5]}"
    bad = np.flatnonzero((bits(got) != bits(ref)).reshape(-1) & ~nan.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[0]}: got {got.reshape(-1)[bad[0]]!r}, expected {ref.reshape(-1)[bad[0]]!r}"


def specials(dtype):
    one, ulp, tiny = dtype(1), np.finfo(dtype).eps, np.finfo(dtype).smallest_subnormal
    return np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, one, -one, one + ulp, -(one + ulp), one - ulp / 2, tiny, -tiny, 37 * tiny,
                     np.finfo(dtype).tiny, one / dtype(0.731), -one / dtype(0.731), 0.5, -0.5, 2.0, 1.368], dtype)


def raw(dt, v):
    """The bit pattern of v (a float, or an int that already is one) as the signed integer a device int view takes."""
    if isinstance(v, float):
        return int(np.array([v], DT[dt]).view(np.int32 if dt == "f32" else np.int64)[0])
    return int(np.array([v], np.uint32 if dt == "f32" else np.uint64).view(np.int32 if dt == "f32" else np.int64)[0])


NEG_NAN = {"f32": 0xFFC00001, "f64": 0xFFF8000000000001}        # quiet NaNs with the sign bit set and a payload
POS_NAN = {"f32": 0x7FC00000, "f64": 0x7FF8000000000000}


# ---------------------------------------------------------------------------------------------- 0. the geometry
def test_plan_info_gives_the_geometry_the_tests_assume():
    assert plan("f32", 3 * 8192 + 1) == dict(vec=4, tile=1024, group=8192, groups=4, finish_threads=1024, stream_tile=1024)
    assert plan("f64", 3 * 4096 + 1) == dict(vec=2, tile=512, group=4096, groups=4, finish_threads=1024, stream_tile=1024)
    for dt in DT:
        p = plan(dt)
        assert p["tile"] == 256 * p["vec"] and p["group"] == 8 * p["tile"] and plan(dt, 1025 * p["group"] + 5)["groups"] == 1026
        assert len(lengths(dt)) == (12 if dt == "f32" else 10)            # float64: vec - 1 = 1 and vec = 2 are in the set already


# ---------------------------------------------------------------------------------------------- 1. gain
@BOTH
def test_gain_every_length_offset_and_special_value(dt):
    e, dtype = ext(), DT[dt]
    sp = specials(dtype)
    cases = []
    for T in lengths(dt):
        x = np.random.default_rng(T).uniform(-2, 2, T).astype(dtype)
        for i, v in enumerate(sp):
            x[(3 + 5 * i) % T] = v
        cases.append(x)
    cases.append(np.tile(sp, plan(dt)["tile"] // len(sp) + 2)[:plan(dt)["tile"] + 3])          # every special in both branches
    assert np.isnan(cases[-1]).any() and np.signbit(cases[-1][cases[-1] == 0]).any()
    assert dt == "f64" or ((np.abs(cases[-1]) < np.finfo(np.float32).tiny) & (cases[-1] != 0)).any()      # float32 denormals
    for x in cases:
        for k in OFFSETS[dt]:
            xd = at_offset(x, k)
            for g in (0.731, -2.0, 0.0):
                for clamp in (False, True):
                    assert_same(e.gain_forward(xd, g, clamp), R.gain_ref(x, g, clamp), f"gain {dt} T={x.size} k={k} g={g} clamp={clamp}")
            assert_same(xd, x, "the input is never written")
    x2 = np.random.default_rng(9).uniform(-2, 2, (3, plan(dt)["tile"] + 1)).astype(dtype)                # [C, T] at an offset
    assert_same(e.gain_forward(at_offset(x2, 1), 0.731, True), R.gain_ref(x2, 0.731, True), "gain 2-D")


# ---------------------------------------------------------------------------------------------- 2. statistics, planted
def position_classes(dt, T):
    p = plan(dt)
    vec, tile, G = p["vec"], p["tile"], p["group"]
    full = (T // tile) * tile
    assert T % 2 == 1 and T > 2 * G and full < T - 1, "an odd length with a ragged tail of at least two samples past two groups"
    c = {"first": 0, "last of vector 0": vec - 1, "first of vector 1": vec, "last lane of wave 0": 64 * vec - 1,
         "first lane of wave 1": 64 * vec, "last of tile 0": tile - 1, "first of tile 1": tile, "last of group 0": G - 1,
         "first of group 1": G, "last of the last full tile": full - 1, "first of the ragged tail": full,
         "last of the ragged tail (T - 1)": T - 1}
    # each index is in the class it is named for: (thread, element) = ((n mod tile) / vec, n mod vec), wave = thread / 64
    where = {k: dict(group=n // G, tile=n // tile, wave=n % tile // vec // 64, lane=n % tile // vec % 64, elem=n % vec) for k, n in c.items()}
    assert where["last of vector 0"] == dict(group=0, tile=0, wave=0, lane=0, elem=vec - 1)
    assert where["first of vector 1"] == dict(group=0, tile=0, wave=0, lane=1, elem=0)
    assert where["last lane of wave 0"] == dict(group=0, tile=0, wave=0, lane=63, elem=vec - 1)
    assert where["first lane of wave 1"] == dict(group=0, tile=0, wave=1, lane=0, elem=0)
    assert where["last of tile 0"] == dict(group=0, tile=0, wave=3, lane=63, elem=vec - 1)
    assert where["first of tile 1"] == dict(group=0, tile=1, wave=0, lane=0, elem=0)
    assert where["last of group 0"] == dict(group=0, tile=7, wave=3, lane=63, elem=vec - 1)
    assert where["first of group 1"] == dict(group=1, tile=8, wave=0, lane=0, elem=0)
    last_full = where["last of the last full tile"]
    assert (last_full["tile"] + 1) * tile <= T < (last_full["tile"] + 2) * tile and (last_full["wave"], last_full["lane"], last_full["elem"]) == (3, 63, vec - 1)
    assert where["first of the ragged tail"] == dict(group=2, tile=last_full["tile"] + 1, wave=0, lane=0, elem=0)
    assert where["last of the ragged tail (T - 1)"]["tile"] == last_full["tile"] + 1 and c["last of the ragged tail (T - 1)"] == T - 1
    return c


def planted_base(dt, k, seed=0):
    """[3, T] on the device at offset k with |x| <= 0.5, its numpy twin, and which rows start misaligned."""
    p = plan(dt)
    T = 2 * p["group"] + p["tile"] + 3
    x = np.random.default_rng(100 + seed).uniform(-0.5, 0.5, (3, T)).astype(DT[dt])
    t = at_offset(x, k)
    mis = [(t.data_ptr() + r * T * t.element_size()) % 16 != 0 for r in range(3)]
    return t, x, mis


@BOTH
def test_absmax_planted_in_every_position_class(dt):
    """One +-1.5 in a signal of |x| <= 0.5 must be the row's and the tensor's abs-max wherever it sits; the other rows keep their
    own maxima.  Odd T: with k = 0 row 0 is aligned (vector branch) and row 1 is not (scalar branch); the offsets move that."""
    e = ext()
    seen = set()
    for k in OFFSETS[dt]:
        t, x, mis = planted_base(dt, k)
        if k == 0:
            assert not mis[0] and mis[1] and (mis[2] or dt == "f64")
        own = R.absmax_ref(x)
        assert (own <= 0.5).all()
        ti = t.view(IDT[dt])
        T = x.shape[1]
        for ci, (name, pos) in enumerate(position_classes(dt, T).items()):
            for row in range(3):
                v = 1.5 if (ci + row) % 2 else -1.5
                keep = int(ti[row, pos])
                ti[row, pos] = raw(dt, v)
                per = e.stat_forward(t, e.STAT_ABSMAX, per_row=True).cpu().numpy()
                glob = e.stat_forward(t, e.STAT_ABSMAX).cpu().numpy()
                ti[row, pos] = keep
                exp = own.copy()
                exp[row] = 1.5
                assert np.array_equal(per, exp), f"{dt} k={k} {name} (index {pos}) row {row}: per row {per} != {exp}"
                assert glob.tolist() == [1.5], f"{dt} k={k} {name} (index {row * T + pos} of the flat view): {glob}"
                seen.add((name, mis[row]))
        assert np.array_equal(e.stat_forward(t, e.STAT_ABSMAX, per_row=True).cpu().numpy(), own)         # everything was put back
    names = set(position_classes(dt, 2 * plan(dt)["group"] + plan(dt)["tile"] + 3))
    assert seen == {(n, m) for n in names for m in (False, True)}, "every class on an aligned and on a misaligned row"


@BOTH
def test_absmax_non_finite_wins_from_every_position_class(dt):
    e = ext()
    for k in (0, 1):
        t, x, _ = planted_base(dt, k, seed=1)
        own = R.absmax_ref(x)
        ti = t.view(IDT[dt])
        for ci, (name, pos) in enumerate(position_classes(dt, x.shape[1]).items()):
            row = ci % 3
            keep = int(ti[row, pos])
            for what, pattern, exp in (("NaN", raw(dt, POS_NAN[dt]), np.nan), ("-NaN", raw(dt, NEG_NAN[dt]), np.nan),
                                       ("inf", raw(dt, float("inf")), np.inf), ("-inf", raw(dt, float("-inf")), np.inf)):
                ti[row, pos] = pattern
                per = e.stat_forward(t, e.STAT_ABSMAX, per_row=True).cpu().numpy()
                glob = e.stat_forward(t, e.STAT_ABSMAX).cpu().numpy()
                want = own.copy()
                want[row] = exp
                assert np.array_equal(per, want, equal_nan=True), f"{dt} k={k} {what} at {name} row {row}: {per}"
                assert np.array_equal(glob, [exp], equal_nan=True), f"{dt} k={k} {what} at {name}: {glob}"
                if what == "inf":                      # a NaN beats an inf, whichever comes first
                    other = (pos + x.shape[1] // 2) % x.shape[1]
                    keep2 = int(ti[row, other])
                    ti[row, other] = raw(dt, NEG_NAN[dt])
                    assert np.isnan(e.stat_forward(t, e.STAT_ABSMAX, per_row=True).cpu().numpy()[row])
                    ti[row, other] = keep2
            ti[row, pos] = keep
    z = np.full((2, plan(dt)["tile"] + 5), -0.0, DT[dt])
    for k in (0, 1):
        st = e.stat_forward(at_offset(z, k), e.STAT_ABSMAX, per_row=True).cpu().numpy()
        assert st.tolist() == [0.0, 0.0] and not np.signbit(st).any(), "an all -0.0 row gives +0.0"


@BOTH
def test_nan_in_the_sum_of_squares_gives_nan_rms_and_an_unchanged_signal(dt):
    e = ext()
    t, x, _ = planted_base(dt, 1, seed=2)
    for ci, (name, pos) in enumerate(position_classes(dt, x.shape[1]).items()):
        row = ci % 3
        ti = t.view(IDT[dt])
        keep = int(ti[row, pos])
        ti[row, pos] = raw(dt, NEG_NAN[dt] if ci % 2 else POS_NAN[dt])
        xn = t.cpu().numpy()
        rms = e.stat_forward(t, e.STAT_RMS, per_row=True).cpu().numpy()
        assert np.isnan(rms[row]) and not np.isnan(np.delete(rms, row)).any(), (name, rms)
        assert np.isnan(e.stat_forward(t, e.STAT_RMS).cpu().numpy()).all()
        assert_same(e.normalize_forward(t, 0.9, e.STAT_RMS, False), xn, f"NaN at {name}: `nan > 0` is false, the signal is returned")
        ti[row, pos] = keep


def big_row(dt, k):
    """[1, 1025 G + 5] made on the device: (x_int, N) with x_int[n] = (n mod 7) - 3 at element offset k."""
    G = plan(dt)["group"]
    N = 1025 * G + 5
    buf = torch.empty(N + 8, dtype=TDT[dt], device=DEV)
    t = buf[k:k + N].view(1, N)
    t.copy_((torch.arange(N, device=DEV) % 7 - 3).view(1, N))
    assert t.is_contiguous() and (t.data_ptr() % 16 != 0) == (k != 0)
    return t, N


@BOTH
def test_row_longer_than_the_finish_workgroup(dt):
    """1025 G + 5 samples: 1026 partials for 1024 finish threads.  A maximum in group 1023 (the last partial of the first strided
    trip), 1024 (the first of the second) and 1025 (the ragged last group) must all come back; and the integer signal's RMS
    is exact over both trips."""
    e = ext()
    G = plan(dt)["group"]
    for k in (0, 1):
        t, N = big_row(dt, k)
        q = plan(dt, N)
        assert q["groups"] == 1026 > q["finish_threads"] == 1024
        S = 28 * (N // 7) + sum((j - 3) ** 2 for j in range(N % 7))
        exp = np.sqrt(np.float64(S) / np.float64(N))
        assert S < 2 ** 53
        for per_row in (True, False):
            got = e.stat_forward(t, e.STAT_RMS, per_row=per_row).cpu().numpy()
            assert got.tolist() == [exp], f"{dt} k={k} per_row={per_row}: RMS {got[0]!r} != {exp!r} (S = {S})"
        t.mul_(0.125)                                       # |x| <= 0.375, exact
        assert e.stat_forward(t, e.STAT_ABSMAX).item() == 0.375
        ti = t.view(IDT[dt])
        for name, pos, grp in (("group 1023, first", 1023 * G, 1023), ("group 1023, last", 1024 * G - 1, 1023),
                               ("group 1024, first", 1024 * G, 1024), ("group 1024, last", 1025 * G - 1, 1024),
                               ("last group, first", 1025 * G, q["groups"] - 1), ("last group, last", N - 1, q["groups"] - 1)):
            assert pos // G == grp and 0 <= pos < N and (grp < q["finish_threads"]) == (grp == 1023)      # first trip | second trip
            keep = int(ti[0, pos])
            ti[0, pos] = raw(dt, -1.5 if pos % 2 else 1.5)
            for per_row in (True, False):
                got = e.stat_forward(t, e.STAT_ABSMAX, per_row=per_row).cpu().numpy()
                assert got.tolist() == [1.5], f"{dt} k={k} {name} (index {pos}) per_row={per_row}: {got}"
            ti[0, pos] = raw(dt, NEG_NAN[dt])
            assert np.isnan(e.stat_forward(t, e.STAT_ABSMAX).item()), name
            ti[0, pos] = keep
        assert e.stat_forward(t, e.STAT_ABSMAX).item() == 0.375
        del t


# ---------------------------------------------------------------------------------------------- 3. statistics, exact
@BOTH
def test_rms_of_integer_data_is_exact(dt):
    """x[n] = (n mod 7) - 3 over the flat [3, T]: S is an integer below 2^53, every float64 partial sum is exact in any order, so
    a skipped or twice-counted sample changes the result.  Division and square root are correctly rounded on both sides."""
    e = ext()
    for T in lengths(dt):
        kk = (np.arange(3 * T, dtype=np.int64) % 7 - 3).reshape(3, T)
        x = kk.astype(DT[dt])
        S = (kk * kk).sum(axis=1)
        exp_rows = np.sqrt(S.astype(np.float64) / np.float64(T))
        exp_all = np.sqrt(np.float64(S.sum()) / np.float64(3 * T))
        for k in OFFSETS[dt]:
            t = at_offset(x, k)
            got = e.stat_forward(t, e.STAT_RMS, per_row=True).cpu().numpy()
            assert np.array_equal(got, exp_rows), f"{dt} T={T} k={k}: per row {got} != {exp_rows} (S = {S})"
            got = e.stat_forward(t, e.STAT_RMS).cpu().numpy()
            assert got.tolist() == [exp_all], f"{dt} T={T} k={k}: global {got} != {exp_all}"
            assert np.array_equal(e.stat_forward(t, e.STAT_ABSMAX, per_row=True).cpu().numpy(), np.abs(kk).max(axis=1).astype(np.float64))


# ---------------------------------------------------------------------------------------------- 4. normalize apply, exact
MODES = [("absmax", False), ("absmax", True), ("rms", False), ("rms", True)]


def norm_signal(dt, T, seed):
    x = (np.random.default_rng(seed).uniform(-3, 3, (3, T))).astype(DT[dt])
    x[1] = 0
    x[1, ::3] = -0.0                                       # the zero row must come back bit for bit, signs included
    return x


@BOTH
def test_normalize_apply_is_exact(dt):
    """normalize_forward == (x / dtype(s)) * dtype(peak) with s the statistic stat_forward returns for the same input (proven
    exact above): a division and a multiplication, each correctly rounded, the division not contractable -- no tolerance."""
    e = ext()
    for T in lengths(dt):
        x = norm_signal(dt, T, T)
        for k in OFFSETS[dt]:
            t = at_offset(x, k)
            for stat, per_row in MODES:
                mode = e.STAT_ABSMAX if stat == "absmax" else e.STAT_RMS
                s = e.stat_forward(t, mode, per_row=per_row).cpu().numpy()
                ref = R.normalize_apply_ref(x, s, 0.9)
                assert_same(e.normalize_forward(t, 0.9, mode, per_row), ref, f"normalize {dt} T={T} k={k} {stat} per_row={per_row}")
                if per_row:
                    assert bits(ref[1]).tolist() == bits(x[1]).tolist()
            assert_same(t, x, "the input is never written")


@BOTH
def test_normalize_apply_zero_and_infinite_statistics(dt):
    e = ext()
    T = plan(dt)["tile"] + plan(dt)["vec"] + 1
    z = np.zeros((2, T), DT[dt])
    z[:, ::2] = -0.0
    x = norm_signal(dt, T, 5)
    x[2, T - 2] = -np.inf
    for k in OFFSETS[dt]:
        for stat, per_row in MODES:
            mode = e.STAT_ABSMAX if stat == "absmax" else e.STAT_RMS
            assert_same(e.normalize_forward(at_offset(z, k), 0.9, mode, per_row), z, f"all-zero signal {stat} per_row={per_row} k={k}")
            t = at_offset(x, k)
            s = e.stat_forward(t, mode, per_row=per_row).cpu().numpy()
            assert np.isinf(s[-1])
            ref = R.normalize_apply_ref(x, s, 0.9)
            assert np.isnan(ref[2, T - 2]) and not ref[2, :T - 2].any() and (per_row or not ref[0].any())      # inf / inf, x / inf
            assert_same(e.normalize_forward(t, 0.9, mode, per_row), ref, f"row with an inf {stat} per_row={per_row} k={k}")


@BOTH
def test_normalize_apply_on_a_supplied_statistic(dt):
    """The apply pass alone on a raw statistic (max|x|, or the sum of squares) for [rows] and [1], zero and NaN entries included."""
    e = ext()
    T = 2 * plan(dt)["tile"] + 3
    x = norm_signal(dt, T, 6)
    for k in OFFSETS[dt]:
        t = at_offset(x, k)
        for stat in ([2.5, 0.0, float("nan")], [0.75]):
            per_row = len(stat) > 1
            sd = torch.tensor(stat, dtype=torch.float64, device=DEV)
            assert_same(e.normalize_apply(t, sd, 0.8, e.STAT_ABSMAX, per_row), R.normalize_apply_ref(x, np.array(stat), 0.8),
                        f"apply absmax {dt} k={k} {stat}")
            n = T if per_row else 3 * T
            with np.errstate(all="ignore"):
                rms = np.sqrt(np.array(stat) / np.float64(n))
            assert_same(e.normalize_apply(t, sd, 0.8, e.STAT_RMS, per_row), R.normalize_apply_ref(x, rms, 0.8), f"apply rms {dt} k={k} {stat}")


# ---------------------------------------------------------------------------------------------- 5. branch sum
def sum_variants(dt, n):
    """Per-input element offsets: all aligned, all at each misaligned offset, one misaligned among aligned, only the last
    misaligned, and a mixture."""
    v = {"aligned": [0] * n}
    for k in OFFSETS[dt][1:]:
        v[f"all at {k}"] = [k] * n
    v["one misaligned"] = [1 if i == n // 2 else 0 for i in range(n)]
    v["only the last misaligned"] = [0] * (n - 1) + [1]
    v["mixed"] = [OFFSETS[dt][(i + 1) % len(OFFSETS[dt])] for i in range(n)]
    return v


@BOTH
def test_branch_sum_equals_sequential_adds(dt):
    e = ext()
    for T in lengths(dt):
        master = dev(np.random.default_rng(T).uniform(-1, 1, (17, T)).astype(DT[dt]))
        for n in (1, 2, 16, 17):
            ref = torch.zeros_like(master[0])
            for i in range(n):
                ref += master[i]
            for name, offs in sum_variants(dt, n).items():
                xs = [at_offset(master[i], k) for i, k in enumerate(offs)]
                assert any(t.data_ptr() % 16 for t in xs) == (name != "aligned")
                if name == "only the last misaligned":
                    assert [t.data_ptr() % 16 != 0 for t in xs] == [False] * (n - 1) + [True]
                got = e.sum_forward(xs)
                assert torch.equal(got, ref), f"sum {dt} T={T} n={n} {name}: {int((got != ref).sum())} elements differ"
    x2 = [at_offset(np.random.default_rng(i).uniform(-1, 1, (3, 1025)).astype(DT[dt]), i % 2) for i in range(3)]     # [C, T]
    assert torch.equal(e.sum_forward(x2), (torch.zeros_like(x2[0]) + x2[0] + x2[1]) + x2[2])


# ---------------------------------------------------------------------------------------------- 6. delay line, one-shot
DECAY, MIX = 0.6, 0.45


def delay_cases(dt):
    """(D, T) with T > D: every D of the issue's set at T = D + 1, tile + 1, 2 tile + 3 and the aligned 3 tile, and D = T - 1."""
    p = plan(dt)
    vec, tile = p["vec"], p["tile"]
    Ds = sorted({0, 1, vec - 1, vec, vec + 1, tile - 1, tile, tile + 1})
    Ts = [tile + 1, 2 * tile + 3, 3 * tile]
    out = {(D, D + 1) for D in Ds}
    for T in Ts:
        out |= {(D, T) for D in Ds + [T - 1] if D < T}
    return sorted(out)


def check_delay(what, got, x, D, dt, hist=None, tile=None):
    y, bnd, term = R.delay_line_ref(x, D, DECAY, MIX, hist)
    got = got.cpu().numpy()
    assert got.shape == x.shape and got.dtype == x.dtype
    err = np.abs(got.astype(np.longdouble) - y).astype(np.float64)
    ok = err <= bnd
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, 0.0, err)), err.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} outputs outside the bound; worst at {i}: err {err[i]:.3e}, bound {bnd[i]:.3e}")
    if tile:                                               # at work: the delayed term is far above the bound somewhere in every tile it reaches
        first = 0 if hist is not None else D
        for a in range(0, x.shape[1], tile):
            lo, hi = max(a, first), min(a + tile, x.shape[1])
            if lo < hi:
                assert (term[:, lo:hi] >= 1e3 * bnd[:, lo:hi]).any(axis=1).all(), f"{what}: tile at {a} does not see the delayed term"
    ratio = float((err / np.maximum(bnd, 1e-300)).max()) if err.size else 0.0
    WORST[dt] = max(WORST.get(dt, 0.0), ratio)
    return ratio


@BOTH
def test_delay_line_within_the_bound_at_every_seam(dt):
    e = ext()
    tile = plan(dt)["tile"]
    for D, T in delay_cases(dt):
        x = np.random.default_rng(D * 7919 + T).uniform(-1, 1, (3, T)).astype(DT[dt])
        for k in OFFSETS[dt]:
            t = at_offset(x, k)
            y = e.delay_line_forward(t, D, DECAY, MIX)
            assert y is not t
            check_delay(f"delay line {dt} D={D} T={T} k={k}", y, x, D, dt, tile=tile)
            assert_same(t, x, "the input is never written")
    print(f"\ndelay line err/bound, one-shot {dt}: {WORST[dt]:.4f}")


@BOTH
def test_delay_line_exact_cases(dt):
    e, dtype = ext(), DT[dt]
    tile = plan(dt)["tile"]
    c = dtype(MIX * DECAY)
    for D, T in delay_cases(dt):
        k = (D + T) % len(OFFSETS[dt])
        x = np.random.default_rng(D + T).uniform(-1, 1, (3, T)).astype(dtype)
        t = at_offset(x, k)
        for decay, mix in ((0.0, 0.5), (0.5, 0.0)):
            assert_same(e.delay_line_forward(t, D, decay, mix), x, f"zero coefficient {dt} D={D} T={T}")
        for m in sorted({0, T - D - 1, min(tile - 1, T - D - 1), (T - D - 1) // 2}):
            imp = np.zeros((3, T), dtype)
            imp[:, m] = 1
            exp = np.zeros((3, T), np.longdouble)
            exp[:, m] += 1
            exp[:, m + D] += np.longdouble(c)
            y = e.delay_line_forward(at_offset(imp, k), D, DECAY, MIX).cpu().numpy()
            assert np.array_equal(y, exp.astype(dtype)), f"impulse at {m} {dt} D={D} T={T}: nonzero at {np.flatnonzero(y[0])}, {y[0][y[0] != 0]}"
            xn = x.copy()
            xn[1, m] = np.nan
            yn = e.delay_line_forward(at_offset(xn, k), D, DECAY, MIX).cpu().numpy()
            assert [tuple(i) for i in np.argwhere(np.isnan(yn))] == sorted({(1, m), (1, m + D)}), f"NaN at {m} {dt} D={D} T={T}"
    for D in (1, tile, tile + 1):
        for T in (1, D - 1, D):
            if T >= 1:
                s = at_offset(np.ones((3, T), dtype), 1)
                assert e.delay_line_forward(s, D, DECAY, MIX) is s


# ---------------------------------------------------------------------------------------------- 7. delay line, stream
def stream_chunks(D, ST):
    return [D + 1, 0, 1, ST + 1, D - 1, D, ST, 0, 1, D + 1]


@BOTH
def test_delay_line_stream_equals_one_shot_and_the_definition(dt):
    e, dtype = ext(), DT[dt]
    ST = plan(dt)["stream_tile"]
    assert ST == 1024
    worst = 0.0
    for D in (1, 3, ST - 1, ST, ST + 1):
        chunks = stream_chunks(D, ST) if D != 3 else [0] + stream_chunks(D, ST)
        assert {0, 1, D - 1, D, D + 1, ST, ST + 1} <= set(chunks)
        total = sum(chunks)
        x = np.random.default_rng(D).uniform(-1, 1, (3, total)).astype(dtype)
        for given in (False, True):
            hist_np = np.random.default_rng(D + 1).uniform(-1, 1, (3, D)).astype(dtype) if given else None
            hist = dev(hist_np) if given else None
            ys, a = [], 0
            for n in chunks:
                xc = x[:, a:a + n]
                y, h = e.delay_line_stream_forward(dev(xc), hist, D, DECAY, MIX)
                assert y.shape == (3, n) and h.shape == (3, D)
                new = R.hist_ref(xc, D, hist_np)
                assert_same(h, new, f"stream history {dt} D={D} chunk of {n} at {a} given={given}")
                if hist_np is not None:
                    worst = max(worst, check_delay(f"stream {dt} D={D} chunk of {n} at {a} given={given}", y, xc, D, dt, hist=hist_np))
                ys.append(y)
                hist, hist_np, a = h, new, a + n
            if not given:
                one = e.delay_line_forward(dev(x), D, DECAY, MIX)
                assert torch.equal(torch.cat(ys, dim=1), one), f"stream {dt} D={D}: the chunks are not the one-shot kernel's bits"
                check_delay(f"one-shot {dt} D={D} T={total}", one, x, D, dt, tile=plan(dt)["tile"])
    print(f"\ndelay line err/bound, stream {dt}: {worst:.4f}")


# ---------------------------------------------------------------------------------------------- 8. percentile select
def test_quantile_abs_small_and_misaligned():
    e = ext()
    g = torch.Generator().manual_seed(5)
    for n in (1, 2, 3, 4, 5):
        x = torch.randn(n, generator=g)
        for k in (0, 1, 2, 3):
            xd = at_offset(x, k)
            for q in (0.0, 0.25, 0.5, 0.97, 1.0):
                ref = float(torch.quantile(x.abs(), q, interpolation="linear"))
                assert float(e.quantile_abs(xd, q).cpu()) == ref, (n, k, q)


def test_quantile_abs_ties_on_both_sides_of_the_level_boundaries():
    """Keys that differ only across bit 19 (level 1 | 2) and bit 7 (level 2 | 3), each many times over and with both signs: a bin
    picked one off, or a rank that forgets the ties below it, lands on a neighbouring key."""
    e = ext()
    base = 0x3F000000                                      # 0.5
    keys = [base + d for d in (0, (1 << 7) - 1, 1 << 7, (1 << 7) + 1, (1 << 19) - 1, 1 << 19, (1 << 19) + 1,
                               (1 << 19) + (1 << 7) - 1, (1 << 19) + (1 << 7), (2 << 19) - 1, 2 << 19)]
    vals = np.array(keys, np.uint32).view(np.float32)
    assert len(set(vals.tolist())) == len(keys) and np.all(np.diff(vals) > 0)
    rng = np.random.default_rng(8)
    for n in (len(keys), 4099, 20001):
        x = vals[rng.integers(0, len(keys), n)] * rng.choice(np.array([-1, 1], np.float32), n)
        xt = torch.from_numpy(x)
        srt = np.sort(np.abs(x))
        for k in (0, 1, 2, 3):
            xd = at_offset(xt, k)
            qs = [0.0, 0.25, 0.5, 0.75, 0.97, 1.0] + [float(i) / (n - 1) for i in np.flatnonzero(np.diff(srt) > 0)[:12]]
            for q in qs:
                ref = float(torch.quantile(xt.abs(), q, interpolation="linear"))
                assert float(e.quantile_abs(xd, q).cpu()) == ref, (n, k, q)


# ---------------------------------------------------------------------------------------------- 9. report
def test_report_worst_delay_line_deviation():
    """Printed for DESIGN.md: the largest |device - definition| / bound the delay-line tests of this file saw, per dtype."""
    for dt, w in sorted(WORST.items()):
        print(f"\ndelay line (one-shot and stream) worst err/bound {dt}: {w:.4f}")
    assert all(0.0 <= w <= 1.0 for w in WORST.values())
