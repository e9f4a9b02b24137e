"""GPU -- rows are independent signals on EVERY paired overlap-save kernel, in both directions.

Two real frames ride one complex transform; with an odd frame count per row F the last frame of row c rides with the first
frame of row c + 1 (with F = 1 every pair does).  A NaN / Inf in either frame must stay in its own row.  Every kernel that has
such a pair is reached by natural routing -- the row length comes from the plan query, (path, N, F) and the kernels' names (from
the library's profile) are asserted -- and held to the host model tests/ols_pairs_reference.py (proven against a float64
emulation in tests/test_ols_pairs_host.py): the non-finite set is exactly `poisoned_mask`, everything that shares no transform
with a hit frame is bit-equal to a clean run, the frame of the neighbouring row that rode with a poisoned frame is finite and
within the project's tolerance of a float64 convolution of its row computed on the CPU, an epilogue statistic is NaN for the
bad rows only.  Then rows that are not whole cache lines, and the FIR stream (one frame per channel: every pair straddles)."""
import functools
import json

import numpy as np
import pytest
import torch

from tests.gpu_common import *  # noqa: F401,F403
from tests.ols_pairs_reference import poisoned_mask

pytestmark = pytest.mark.gpu

PASSES16 = {"ols_col_fwd16_kernel", "ols_row_kernel", "ols_col_inv16_kernel"}           # 256-point rows run under the plain row name
PASSES18 = {"ols_col_fwd16_kernel", "ols_row1024_kernel", "ols_col_inv16_kernel"}
PASSES20 = {"ols_col_fwd16_kernel", "ols_row4096_kernel", "ols_col_inv16_kernel"}
PASSES64 = {"ols64_col_fwd_kernel", "ols64_row_kernel", "ols64_col_inv_kernel"}

# id: dtype, taps, a row length that lies in the target's routing class (the first plan query), the least row length of the
# class (0: none), frames per row, (path, N), kernels of one call.  F is the smallest odd count the route allows.
TARGETS = {
    "lds4096-f32-F1": (np.float32, 300, 2048, 0, 1, ("lds", 4096), {"ols_lds4096_kernel"}),
    "lds4096-f32-F3": (np.float32, 300, 2048, 0, 3, ("lds", 4096), {"ols_lds4096_kernel"}),
    "lds4096-f64-F1": (np.float64, 300, 2048, 0, 1, ("lds", 4096), {"ols_lds4096_kernel"}),
    "lds4096-f64-F3": (np.float64, 300, 2048, 0, 3, ("lds", 4096), {"ols_lds4096_kernel"}),
    "lds8192-f32-F1": (np.float32, 2500, 4096, 0, 1, ("lds", 8192), {"ols_lds8192_kernel"}),
    "lds8192-f32-F3": (np.float32, 2500, 4096, 0, 3, ("lds", 8192), {"ols_lds8192_kernel"}),
    "lds8192-f64-F1": (np.float64, 2500, 4096, 0, 1, ("lds", 8192), {"ols_lds8192_kernel"}),
    "lds8192-f64-F3": (np.float64, 2500, 4096, 0, 3, ("lds", 8192), {"ols_lds8192_kernel"}),
    "lds8192-f32-long": (np.float32, 1024, 65536, 65536, 11, ("lds", 8192), {"ols_lds8192_kernel"}),
    "lds16k-f32-F1": (np.float32, 6000, 8192, 0, 1, ("lds", 16384), {"ols_lds16k_kernel"}),
    "lds16k-f32-F3": (np.float32, 6000, 8192, 0, 3, ("lds", 16384), {"ols_lds16k_kernel"}),
    "lds16k-w8-f32-long": (np.float32, 6000, 65536, 65536, 7, ("lds", 16384), {"ols_lds16k_w8_kernel"}),
    "passes-2^16-f32": (np.float32, 9000, 131072, 0, 3, ("passes", 1 << 16), PASSES16),
    "passes-2^18-f32-long": (np.float32, 20000, 1 << 21, 1 << 21, 9, ("passes", 1 << 18), PASSES18),
    "passes-2^20-f32": (np.float32, 66559, 1 << 21, 0, 3, ("passes", 1 << 20), PASSES20),
    "passes-2^20-f64": (np.float64, 20000, 1 << 21, 0, 3, ("passes", 1 << 20), PASSES64),
}
MARGIN = 100          # samples between a planted position and every window edge: more than any lead (< 32) plus row shift (< 32)


def _tdt(dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


def _tol(dtype):
    return TOL_CONV_F32 if dtype == np.float32 else TOL_CONV_F64


def _profiled(fn):
    """fn() with the library's profile on: (result, names of the kernels it launched)."""
    from torchfx_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.tfx_prof_enable(1)
    lib.tfx_prof_collect()
    try:
        out = fn()
        names = set(json.loads(lib.tfx_prof_collect().decode()))
    finally:
        lib.tfx_prof_enable(0)
    return out, names


def _taps(K, dtype):
    k = np.random.default_rng(K).standard_normal(K) * np.exp(-np.arange(K) / (K / 5.0))
    return (k / np.abs(k).sum()).astype(dtype)                     # sum |k| = 1: |y| <= max |x| = 1, the tolerance's scale is 1


def _row_length(tid, unaligned=False):
    """T from the plan query: about (F - 1/2) S in whole cache lines, at least the routing class's least length; the second
    query is the one the test runs with -- (path, N, F) asserted."""
    dtype, K, T0, Tmin, F, route, _ = TARGETS[tid]
    line = 32 if dtype == np.float32 else 16
    S = ext().ols_plan_info(K, T0, (K - 1, 0), _tdt(dtype))["S"]
    T = max(int((F - 0.5) * S) // line * line, Tmin)
    if unaligned:
        T += 7
    info = ext().ols_plan_info(K, T, (K - 1, 0), _tdt(dtype))
    assert (info["path"], info["N"], info["F"]) == (*route, F), (tid, T, info)
    return T, info


@functools.lru_cache(maxsize=1)
def _target(tid, C):
    """Signal, taps, geometry, the clean run (output and per-row absmax through the epilogue) and -- on demand -- the float64
    row-wise reference of one target; shared by its NaN and Inf cases."""
    from scipy.signal import fftconvolve
    dtype, K, _, _, F, _, kernels = TARGETS[tid]
    T, info = _row_length(tid)
    x = rnd((C, T), 5 + K, dtype)
    k = _taps(K, dtype)
    kf = torch.from_numpy(k[::-1].copy())
    xd = dev(x)
    ext().fft_conv_forward(xd, kf, (K - 1, 0))                     # the filter's plan is built (on the device for the largest block) outside the profile
    clean, names = _profiled(lambda: ext().fft_conv_forward(xd, kf, (K - 1, 0)))
    assert names == kernels, f"{tid}: the call ran {sorted(names)}"
    ep = ext().Epilogue(gain=1.0, stat="absmax", per_row=True)
    ext().fft_conv_forward(xd, kf, (K - 1, 0), epilogue=ep)
    assert torch.isfinite(clean).all()

    @functools.lru_cache(maxsize=None)
    def ref_row(c):                                                 # a row's float64 convolution; the bad samples lie in OTHER rows
        return fftconvolve(x[c].astype(np.float64), k.astype(np.float64))[:T]

    return dict(K=K, T=T, F=F, S=info["S"], N=info["N"], dtype=dtype, xd=xd, kf=kf, clean=clean, stat=ep.stat_value.clone(),
                ref_row=ref_row, kernels=kernels)


def _hit(n, t):
    """Frames of a row whose windows hold sample n -- the same for every lead in [0, 64) (lead and row shift), asserted."""
    hits = {tuple(f for f in range(t["F"]) if f * t["S"] - (t["K"] - 1) - lead <= n < f * t["S"] - (t["K"] - 1) - lead + t["N"])
            for lead in range(64)}
    assert len(hits) == 1 and 0 <= n < t["T"], (n, hits)
    return hits.pop()


def _plantings(t, C):
    """name -> [(row, n)]: where the bad samples go.  F = 1: each row in turn."""
    F, S, K, T = t["F"], t["S"], t["K"], t["T"]
    if F == 1:
        return {f"row{r}": [(r, T // 2 + r)] for r in range(C)}
    last = (F - 1) * S + MARGIN                                     # behind the window of frame F - 2: the last frame alone
    both = (F - 1) * S - (K - 1) + MARGIN                           # the first samples of the last window, still inside frame F - 2's
    out = {"tail_of_row0": [(0, last)], "head_of_row1": [(1, 37)], "tail_of_row0+head_of_row1": [(0, last), (1, 37)],
           "tail_of_row2": [(2, last)], "last_two_frames_of_row0": [(0, both)]}
    assert _hit(last, t) == (F - 1,) and _hit(37, t) == (0,) and _hit(both, t) == (F - 2, F - 1)
    return out


def _hop(t, f):
    return slice(f * t["S"], min((f + 1) * t["S"], t["T"]))


def _check(t, C, plant, bad, what, worst):
    K, T, F, S, N = t["K"], t["T"], t["F"], t["S"], t["N"]
    xb = t["xd"].clone()
    for r, n in plant:
        xb[r, n] = bad
    y, names = _profiled(lambda: ext().fft_conv_forward(xb, t["kf"], (K - 1, 0)))
    assert names == t["kernels"], f"{what}: ran {sorted(names)}"
    mask = np.zeros((C, T), dtype=bool)
    shared = np.zeros((C, T), dtype=bool)                           # hops of every frame that shares a transform with a hit frame
    riders = set()                                                  # (row, frame) of another row that rode with a poisoned frame
    for r, n in plant:
        mask |= poisoned_mask(r, n, C, T, K, K - 1, N, S, F, 0)
        for f in _hit(n, t):
            g = r * F + f
            for h in (g, g ^ 1):
                if h < C * F:
                    shared[h // F, _hop(t, h % F)] = True
                    if h // F != r:
                        riders.add((h // F, h % F))
    bad_rows = sorted({r for r, _ in plant})
    riders = {(r, f) for r, f in riders if not mask[r, _hop(t, f)].any()}            # "both at once": each rider is poisoned itself
    nonfinite = ~torch.isfinite(y)
    got = nonfinite.cpu().numpy()
    assert np.array_equal(got, mask), (f"{what}: non-finite outputs differ from the mask -- outside it per row "
                                       f"{(got & ~mask).sum(axis=1).tolist()}, missing per row {(mask & ~got).sum(axis=1).tolist()}")
    keep = torch.from_numpy(~shared).to(DEV)
    assert torch.equal(y[keep], t["clean"][keep]), f"{what}: frames that share no transform with a hit frame changed"
    for r, f in sorted(riders):
        seg = y[r, _hop(t, f)].cpu().numpy().astype(np.float64)
        assert np.isfinite(seg).all()
        err = float(np.abs(seg - t["ref_row"](r)[_hop(t, f)]).max())
        worst[0] = max(worst[0], err / _tol(t["dtype"]))
        print(f"{what}: shared frame (row {r}, frame {f}) deviates by {err:.3e} = {err / _tol(t['dtype']):.3f} of the tolerance")
        assert err <= _tol(t["dtype"]), f"{what}: shared frame (row {r}, frame {f}) deviates by {err:.3e}"
    ep = ext().Epilogue(gain=1.0, stat="absmax", per_row=True)
    y2 = ext().fft_conv_forward(xb, t["kf"], (K - 1, 0), epilogue=ep)
    st = ep.stat_value
    assert torch.equal(~torch.isfinite(y2), nonfinite), f"{what}: the epilogue call's non-finite set differs"
    # the statistic: NaN for the bad rows; for every other row the maximum of what was stored, equal to the clean run's -- bit for
    # bit where the row shares no transform with a hit frame; a row with a rider frame differs from the clean run by that frame's
    # rounding (the real part of a complex product rounds differently when the imaginary operand changes), and the maxima of two
    # rows that both lie within the tolerance of the reference differ by twice the tolerance at most
    assert torch.isnan(st[bad_rows]).all(), f"{what}: statistic of the bad rows {st[bad_rows].tolist()}"
    rider_rows = sorted({r for r, _ in riders})
    plain = [c for c in range(C) if c not in bad_rows and c not in rider_rows]
    assert torch.equal(st[plain], t["stat"][plain]), f"{what}: statistic of the rows that share nothing with the bad ones changed"
    assert torch.equal(st[rider_rows], y2[rider_rows].abs().amax(dim=1).double()), f"{what}: statistic is not the stored rows' maximum"
    assert ((st[rider_rows] - t["stat"][rider_rows]).abs() <= 2 * _tol(t["dtype"])).all(), f"{what}: statistic of the rider rows"


PLANTINGS = ("tail_of_row0", "head_of_row1", "tail_of_row0+head_of_row1", "tail_of_row2", "last_two_frames_of_row0")
CASES = [(tid, C, name) for tid, spec in TARGETS.items()
         for C, names in (((2, ("row0", "row1")), (3, ("row0", "row1", "row2"))) if spec[4] == 1 else ((4, PLANTINGS),)) for name in names]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("tid,C,name", CASES, ids=[f"{tid}-C{C}-{name}" for tid, C, name in CASES])
def test_non_finite_rows_stay_apart(tid, C, name, bad):
    """Every paired kernel, both directions of a straddling pair (see the module docstring).  C = 4: pairs straddle rows 0|1 and
    2|3; F = 1: C = 2 and C = 3, each row in turn."""
    t = _target(tid, C)
    worst = [0.0]
    _check(t, C, _plantings(t, C)[name], bad, f"{tid} C={C} {name} {bad}", worst)
    print(f"RESULT {tid} C={C} {name} {bad}: kernels {sorted(TARGETS[tid][6])}, largest shared-frame deviation {worst[0]:.3f} of the tolerance")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("tid", ["lds8192-f32-F3", "passes-2^16-f32"])
def test_non_finite_rows_stay_apart_on_misaligned_rows(tid, bad):
    """T % 32 != 0 and a view that starts inside a 128-byte line: the three-pass pipeline moves every row's frame grid onto
    lines of memory (by less than 32 samples), so the hops are known to 32 samples: the non-finite set holds [n, n + K), lies in
    the mask widened by 32 samples at each hop boundary, and the other rows are finite and within tolerance of the float64
    reference."""
    from scipy.signal import fftconvolve
    dtype, K, _, _, F, _, kernels = TARGETS[tid]
    C = 4
    T, info = _row_length(tid, unaligned=True)
    assert T % 32 != 0
    t = dict(K=K, T=T, F=F, S=info["S"], N=info["N"])
    x = rnd((C, T), 11, dtype)
    k = _taps(K, dtype)
    kf = torch.from_numpy(k[::-1].copy())
    buf = torch.zeros(C * T + 32, dtype=_tdt(dtype), device=DEV)
    xv = buf[5:5 + C * T].view(C, T)
    assert xv.data_ptr() % 128 != 0
    ref = np.stack([fftconvolve(x[c].astype(np.float64), k.astype(np.float64))[:T] for c in range(C)])
    last = (F - 1) * info["S"] + MARGIN
    assert _hit(last, t) == (F - 1,) and _hit(37, t) == (0,)
    for name, (row, n) in {"tail_of_row0": (0, last), "head_of_row1": (1, 37), "tail_of_row2": (2, last)}.items():
        xb = x.copy()
        xb[row, n] = bad
        xv.copy_(torch.from_numpy(xb))
        y, names = _profiled(lambda: ext().fft_conv_forward(xv, kf, (K - 1, 0)))
        assert names == kernels, f"{tid} {name}: ran {sorted(names)}"
        got = ~np.isfinite(y.cpu().numpy())
        assert got[row, n:n + K].all(), f"{tid} {name}: the samples the bad one reaches must be non-finite"
        mask = poisoned_mask(row, n, C, T, K, K - 1, info["N"], info["S"], F, 0)[row]
        wide = np.convolve(mask.astype(np.int32), np.ones(65, dtype=np.int32), mode="same") > 0       # 32 samples to each side of every hop
        assert not (got[row] & ~wide).any(), f"{tid} {name}: {(got[row] & ~wide).sum()} non-finite outputs outside the widened mask"
        others = [c for c in range(C) if c != row]
        assert not got[others].any(), f"{tid} {name}: non-finite outputs per row {got.sum(axis=1).tolist()}"
        close(y[others], ref[others].astype(dtype), _tol(dtype), f"{tid} {name}: the other rows")


@pytest.mark.parametrize("where", ["chunk", "history"])
@pytest.mark.parametrize("K,kernel", [(300, "ols_lds4096_kernel"), (2500, "ols_lds8192_kernel")], ids=["4096", "8192"])
def test_fir_stream_channels_stay_apart(K, kernel, where):
    """A stereo FIR stream in chunks of at most one hop: one frame per channel and chunk, so EVERY pair straddles the two
    channels.  A NaN in channel 0's chunk, or only in channel 0's carried history, never reaches channel 1: finite in every chunk
    and within tolerance of the float64 convolution of the whole stream.  Channel 0 is non-finite in every chunk whose window
    (history included) holds the NaN and finite before."""
    from scipy.signal import fftconvolve
    C, chunk, H = 2, 1024, K - 1
    assert chunk <= ext().ols_plan_info(K, chunk, (H, 0))["S"]
    k = _taps(K, np.float32)
    kf = torch.from_numpy(k[::-1].copy())
    full = rnd((C, H + 3 * chunk), 21)                              # the samples before the stream (its first history), then three chunks
    n_bad = H + chunk + 100 if where == "chunk" else H - 50        # inside the second chunk / inside the history handed to the first
    zeroed = full.copy()
    zeroed[0, n_bad] = 0.0
    ref1 = fftconvolve(full[1].astype(np.float64), k.astype(np.float64))[H:H + 3 * chunk]
    ref0 = fftconvolve(zeroed[0].astype(np.float64), k.astype(np.float64))[H:H + 3 * chunk]
    full[0, n_bad] = float("nan")
    hist = dev(full[:, :H])
    for i in range(3):
        lo = H + i * chunk
        (y, hist), names = _profiled(lambda: ext().fir_stream_forward(dev(full[:, lo:lo + chunk]), kf, hist, direct=False))
        assert names == {kernel}, f"chunk {i}: ran {sorted(names)}"
        y = y.cpu().numpy()
        assert np.isfinite(y[1]).all(), f"chunk {i}: channel 0's NaN reached channel 1 ({(~np.isfinite(y[1])).sum()} samples)"
        close(y[1], ref1[i * chunk:(i + 1) * chunk].astype(np.float32), TOL_CONV_F32, f"chunk {i}, channel 1")
        if lo - H <= n_bad < lo + chunk:                            # the chunk's window (history + chunk) holds the NaN
            assert not np.isfinite(y[0]).any(), f"chunk {i}: channel 0 must be non-finite"
        else:
            close(y[0], ref0[i * chunk:(i + 1) * chunk].astype(np.float32), TOL_CONV_F32, f"chunk {i}, channel 0")
