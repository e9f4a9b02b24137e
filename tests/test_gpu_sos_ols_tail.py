"""GPU parity -- the tail geometry of the cascade-in-pass-A pipeline (`tfx_sos_fft_conv_forward` at N = 2^21): where what a
row's last frame has to deliver fits the hop of a 2^20-point frame, that frame runs at 2^20 points from t0 = (F - 1) * S
on, on the caller's stream, beside the F - 1 main frames (olsnative_tail_geometry, olsnative_forward).

Three rows: the tail frames of rows 0 and 1 share one complex transform, row 2's pair is half empty.  Row lengths around
both ends of the tail route, S_main and S_tail taken from the plan query.  References: the float64 recursion -> float32 ->
float64 FFT convolution on the CPU, and the staged pair of launches.  Tolerances: tests/gpu_common.py.

What "another row keeps its bits" can mean here: two real frames that ride one complex transform share its rounding (a
twiddle product mixes real and imaginary parts), so a frame whose PARTNER's input changes -- the flagged frame enters the
transform as zeros from the bad sample on -- changes in its last bits, as a pair of main frames always has.  So: a row is
bit-identical to the clean run wherever it shares no transform with the flagged frame (all of row 2, and every other frame
of the partner row), and on the one frame that does it is finite and meets the chain bar against the staged launches."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_common import *  # noqa: F401,F403
from tests.test_gpu_sos_ols import cfg2_sos, taps

pytestmark = pytest.mark.gpu

K = 8193
C = 3
PAD = (K - 1, 0)


@functools.lru_cache(maxsize=None)
def geometry():
    """(S_main, S_tail) of the forced 2^21-point block for these taps: from the plan query, never recomputed."""
    info = ext().sos_fft_conv_plan_info(3_000_000, cfg2_sos(), K, PAD, force_block=2)
    assert info is not None and info["N"] == 1 << 21 and info["tail_N"] == 1 << 20 and info["F"] == 2
    return info["S"], info["tail_S"]


def row_length(which):
    s_main, s_tail = geometry()
    return {"one_sample": s_main + 1, "odd": s_main + 70_001, "full_tail": s_main + s_tail, "too_long": s_main + s_tail + 1}[which]


def kernel():
    k = taps(K)
    return k, torch.from_numpy(k[::-1].copy())


def cpu_chain(y_f64, k):
    """float64 cascade output -> float32 -> causal convolution with the taps in float64 (one FFT per row)."""
    y32 = y_f64.astype(np.float32).astype(np.float64)
    T = y32.shape[-1]
    n = 1 << int(np.ceil(np.log2(T + len(k))))
    return np.fft.irfft(np.fft.rfft(y32, n) * np.fft.rfft(k.astype(np.float64), n), n)[:, :T]


@functools.lru_cache(maxsize=None)
def case(which):
    """Input, CPU reference (sections and chain) and the staged pair of launches for one row length: computed once."""
    T = row_length(which)
    sos = cfg2_sos()
    x = rnd((C, T), 31)
    k, kf = kernel()
    y64, _, _, sec = O.sos_forward(x.astype(np.float64), sos, sections=True)
    ref = cpu_chain(y64, k)
    ys, _, _ = ext().sos_forward(dev(x), None, torch.from_numpy(sos), None, None)
    staged = ext().fft_conv_forward(ys, kf, PAD).cpu().numpy()
    for a in (sec, ref, staged):                      # shared by the tests below: nobody changes them (x: tests copy it first)
        a.setflags(write=False)
    return x, sec, ref, staged


@pytest.mark.parametrize("which", ["one_sample", "odd", "full_tail", "too_long"])
def test_tail_route_against_cpu_reference_and_staged(which):
    """Row lengths S_main + 1 (a tail of one sample), S_main + 70 001 (odd: the rows' frame grids are shifted), S_main +
    S_tail (the longest tail) take the tail route; S_main + S_tail + 1 must not, and the plan query says so.  Every sample
    of every section across the main / tail seam, the chain against the CPU reference and the staged launches."""
    s_main, s_tail = geometry()
    T = row_length(which)
    sos = cfg2_sos()
    info = ext().sos_fft_conv_plan_info(T, sos, K, PAD, force_block=2)
    assert info is not None and (info["N"], info["S"], info["F"]) == (1 << 21, s_main, 2)
    if which == "too_long":
        assert (info["tail_N"], info["tail_S"]) == (0, 0)
    else:
        assert (info["tail_N"], info["tail_S"]) == (1 << 20, s_tail)
    x, sec_ref, ref, staged = case(which)
    _, kf = kernel()
    y, sec = ext().sos_fft_conv_forward(dev(x), sos, kf, PAD, return_sections=True, force_block=2)
    y2 = ext().sos_fft_conv_forward(dev(x), sos, kf, PAD, force_block=2)
    assert tuple(y.shape) == (C, T) and torch.equal(y, y2)
    for s in range(sos.shape[0]):
        close(sec[s], sec_ref[s], TOL_IIR_F64OUT, f"section {s} ({which})")
    y = y.cpu().numpy()
    for lo, hi, what in [(0, s_main - 64, "main"), (s_main - 64, min(T, s_main + 64), "seam"), (min(T, s_main + 64), T, "tail")]:
        if hi > lo:
            print(f"{which} {what}: max err vs CPU {np.abs(y[:, lo:hi] - ref[:, lo:hi]).max():.3e}, "
                  f"vs staged {np.abs(y[:, lo:hi] - staged[:, lo:hi]).max():.3e}")
    close(y, ref, TOL_CONV_F32, f"chain vs CPU reference ({which})")
    close(y, staged, TOL_CONV_F32, f"chain vs staged launches ({which})")


@pytest.mark.parametrize("where", ["main_of_row1", "tail_of_row1", "tail_of_row0"])
def test_non_finite_sample_and_the_tail(where):
    """A NaN in the main part of row 1 makes row 1 NaN through its tail; a NaN that only row 1's tail frame holds makes it
    NaN from t0 on; a NaN in row 0's tail leaves row 1, whose tail frame shares the transform, finite.  Other rows keep their
    bits in the sense of the module docstring; sections are non-finite exactly where the float64 recursion's are."""
    s_main, _ = geometry()
    T = row_length("odd")
    sos = cfg2_sos()
    x0, _, _, _ = case("odd")
    _, kf = kernel()
    row, n = {"main_of_row1": (1, s_main // 2), "tail_of_row1": (1, T - 3), "tail_of_row0": (0, T - 3)}[where]
    x = x0.copy()
    x[row, n] = float("nan")
    clean = ext().sos_fft_conv_forward(dev(x0), sos, kf, PAD, force_block=2).cpu().numpy()
    y, sec = ext().sos_fft_conv_forward(dev(x), sos, kf, PAD, return_sections=True, force_block=2)
    y = y.cpu().numpy()
    ys, _, _ = ext().sos_forward(dev(x), None, torch.from_numpy(sos), None, None)
    staged = ext().fft_conv_forward(ys, kf, PAD).cpu().numpy()
    sh = [(c * T) % 32 for c in range(C)]                     # T % 32 != 0: row c's frame grid is moved left by sh[c]
    seam = [s_main - sh[c] for c in range(C)]                 # first output sample of row c's tail frame
    start = 0 if where == "main_of_row1" else seam[row]       # first sample of the first frame whose window holds n
    fin = np.isfinite(y)
    assert fin[row, :start].all() and not fin[row, start:].any(), f"row {row} must be non-finite exactly from {start}"
    assert np.array_equal(y[row, :start], clean[row, :start])
    assert not np.isfinite(staged[row, n:]).any()
    other = 1 - row                                           # rows 0 and 1 share their main and their tail transforms
    lo, hi = (0, seam[other]) if where == "main_of_row1" else (seam[other], T)      # the frame that rode with the flagged one
    shared = np.zeros(T, dtype=bool)
    shared[lo:hi] = True
    assert fin[other].all() and fin[2].all()
    assert np.array_equal(y[2], clean[2]), "row 2 shares no transform with row 0 or 1"
    assert np.array_equal(y[other, ~shared], clean[other, ~shared]), f"row {other} outside the shared frame"
    print(f"{where}: row {other} on the shared frame: max diff to the clean run {np.abs(y[other, shared] - clean[other, shared]).max():.3e}")
    close(y[other], staged[other], TOL_CONV_F32, f"row {other} vs staged launches")
    _, _, _, ref = O.sos_forward(x.astype(np.float64), sos, sections=True)
    sec = sec.cpu().numpy()
    for s in range(sos.shape[0]):
        assert np.array_equal(np.isfinite(sec[s]), np.isfinite(ref[s])), f"section {s}: non-finite in other places than the recursion"
        m = np.isfinite(ref[s])
        close(sec[s][m], ref[s][m], TOL_IIR_F64OUT, f"section {s} (finite part)")


@pytest.mark.parametrize("per_row", [True, False], ids=["per_row", "global"])
def test_epilogue_statistic_counts_the_tail(per_row):
    """Gain and max|y| in the epilogue against gain and statistic staged behind the plain call.  Row 0 peaks in its tail
    frame, row 1 in its main frame: a row's partials of both geometries must reach the reduction."""
    s_main, _ = geometry()
    sos = cfg2_sos()
    x0, _, _, _ = case("odd")
    _, kf = kernel()
    x = x0.copy()
    x[0, :s_main] *= 0.125
    x[1, s_main - 4096:] *= 0.125
    E = ext()
    ep = E.Epilogue(gain=0.5, stat="absmax", per_row=per_row)
    y = E.sos_fft_conv_forward(dev(x), sos, kf, PAD, force_block=2, epilogue=ep)
    exp = E.sos_fft_conv_forward(dev(x), sos, kf, PAD, force_block=2) * 0.5
    assert torch.equal(y, exp)
    peak = exp.abs().amax(dim=1).double().cpu().numpy()
    assert int(exp[0].abs().argmax()) > s_main and int(exp[1].abs().argmax()) < s_main - 64
    want = peak if per_row else peak.max(keepdims=True)
    assert np.array_equal(ep.stat_value.cpu().numpy().reshape(-1), want), "max|y| is exact"
