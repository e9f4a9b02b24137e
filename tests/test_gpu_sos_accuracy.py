"""Accuracy of the SOS cascade (csrc/sos.hip) at 48, 96 and 192 kHz on the designs whose poles sit next to z = 1, against a
__float128 recursion (tests/sos_reference.py; tests/test_sos_reference_host.py proves that reference and the grid's facts).
Every expected value comes from the wide oracle, never from the code under test.

Bars:
* float32 results: the project's TOL_IIR_F32OUT of the output scale, and at most 1 % of the outputs may differ from the float32
  rounding of the truth -- the sequential float64 recursion differs on less than 0.1 % on every case.
* float64 results (outputs, section outputs, states, bank and sum outputs): err <= F max(e_seq, 8 2^-53) with F = 4 and e_seq
  the sequential float64 recursion's own distance from the truth on the same case, computed here from the two oracles.  F: the
  largest e_seq moves by up to 1.7 times between seeds, and a refined lane scan sits at up to 1.7 times e_seq in emulation.
* returned states: float64 values in every run, held to the float64 bar of their section; in float32 runs of a cascade the
  float32 rule leaves unrefined (replayed error of the lane scan below 1e-10), to F times that rule where it is wider.
* block energies: |S - S_wide| <= F max(max over blocks |S_seq - S_wide|, 8 2^-53 S_wide) per block.
Every figure is printed ("SOSACC ...") before it is asserted; profiles/sos_accuracy.txt is such a run.
"""
import numpy as np
import pytest
import torch

from tests import sos_reference as R
from tests.gpu_common import DEV, TOL_IIR_F32OUT, ext

pytestmark = pytest.mark.gpu

WRONG32_MAX = 0.01
CHUNK = 4096


def dev(a, dtype=None):
    a = np.array(a, dtype=dtype)              # a copy: the shared references are read-only arrays
    return torch.from_numpy(a).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def tsos(c):
    return torch.from_numpy(c.sos.copy())


def check32(what, y, ref, tol=TOL_IIR_F32OUT):
    y = host(y)
    assert y.dtype == np.float32
    e, w = R.err(y, ref), R.wrong32(y, ref)
    print(f"SOSACC f32 {what}: err {e:.2e} wrong32 {w:.2e}")
    assert e <= tol, f"{what}: err {e:.3e} > {tol:.3e}"
    assert w <= WRONG32_MAX, f"{what}: {w:.2%} of the float32 outputs are not the rounded truth"


def check64(what, y, ref, e_seq):
    y = host(y) if isinstance(y, torch.Tensor) else y
    assert y.dtype == np.float64
    e, b = R.err(y, ref), R.bar(e_seq)
    print(f"SOSACC f64 {what}: e_seq {e_seq:.2e} err {e:.2e} ratio {e / max(e_seq, R.FLOOR):.2f}")
    assert e <= b, f"{what}: err {e:.3e} > {R.F} x max(e_seq = {e_seq:.3e}, {R.FLOOR:.1e})"


UNREFINED_F32 = 4e-10     # see check_states


def check_states(what, c, sx, sy, f64, refined=None):
    """state_x = the last two inputs of every section, state_y[s] = the last two outputs of section s ([K, C, 2], newest
    first).  Section 0's inputs are the signal: exact.  Everything else is a float64 section output, whatever the dtype of
    the stored samples, and gets that section's float64 bar, F max(e_sec, 8 2^-53) of the section's scale -- with one
    exception the library documents: a launch with a float32 result leaves a cascade unrefined while the replayed error of
    its lane scan stays below 1e-10 of the output scale, so the states such a launch returns are held to
    F times that, 4e-10, where that is the wider of the two.  `refined` = plan info's refine_f32 for float32 results."""
    sx, sy = host(sx), host(sy)
    assert sx.shape == c.sx.shape and sy.shape == c.sy.shape
    assert np.array_equal(sx[0], c.sx[0]), f"{what}: state_x[0] is not the last two samples of the signal"
    if not f64 and refined is None:
        refined = ext().sos_plan_info(c.sos)["refine_f32"]
    for s in range(c.K):
        scale = R.scale_of(c.sec[s])
        rel = R.bar(c.e_sec[s]) if (f64 or refined) else max(R.bar(c.e_sec[s]), UNREFINED_F32)
        tol = rel * scale
        ey = float(np.abs(sy[s] - c.sy[s]).max())
        ex = float(np.abs(sx[s + 1] - c.sx[s + 1]).max()) if s + 1 < c.K else 0.0
        print(f"SOSACC state {what} section {s}: e_sec {c.e_sec[s]:.2e} err {max(ex, ey) / scale:.2e} "
              f"ratio {max(ex, ey) / scale / max(c.e_sec[s], R.FLOOR):.2f} bar {rel:.1e}")
        assert ey <= tol, f"{what}: state_y[{s}] off by {ey:.3e} > {tol:.3e}"
        assert ex <= tol, f"{what}: state_x[{s + 1}] off by {ex:.3e} > {tol:.3e}"


# ---- (1) float32 in, float32 out, default precision: every tile variant ------------------------------------------------------
@pytest.mark.parametrize("name,fs", R.GRID, ids=R.GRID_IDS)
def test_float32_results(name, fs, sos_variant):
    """A cascade that takes the refined start states runs the shipping geometry under every variant (LC = 64 here): for the
    hard designs the six runs are one kernel, and the variants' own kernels are exercised by the cascades left unrefined."""
    c = R.case(name, fs)
    y, sx, sy = ext().sos_forward(dev(c.x), None, tsos(c), None, None)
    check32(f"{name}@{fs} variant {sos_variant}", y, c.y)
    check_states(f"{name}@{fs}", c, sx, sy, f64=False)


@pytest.mark.parametrize("fs", R.RATES)
def test_float32_results_on_unaligned_rows(fs):
    """T = 65535: rows that do not start on 16 bytes take the dword path."""
    c = R.case(R.HIGHPASS_20, fs, R.ROWS, R.T - 1)
    y, sx, sy = ext().sos_forward(dev(c.x), None, tsos(c), None, None)
    check32(f"{R.HIGHPASS_20}@{fs} T={R.T - 1}", y, c.y)
    check_states(f"{R.HIGHPASS_20}@{fs} T={R.T - 1}", c, sx, sy, f64=False)


@pytest.mark.parametrize("fs", R.RATES)
def test_float32_results_through_the_fused_epilogue(fs):
    """gain = 0.5 is exact on the rounded sample: the reference is the wide result halved."""
    c = R.case(R.HIGHPASS_20, fs)
    y, _, _ = ext().sos_forward(dev(c.x), None, tsos(c), None, None, epilogue=ext().Epilogue(gain=0.5))
    y = host(y)
    assert y.dtype == np.float32
    e, w = R.err(2.0 * y.astype(np.float64), c.y), R.wrong32(y, 0.5 * c.y)
    print(f"SOSACC f32 {R.HIGHPASS_20}@{fs} epilogue gain 0.5: err {e:.2e} wrong32 {w:.2e}")
    assert e <= TOL_IIR_F32OUT and w <= WRONG32_MAX, (e, w)


@pytest.mark.parametrize("fs", R.RATES)
def test_float32_results_in_the_unit_b0_and_the_plain_form(fs):
    """The shipping geometry runs cascades of two and more sections in the unit-b0 form and single sections in the plain
    form; plan info says which, and says that the hard designs take the refined start states and the benign one does not."""
    for name, unit in ((R.HIGHPASS_20, True), ("notch50_q30", False)):
        c = R.case(name, fs)
        info = ext().sos_plan_info(c.sos)
        assert info["unit_form"] is unit and info["refine_f32"] and info["refine_f64"], (name, fs, info)
        y, _, _ = ext().sos_forward(dev(c.x), None, tsos(c), None, None)
        check32(f"{name}@{fs} {'unit-b0' if unit else 'plain'} form", y, c.y)
    info = ext().sos_plan_info(R.design("lp2k_butter4", fs))
    assert info["unit_form"] and not info["refine_f32"] and not info["refine_f64"], info


# ---- (2) float64 results -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fs", R.GRID, ids=R.GRID_IDS)
def test_float64_results(name, fs):
    c = R.case(name, fs)
    E, sos = ext(), tsos(c)
    y, sx, sy = E.sos_forward(dev(c.x, np.float64), None, sos, None, None)
    check64(f"{name}@{fs} f64->f64", y, c.y, c.e_seq)
    check_states(f"{name}@{fs} f64->f64", c, sx, sy, f64=True)
    y, sx, sy = E.sos_forward(dev(c.x), None, sos, None, None, out_dtype=torch.float64)
    check64(f"{name}@{fs} f32->f64", y, c.y, c.e_seq)
    check_states(f"{name}@{fs} f32->f64", c, sx, sy, f64=True)
    y, sx, sy, sec = E.sos_forward(dev(c.x, np.float64), None, sos, None, None, return_sections=True)
    sec = host(sec)
    for s in range(c.K):
        check64(f"{name}@{fs} section {s}", sec[s], c.sec[s], c.e_sec[s])
    check64(f"{name}@{fs} with sections", y, c.y, c.e_seq)


@pytest.mark.parametrize("fs", R.RATES)
def test_float64_bank_and_sum(fs):
    """Two hard cascades as the bands of a bank (every band against its own wide result) and of the sum mode (against the
    sum of the wide band outputs; the sequential recursion's error of the sum is the error of the two float64 outputs added)."""
    a, b = R.case(R.HIGHPASS_20, fs), R.case("hp20_cheby1_4", fs)
    banks = torch.from_numpy(np.stack([a.sos, b.sos]))
    x = dev(a.x, np.float64)
    y, sx, sy = ext().sos_bank_forward(x, banks, None, None)
    y = host(y).reshape(2, R.ROWS, R.T)
    check64(f"bank@{fs} band 0", y[0], a.y, a.e_seq)
    check64(f"bank@{fs} band 1", y[1], b.y, b.e_seq)
    ys, _, _ = ext().sos_bank_sum_forward(x, banks, None, None)
    ref = a.y + b.y
    check64(f"sum@{fs}", ys, ref, R.err(a.y_seq + b.y_seq, ref))


# ---- (3) carried states: 16 chunks of 4096 samples against the one-shot wide result ---------------------------------------------
@pytest.mark.parametrize("name,fs", R.GRID, ids=R.GRID_IDS)
def test_chunks_with_carried_states(name, fs):
    c = R.case(name, fs)
    E, sos = ext(), tsos(c)
    for f64 in (False, True):
        x = dev(c.x, np.float64 if f64 else np.float32)
        sx = sy = None
        out = []
        for n0 in range(0, R.T, CHUNK):
            y, sx, sy = E.sos_forward(x[:, n0:n0 + CHUNK].contiguous(), None, sos, sx, sy)
            out.append(y)
        y = torch.cat(out, dim=1)
        what = f"{name}@{fs} {R.T // CHUNK} chunks"
        if f64:
            check64(what + " f64", y, c.y, c.e_seq)
        else:
            check32(what + " f32", y, c.y)
        check_states(what, c, sx, sy, f64=f64)


# ---- (4) time segments -------------------------------------------------------------------------------------------------------
SEG_ROWS, SEG_T = 2, 262144


@pytest.mark.parametrize("nseg", [2, 3])
@pytest.mark.parametrize("fs", R.RATES)
def test_time_segments(fs, nseg, monkeypatch):
    """Rows cut into 2 and 3 segments that start from a warm-up halo: every grid design whose halo fits a quarter of the row."""
    E = ext()
    ran = []
    for name in R.DESIGNS:
        sos = R.design(name, fs)
        warm = E.sos_plan_info(sos)["warmup"]
        if not 0 < warm <= SEG_T // 4:
            continue
        c = R.case(name, fs, SEG_ROWS, SEG_T)
        monkeypatch.setenv("TFX_SOS_NSEG", str(nseg))
        y, sx, sy = E.sos_forward(dev(c.x, np.float64), None, tsos(c), None, None)
        monkeypatch.delenv("TFX_SOS_NSEG")
        check64(f"{name}@{fs} {nseg} segments", y, c.y, c.e_seq)
        check_states(f"{name}@{fs} {nseg} segments", c, sx, sy, f64=True)
        ran.append(name)
    # the K-weighting high-pass (38 Hz: halo 11 326, 22 952, 46 512 samples) fits at every rate, the 20 Hz Butterworth at 48 kHz
    assert {"lp2k_butter4", "kweighting"} <= set(ran) and (fs != 48000 or R.HIGHPASS_20 in ran), ran


# ---- (5) block energies --------------------------------------------------------------------------------------------------------
def block_sums(y, fs):
    """Energies of the 100 ms blocks of y [C, T], squared and summed in long double; [C, nblk] long double."""
    nblk = y.shape[1] * 10 // fs
    e = [(i * fs) // 10 for i in range(nblk + 1)]
    w = y.astype(np.longdouble)
    return np.stack([np.sum(w[:, e[i]:e[i + 1]] ** 2, axis=1) for i in range(nblk)], axis=1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("fs", [96000, 192000])
@pytest.mark.parametrize("name", ["kweighting", R.HIGHPASS_20])
def test_block_energies(name, fs, dtype):
    c = R.case(name, fs)
    s = host(ext().sos_block_energy(dev(c.x, dtype), tsos(c), fs, 10))
    s_wide, s_seq = block_sums(c.y, fs), block_sums(c.y_seq, fs)
    assert s.dtype == np.float64 and s.shape == s_wide.shape and s.shape[1] >= 3
    e_seq = float(np.abs(s_seq - s_wide).max())
    e = np.abs(s.astype(np.longdouble) - s_wide)
    bar = R.F * np.maximum(e_seq, R.FLOOR * s_wide)
    print(f"SOSACC energy {name}@{fs} {np.dtype(dtype).name}: e_seq {e_seq:.2e} err {float(e.max()):.2e} "
          f"ratio {float((e / np.maximum(e_seq, R.FLOOR * s_wide)).max()):.2f} (energies about {float(s_wide.mean()):.0f})")
    assert np.all(e <= bar), (float(e.max()), e_seq)


# ---- (6) precision = "auto" ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", R.RATES)
def test_auto_precision_float32_error_is_inside_its_estimate(fs):
    ran = []
    for name in R.DESIGNS:
        c = R.case(name, fs)
        info = ext().sos_plan_info(c.sos)
        if info["auto_precision"] != "f32":
            continue
        y, _, _ = ext().sos_forward(dev(c.x), None, tsos(c), None, None, precision="f32")
        e = R.err(host(y), c.y)
        print(f"SOSACC f32math {name}@{fs}: err {e:.2e} bound {info['f32_error_bound']:.2e}")
        assert e <= info["f32_error_bound"] and e <= 2e-5, (name, fs, e, info)
        ya, _, _ = ext().sos_forward(dev(c.x), None, tsos(c), None, None, precision="auto")
        assert torch.equal(ya, y)
        ran.append(name)
    assert "lp2k_butter4" in ran, ran
