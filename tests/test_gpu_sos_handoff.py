"""The hand-off route of the SOS cascade (csrc/sos_route.h): rows cut into segments that start from the exact
state, for cascades whose memory is too long for a warm-up halo.  Shapes are the accuracy grid's (tests/sos_reference.py), every
expected value comes from the wide oracle, the bars are tests/test_gpu_sos_accuracy.py's: F max(e_seq, FLOOR) for float64
results, section outputs and states; TOL_IIR_F32OUT and at most 1 % wrongly rounded for float32 results.  Every test asserts
through sos_route_info which route its calls take.  Every figure is printed ("SOSHO ...") before it is asserted."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import sos_reference as R
from tests.gpu_common import DEV, TOL_IIR_F32OUT, ext, rnd

pytestmark = pytest.mark.gpu

WRONG32_MAX = 0.01
UNREFINED_F32 = 4e-10     # tests/test_gpu_sos_accuracy.py::check_states
PLANT_SOS = np.array([[1.0, 0.05, 0.02, 1.0, -0.1, 0.05], [1.05, -0.08, 0.01, 1.0, 0.12, 0.04]])     # direct tap 1.05, the next ones below 0.06
INTEGRATOR = np.array([[1.0, 0, 0, 1, -1.0, 0]])
LEAKY = np.array([[1e-4, 0, 0, 1, -0.9999, 0]])
F32, F64 = torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in ("TFX_SOS_NSEG", "TFX_SOS_HANDOFF", "TFX_SOS_VARIANT"):
        monkeypatch.delenv(k, raising=False)


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)       # a copy: the shared references are read-only arrays


def host(t):
    return t.detach().cpu().numpy()


def tsos(sos):
    return torch.from_numpy(np.array(sos, dtype=np.float64))


def force(monkeypatch, nseg=0):
    monkeypatch.setenv("TFX_SOS_HANDOFF", "1")
    if nseg:
        monkeypatch.setenv("TFX_SOS_NSEG", str(nseg))
    else:
        monkeypatch.delenv("TFX_SOS_NSEG", raising=False)


def handoff_info(sos, rows, length, dtype=F32, out_dtype=None, sections=False):
    """The route of the call about to be made (current device, current knobs): it must be the hand-off."""
    info = ext().sos_route_info(sos, rows, length, dtype, out_dtype, sections=sections)
    assert info["route"] == "handoff" and info["nseg"] >= 2 and info["warmup"] == 0, info
    assert (info["nseg"] - 1) * info["seg_len"] < length <= info["nseg"] * info["seg_len"], info
    return info


def check32(what, y, ref, tol=TOL_IIR_F32OUT):
    y = host(y)
    assert y.dtype == np.float32
    e, w = R.err(y, ref), R.wrong32(y, ref)
    print(f"SOSHO f32 {what}: err {e:.2e} wrong32 {w:.2e}")
    assert e <= tol, f"{what}: err {e:.3e} > {tol:.3e}"
    assert w <= WRONG32_MAX, f"{what}: {w:.2%} of the float32 outputs are not the rounded truth"


def check64(what, y, ref, e_seq):
    y = host(y) if isinstance(y, torch.Tensor) else y
    assert y.dtype == np.float64
    e, b = R.err(y, ref), R.bar(e_seq)
    print(f"SOSHO f64 {what}: e_seq {e_seq:.2e} err {e:.2e} ratio {e / max(e_seq, R.FLOOR):.2f}")
    assert e <= b, f"{what}: err {e:.3e} > {R.F} x max(e_seq = {e_seq:.3e}, {R.FLOOR:.1e})"


def check_states(what, c, sx, sy, f64, refined=None):
    """As tests/test_gpu_sos_accuracy.py::check_states: float64 section values at their section's float64 bar; a float32-result
    launch of a cascade the float32 rule leaves unrefined is held to F times that rule where it is wider."""
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
        print(f"SOSHO state {what} section {s}: e_sec {c.e_sec[s]:.2e} err {max(ex, ey) / scale:.2e} "
              f"ratio {max(ex, ey) / scale / max(c.e_sec[s], R.FLOOR):.2f} bar {rel:.1e}")
        assert ey <= tol, f"{what}: state_y[{s}] off by {ey:.3e} > {tol:.3e}"
        assert ex <= tol, f"{what}: state_x[{s + 1}] off by {ex:.3e} > {tol:.3e}"


def run_three_dtypes(c, what, rows, length):
    E, sos = ext(), tsos(c.sos)
    info = handoff_info(c.sos, rows, length)
    y, sx, sy = E.sos_forward(dev(c.x), None, sos, None, None)
    check32(f"{what} f32->f32 ({info['nseg']} x {info['seg_len']}, {info['passes']} passes)", y, c.y)
    check_states(f"{what} f32->f32", c, sx, sy, f64=False)
    handoff_info(c.sos, rows, length, F32, F64)
    y, sx, sy = E.sos_forward(dev(c.x), None, sos, None, None, out_dtype=F64)
    check64(f"{what} f32->f64", y, c.y, c.e_seq)
    check_states(f"{what} f32->f64", c, sx, sy, f64=True)
    handoff_info(c.sos, rows, length, F64)
    y, sx, sy = E.sos_forward(dev(c.x, np.float64), None, sos, None, None)
    check64(f"{what} f64->f64", y, c.y, c.e_seq)
    check_states(f"{what} f64->f64", c, sx, sy, f64=True)


# ---- (1) the whole grid, 2 / 3 / 5 segments asked for (16 tiles of 4096: 2 x 8, 3 x 6 -> 6 6 4, 5 -> 4 x 4; 32 of 2048 for float64
#          signals: 5 -> 7 7 7 7 4) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [2, 3, 5])
@pytest.mark.parametrize("name,fs", R.GRID, ids=R.GRID_IDS)
def test_grid(name, fs, nseg, monkeypatch):
    c = R.case(name, fs)
    force(monkeypatch, nseg)
    run_three_dtypes(c, f"{name}@{fs} nseg {nseg}", R.ROWS, R.T)


# ---- (2) T = 65535: rows that do not start on 16 bytes take the dword path and its tile ----------------------------------------------
@pytest.mark.parametrize("nseg", [3, 5])
@pytest.mark.parametrize("fs", R.RATES)
@pytest.mark.parametrize("name", [R.HIGHPASS_20, "notch50_q30"])
def test_unaligned_rows(name, fs, nseg, monkeypatch):
    c = R.case(name, fs, R.ROWS, R.T - 1)
    force(monkeypatch, nseg)
    info = handoff_info(c.sos, R.ROWS, R.T - 1)
    assert info["seg_len"] % 2048 == 0 and (nseg != 5 or (info["nseg"], info["seg_len"]) == (5, 7 * 2048)), info      # 7 7 7 7 4 tiles of 2048
    run_three_dtypes(c, f"{name}@{fs} T={R.T - 1} nseg {nseg}", R.ROWS, R.T - 1)


# ---- (3) section taps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [3, 5])
@pytest.mark.parametrize("name", ["hp20_cheby1_4", "lp40_butter8"])
def test_section_taps(name, nseg, monkeypatch):
    fs = 192000
    c = R.case(name, fs)
    force(monkeypatch, nseg)
    for dtype in (np.float64, np.float32):
        td = F64 if dtype == np.float64 else F32
        handoff_info(c.sos, R.ROWS, R.T, td, F64, sections=True)
        y, sx, sy, sec = ext().sos_forward(dev(c.x, dtype), None, tsos(c.sos), None, None, out_dtype=F64, return_sections=True)
        sec = host(sec)
        for s in range(c.K):
            check64(f"{name}@{fs} {np.dtype(dtype).name} nseg {nseg} section {s}", sec[s], c.sec[s], c.e_sec[s])
        check64(f"{name}@{fs} {np.dtype(dtype).name} nseg {nseg} with sections", y, c.y, c.e_seq)
        assert np.array_equal(sec[-1], host(y))
        check_states(f"{name}@{fs} with sections", c, sx, sy, f64=True)


# ---- (4) carried state: the scan starts from the caller's state ---------------------------------------------------------------------
@pytest.mark.parametrize("name,fs", [(R.HIGHPASS_20, 48000), ("hp20_cheby1_4", 192000), ("notch50_q30", 96000), ("lp40_butter8", 192000),
                                     ("peak30_q8_12db", 192000)])
def test_carried_state(name, fs, monkeypatch):
    """The first 20 000 samples in one call, the rest in a hand-off call that takes the returned states: the concatenation is
    held to the one-shot bar."""
    c = R.case(name, fs)
    E, sos, n0 = ext(), tsos(c.sos), 20_000
    for f64 in (True, False):
        x = dev(c.x, np.float64 if f64 else np.float32)
        monkeypatch.setenv("TFX_SOS_HANDOFF", "0")
        ya, sx, sy = E.sos_forward(x[:, :n0].contiguous(), None, sos, None, None)
        force(monkeypatch, 3)
        handoff_info(c.sos, R.ROWS, R.T - n0, F64 if f64 else F32)
        yb, sx, sy = E.sos_forward(x[:, n0:].contiguous(), None, sos, sx, sy)
        y = torch.cat([ya, yb], dim=1)
        what = f"{name}@{fs} carried state at {n0}"
        if f64:
            check64(what + " f64", y, c.y, c.e_seq)
        else:
            check32(what + " f32", y, c.y)
        check_states(what, c, sx, sy, f64=f64)


# ---- (5) poles on and next to the unit circle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [0, 5])
def test_integrator(nseg, monkeypatch):
    """y = cumsum(x): no warm-up length exists.  The truth is a long double cumsum, e_seq the float64 cumsum's distance from it."""
    x = R.signal(2, R.T)
    truth = np.cumsum(x.astype(np.longdouble), axis=1)
    seq = np.cumsum(x.astype(np.float64), axis=1)
    scale = max(1.0, float(np.abs(truth).max()))
    e_seq = float(np.abs(seq - truth).max()) / scale
    assert ext().sos_plan_info(INTEGRATOR, refine=False)["warmup"] == -1
    if nseg:
        force(monkeypatch, nseg)
    info = handoff_info(INTEGRATOR, 2, R.T, F64)
    y, sx, sy = ext().sos_forward(dev(x, np.float64), None, tsos(INTEGRATOR), None, None)
    e = float(np.abs(host(y) - truth).max()) / scale
    es = float(np.abs(host(sy)[0] - truth[:, :-3:-1]).max()) / scale
    print(f"SOSHO integrator nseg {info['nseg']}: e_seq {e_seq:.2e} err {e:.2e} ratio {e / max(e_seq, R.FLOOR):.2f} state ratio {es / max(e_seq, R.FLOOR):.2f}")
    assert e <= R.bar(e_seq) and es <= R.bar(e_seq), (e, es, e_seq)
    assert np.array_equal(host(sx)[0], x[:, :-3:-1].astype(np.float64))


@pytest.mark.parametrize("nseg", [0, 5])
def test_leaky_integrator(nseg, monkeypatch):
    x = R.signal(2, R.T)
    c = R.Case(LEAKY, x)
    if nseg:
        force(monkeypatch, nseg)
    info = handoff_info(LEAKY, 2, R.T, F64)
    y, sx, sy = ext().sos_forward(dev(x, np.float64), None, tsos(LEAKY), None, None)
    check64(f"leaky integrator nseg {info['nseg']}", y, c.y, c.e_seq)
    check_states("leaky integrator", c, sx, sy, f64=True)


# ---- (6) the fused epilogue ---------------------------------------------------------------------------------------------------
def _planted(rows, T, index, seed=23):
    """Quiet noise (|x| <= 1e-3) with one impulse of 0.9 at `index` of the last row."""
    x = rnd((rows, T), seed) * np.float32(1e-3)
    x[-1, index] = 0.9
    return torch.from_numpy(x).to(DEV)


@pytest.mark.parametrize("nseg", [2, 3])
def test_epilogue_absmax_planted_at_the_seams(nseg, monkeypatch):
    """A cascade dominated by its direct tap puts the largest output where the impulse is: both sides of every seam, 0, T - 1."""
    E, T = ext(), 4 * 4096 + 1000
    force(monkeypatch, nseg)
    info = handoff_info(PLANT_SOS, 3, T)
    seams = [g * info["seg_len"] for g in range(1, info["nseg"])]
    assert seams and all(0 < s < T for s in seams)
    sos = tsos(PLANT_SOS)
    for index in sorted({0, T - 1} | {s - 1 for s in seams} | set(seams)):
        x = _planted(3, T, index)
        y0, _, _ = E.sos_forward(x, None, sos, None, None)
        assert int(y0.abs().argmax()) == 2 * T + index
        for per_row in (False, True):
            ep = E.Epilogue(gain=0.5, stat="absmax", per_row=per_row)
            y, _, _ = E.sos_forward(x, None, sos, None, None, epilogue=ep)
            assert torch.equal(y, E.gain_forward(y0, 0.5)), (index, per_row)
            view = y.double() if per_row else y.double().reshape(1, -1)
            ref = view.abs().max(dim=1).values
            assert ep.stat_value.dtype == F64 and torch.equal(ep.stat_value, ref), (index, per_row, ep.stat_value.tolist(), ref.tolist())
            assert float(ref[-1]) == float(y[-1, index].abs()) > 0.25


# ---- (7) non-finite samples -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_nonfinite_samples_stay_in_their_row_and_reach_its_end(dtype, bad, monkeypatch):
    c = R.case(R.HIGHPASS_20, 48000)
    E, sos = ext(), tsos(c.sos)
    force(monkeypatch, 3)
    info = handoff_info(c.sos, R.ROWS, R.T, F64 if dtype == np.float64 else F32)
    L, n = info["seg_len"], info["nseg"]
    clean, csx, csy = E.sos_forward(dev(c.x, dtype), None, sos, None, None)
    for at in (L - 1, L, ((n - 1) * L + R.T) // 2):
        x = np.array(c.x, dtype=dtype)
        x[1, at] = bad
        for ep in (None, E.Epilogue(gain=0.5, stat="absmax", per_row=True)):
            y, sx, sy = E.sos_forward(dev(x), None, sos, None, None, epilogue=ep)
            ref = clean if ep is None else E.gain_forward(clean, 0.5)
            assert torch.equal(y[0], ref[0]) and torch.equal(y[2], ref[2]), at
            assert torch.equal(y[1, :at], ref[1, :at]), at
            assert not torch.isfinite(y[1, at:]).any(), (at, int(torch.isfinite(y[1, at:]).sum()))
            assert not torch.isfinite(sy[:, 1]).any() and not torch.isfinite(sx[1:, 1]).any(), at
            assert torch.equal(sy[:, 0], csy[:, 0]) and torch.equal(sy[:, 2], csy[:, 2]) and torch.equal(sx[:, 0], csx[:, 0])
            if ep is not None:
                st = ep.stat_value
                assert not torch.isfinite(st[1]) and torch.equal(st[[0, 2]], ref[[0, 2]].double().abs().max(dim=1).values), (at, st.tolist())


# ---- (8) a row's bits depend on nothing but the row ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fs", [("hp20_cheby1_4", 192000), ("notch50_q30", 48000)])
def test_rows_alone_and_twice(name, fs, monkeypatch):
    c = R.case(name, fs)
    E, sos = ext(), tsos(c.sos)
    force(monkeypatch, 3)
    for dtype in (np.float32, np.float64):
        td = F64 if dtype == np.float64 else F32
        x = dev(c.x, dtype)
        handoff_info(c.sos, R.ROWS, R.T, td)
        y, sx, sy = E.sos_forward(x, None, sos, None, None)
        y2, sx2, sy2 = E.sos_forward(x, None, sos, None, None)
        assert torch.equal(y, y2) and torch.equal(sx, sx2) and torch.equal(sy, sy2)
        for r in range(R.ROWS):
            handoff_info(c.sos, 1, R.T, td)
            yr, sxr, syr = E.sos_forward(x[r:r + 1].contiguous(), None, sos, None, None)
            assert torch.equal(yr[0], y[r]) and torch.equal(sxr[:, 0], sx[:, r]) and torch.equal(syr[:, 0], sy[:, r]), (name, r)


# ---- (9) no knobs -------------------------------------------------------------------------------------------------------------
def test_automatic_route(monkeypatch):
    """The notch at 192 kHz has a warm-up of two million samples: rows of 65 536 hand off on their own.  The benign control
    reports what it reports with the route switched off, and computes the same bits."""
    E = ext()
    c = R.case("notch50_q30", 192000)
    info = handoff_info(c.sos, R.ROWS, R.T)
    assert info["passes"] == 3 and E.sos_plan_info(c.sos)["warmup"] > R.T, info
    run_three_dtypes(c, "notch50_q30@192000 automatic", R.ROWS, R.T)
    b = R.case("lp2k_butter4", 48000)
    auto = E.sos_route_info(b.sos, R.ROWS, R.T)
    y, sx, sy = E.sos_forward(dev(b.x), None, tsos(b.sos), None, None)
    monkeypatch.setenv("TFX_SOS_HANDOFF", "0")
    assert E.sos_route_info(b.sos, R.ROWS, R.T) == auto and auto["route"] == "halo", auto
    y0, sx0, sy0 = E.sos_forward(dev(b.x), None, tsos(b.sos), None, None)
    assert torch.equal(y, y0) and torch.equal(sx, sx0) and torch.equal(sy, sy0)
    check32("lp2k_butter4@48000 automatic", y, b.y)


def test_wave_explain_names_the_route():
    from torchfx_amd import Wave
    from torchfx_amd import filter as F
    x = torch.zeros(R.ROWS, R.T, device=DEV)
    hard, = (Wave(x, 192000, device=DEV) | F.Notch(50, q=30)).explain()
    info = ext().sos_route_info(_designed(F.Notch(50, q=30, fs=192000)), R.ROWS, R.T)
    assert info["route"] == "handoff", info
    assert hard == f"Notch: cascade handoff ({info['nseg']} segments of {info['seg_len']} samples per row, {info['passes']} passes over the signal)", hard
    easy, = (Wave(x, 48000, device=DEV) | F.LoButterworth(2000, order=4)).explain()
    assert easy.startswith("LoButterworth: cascade halo (") and easy.endswith("1 pass over the signal)"), easy


def _designed(f):
    f.compute_coefficients()
    return f._sos.detach().cpu().numpy()
