"""The cases of tests/spectral_cases.py without a GPU: the plan queries give the geometries that tests/test_gpu_istft_edges.py and
tests/test_gpu_stft_edges.py assume, the asymmetric-window inputs tell a reversed, a reversed-before-padding and a late-by-one
window from the right one by at least 100x the bound while the CPU float32 torch.istft stays below 0.05 of it, the one-tap
identities hold for the CPU torch.istft (so the claim "the tap sits at sample 127" is torch's, not the kernel's), torch raises
and passes where the flag tests expect the device to, and every exact probe expects representable values."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests import istft_reference as IR
from tests import spectral_cases as C
from tests import stft_reference as SR
from tests.test_gpu_istft import RDT, plan, three_tiles


def ext():
    from torchfx_amd import torchfx_ext
    return torchfx_ext


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


# ---- the geometries ---------------------------------------------------------------------------------------------------------
def test_the_plans_give_the_geometries_the_gpu_tests_assume():
    for dt in C.DTS:
        p = plan(C.TAP_N, 1, C.tap_frames(dt), dt, 1)                                # one tap, hop 1
        assert p["tile"] == 2048 and p["frames_per_batch"] == (32 if dt == "f32" else 16) and p["workgroups"] == 3
        assert C.tap_frames(dt) == 4098 and p["length"] == 4097
        assert (p["tile"] + C.TAP_N) % p["frames_per_batch"] == 0                  # a middle tile takes in whole batches: 72 of 32
        for c in C.A_CASES + C.F_CASES:
            frames = C.placed_frames(c, dt)
            p = plan(c.n, c.hop, frames, dt, c.wl)
            assert p["route"] == "lds" and p["workgroups"] == 3
            if c.wl < c.n:                                                         # the odd split and a tile off the hop's grid
                assert (c.n - c.wl) // 2 == 27 and c.n - c.wl - 27 == 28 and p["tile"] % c.hop != 0, (c, p)
        for n in (256, 4096):
            for hop in (n, n // 2):
                frames, G, tile, at = C.lone_geometry(n, hop, dt)
                assert plan(n, hop, frames, dt, center=False)["workgroups"] >= 3 and len(at) >= 3
    assert plan(256, 50, 8, "f32", 201)["tile"] == 1792
    p = plan(4096, 1024, three_tiles(4096, 1024, "f64"), "f64", center=False)       # float64 at 4096: every frame straddles a seam
    assert p["tile"] == 4096 and p["frames_per_batch"] == 1 and p["length"] == 9 * 1024 + 4096 and p["workgroups"] == 4
    assert C.lone_geometry(4096, 4096, "f64")[1:3] == (1, 4096)


def test_the_forward_cases_take_the_kernel():
    E = ext()
    for dt in C.DTS:
        for n in C.APART_SIZES:
            for hop in C.short_hops(n):
                for T in C.short_rows(n):
                    p = E.stft_plan_info(n, hop, n, T, 3, RDT[dt], True, "constant")
                    assert p["route"] == "lds" and p["frames"] == 1 + T // hop, (n, hop, T, p)
                    if T <= n // 2:                                                  # too short to reflect: only zeros can pad it
                        with pytest.raises(RuntimeError, match="does not fit"):
                            E.stft_plan_info(n, hop, n, T, 3, RDT[dt], True, "reflect")
            for hop in C.apart_hops(n):
                G, Tc, Tu = C.apart_lengths(n, hop, dt)
                for T, center in ((Tc, True), (Tu, False)):
                    p = E.stft_plan_info(n, hop, n, T, 3, RDT[dt], center, "reflect")
                    assert p["route"] == "lds" and p["frames"] == 2 * G + 1 and p["workgroups"] == 9 and T <= 55000, (n, hop, p)
        for n in C.NOTHING_TO_PAD_SIZES:
            for mode in C.NOTHING_TO_PAD:
                assert E.stft_plan_info(n, n // 4, n, 10 * n, 2, RDT[dt], False, mode)["route"] == "lds"
            assert E.stft_plan_info(n, n // 4, n, 10 * n, 2, RDT[dt], True, "replicate")["route"] == "torch"


# ---- A: the inputs tell a wrong window from the right one ---------------------------------------------------------------
@pytest.mark.parametrize("dt", C.DTS)
@pytest.mark.parametrize("c", C.A_CASES, ids=C.placed_id)
def test_wrong_windows_miss_the_bound_by_100x_and_cpu_torch_has_headroom(c, dt):
    y, b = C.placed_reference(c, dt)
    assert (b > 0).all() and np.isfinite(y).all()
    wrong = C.wrong_windows(c, dt)
    for how, w in wrong.items():
        if c.wl == c.n and how == "short reversed":                              # nothing to pad: the same mistake as "reversed"
            assert np.array_equal(w, wrong["reversed"])
            continue
        assert not np.array_equal(w, C.full(C.placed_window(c, dt), c.n))
        yw, _ = C.placed_reference(c, dt, w)
        miss = float((np.abs(yw - y) / b).max())
        print(f"{C.placed_id(c)} {dt} {how}: misses the bound by {miss:.3e}x")
        assert miss >= 100.0
    if dt == "f32":
        X = C.placed_input(c, dt)
        cpu = torch.istft(X, c.n, c.hop, c.wl, torch.from_numpy(C.placed_window(c, dt)), True, c.normalized).numpy()
        frac, _ = IR.within(cpu, y, b, f"CPU float32 torch.istft, {C.placed_id(c)}")
        assert frac <= 0.05


# ---- B: one tap at hop 1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", C.DTS)
def test_cpu_torch_places_the_single_tap_at_sample_127(dt):
    n, X = C.TAP_N, C.tap_input(dt)
    F = X.shape[-1]
    s = IR.exact_frames(X.numpy(), n)                                               # [rows, F, n] float64
    frame_bound = 8 * SR.U[np.dtype(C.NP[dt])] * (math.log2(n) + 2) * np.linalg.norm(s, axis=-1)
    frames = torch.istft(X, n, n, center=False).numpy()
    assert frames.shape == (2, F * n)
    assert (np.abs(frames.reshape(2, F, n) - s) <= frame_bound[..., None]).all()    # hop = n: the frames side by side
    want = C.tap_expected(frames)
    assert want.shape == (2, F - 1) and C.scales_exactly(want) and np.abs(want).min() > 0
    tol = 2 * frame_bound[:, 1:] + 4 * np.finfo(C.NP[dt]).eps * np.abs(want)           # two transforms of the frame, the scalings
    for tap, factor in C.TAPS:
        y = torch.istft(X, n, 1, 1, torch.tensor([tap], dtype=RDT[dt])).numpy()
        assert y.shape == want.shape and (np.abs(y - factor * want.astype(np.float64)) <= tol).all(), tap
        for off in (-1, 1):                                                        # the neighbouring samples are other values
            other = s[:, 1:, C.TAP_AT + off] * factor
            assert (np.abs(y - other) > tol).mean() > 0.99
        assert float(C.NP[dt](tap) ** 2) == tap * tap
    y, b = IR.reference(X.numpy(), n, 1, n // 2, np.ones(1), 1)                     # the reference indexes as torch does
    assert np.array_equal(y, s[:, 1:, C.TAP_AT])


# ---- C: a lone frame ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", C.DTS)
@pytest.mark.parametrize("n", [256, 4096])
def test_lone_frame_probes_expect_representable_values(n, dt):
    blocks = C.lone_blocks(n, dt)
    for hop in (n, n // 2):
        frames, G, tile, at = C.lone_geometry(n, hop, dt)
        for f in at:
            cover = C.lone_cover(n, hop, frames, f)
            assert set(np.unique(cover)) <= {1.0, 2.0}
            if hop == n:
                assert (cover == 1).all()
            else:
                assert (cover[:hop] == (1 if f == 0 else 2)).all() and (cover[hop:] == (1 if f == frames - 1 else 2)).all()
    X = torch.zeros(2, n // 2 + 1, 3, dtype=blocks.dtype)
    X[:, :, 1] = blocks
    y = torch.istft(X, n, n, center=False).numpy()
    block = y[:, n:2 * n]
    assert C.scales_exactly(block) and (block != 0).all() and (y[:, :n] == 0).all() and (y[:, 2 * n:] == 0).all()


# ---- D: where torch raises ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", C.DTS)
@pytest.mark.parametrize("n", [256, 4096])
def test_cpu_torch_raises_at_the_natural_length_of_a_falling_ramp_and_passes_one_short_of_it(n, dt):
    hop = n // 4
    frames = three_tiles(n, hop, dt)
    X = C.bins(n, frames, 2, dt, 4)
    w = torch.from_numpy(C.falling(n)).to(RDT[dt])
    assert float(w[-1]) == 0 and float(w[0]) > 0 and np.array_equal(w.double().numpy(), C.falling(n))
    natural = IR.natural_length(frames, n, hop, 0)
    with pytest.raises(RuntimeError, match="window overlap add min"):
        torch.istft(X, n, hop, window=w, center=False)
    y = torch.istft(X, n, hop, window=w, center=False, length=natural - 1)
    ref, b = IR.reference(X.numpy(), n, hop, 0, C.falling(n), length=natural - 1)
    assert y.shape == (2, natural - 1) and (b > 0).all()
    IR.within(y.numpy(), ref, b, f"CPU torch.istft {dt} {n}, falling ramp, one short of the natural length", 1.0 if dt == "f32" else 2.0)


def test_cpu_torch_passes_a_constant_window_of_1e_5_and_raises_at_1e_6():
    for n, hop, center in C.NEAR_GEOMETRIES:
        frames = three_tiles(n, hop, "f32")
        X = C.bins(n, frames, 2, "f32", 5)
        for value, passes in C.NEAR:
            env = C.near_envelope(value, n, hop)
            assert (env > 1e-11) == passes and not 0.5e-11 < env < 2e-11, (value, env)   # 1e-10, 4e-10; 1e-12, 4e-12: no rounding decides
            w = torch.full((n,), value, dtype=torch.float32)
            if passes:
                y = torch.istft(X, n, hop, window=w, center=center)
                ref, b = IR.reference(X.numpy(), n, hop, n // 2 if center else 0, w.numpy())
                IR.within(y.numpy(), ref, b, f"CPU torch.istft, constant window {value}, hop {hop}")
            else:
                with pytest.raises(RuntimeError, match="window overlap add min"):
                    torch.istft(X, n, hop, window=w, center=center)
