"""The route of the forward SOS cascade (csrc/sos_route.h), asked through tfx_sos_route_info for a given number of resident
wavefronts: no device is needed.  The halo plan's expected numbers are computed here from the formula the seam tests use
(tests/test_gpu_effects.py::_cascade_seams), not from the library."""
import numpy as np
import pytest
import torch

from tests import sos_reference as R
from torchfx_amd import torchfx_ext as E

SLOTS = 2048                       # 256 CUs x 2 workgroups x 4 wavefronts
ROWS, T = 64, 2_880_000
PLANT_SOS = np.array([[1.0, 0.05, 0.02, 1.0, -0.1, 0.05], [1.05, -0.08, 0.01, 1.0, 0.12, 0.04]])
INTEGRATOR = np.array([[1.0, 0, 0, 1, -1.0, 0]])
UNSTABLE = np.array([[1.0, 0, 0, 1, -2.1, 1.2]])
FS = 48000
HARD = {"notch50_q30": R.design("notch50_q30", FS), "hp20_cheby1_4": R.design("hp20_cheby1_4", FS), "integrator": INTEGRATOR}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    monkeypatch.delenv("TFX_SOS_NSEG", raising=False)
    monkeypatch.delenv("TFX_SOS_HANDOFF", raising=False)
    monkeypatch.delenv("TFX_SOS_VARIANT", raising=False)


def halo_plan(rows, length, plan_warm, tile=4096, slots=SLOTS, nseg=0):
    """Today's plan: halo = warm-up rounded to 256, one resident round of segments, segments of at least 8 halos."""
    cdiv = lambda a, b: -(-a // b)      # noqa: E731
    halo = (plan_warm + 255) & ~255
    target = nseg if nseg else slots // rows
    if plan_warm < 0 or target <= 1 or length <= halo:
        return 1, cdiv(length, tile) * tile, 0
    seg_tiles = cdiv(cdiv(length - halo, target) + halo, tile)
    if not nseg:
        seg_tiles = max(seg_tiles, cdiv(8 * halo, tile))
    stride = max(seg_tiles, 1) * tile - halo
    n = cdiv(length - halo, stride)
    return (n, stride, halo) if n > 1 else (1, cdiv(length, tile) * tile, 0)


def today(info):
    return info["nseg"], info["seg_len"], info["warmup"]


@pytest.mark.parametrize("sos,rows,length", [(R.design("lp2k_butter4", FS), ROWS, T), (PLANT_SOS, 3, 13_288)],
                         ids=["lp2k_butter4", "plant"])
def test_short_memory_cascades_keep_the_halo_plan(sos, rows, length):
    warm = E.sos_plan_info(sos, refine=False)["warmup"]
    info = E.sos_route_info(sos, rows, length, wave_slots=SLOTS)
    assert info["route"] == "halo" and info["passes"] == 1 and info["bytes_per_sample"] == 8.0, info
    assert today(info) == halo_plan(rows, length, warm), (info, halo_plan(rows, length, warm))


@pytest.mark.parametrize("name", sorted(HARD))
def test_long_memory_cascades_hand_off(name, monkeypatch):
    sos = HARD[name]
    warm = E.sos_plan_info(sos, refine=False)["warmup"]
    info = E.sos_route_info(sos, ROWS, T, wave_slots=SLOTS)
    assert info["route"] == "handoff", info
    assert 2 <= info["nseg"] and info["nseg"] * ROWS <= SLOTS, info
    assert info["seg_len"] % 4096 == 0 and info["warmup"] == 0, info                    # whole tiles of the shipping kernel
    assert (info["nseg"] - 1) * info["seg_len"] < T <= info["nseg"] * info["seg_len"], info
    refine = E.sos_plan_info(sos)["refine_f32"]
    assert info["passes"] == (3 if refine else 2) and info["bytes_per_sample"] == 4.0 * info["passes"] + 4.0, (info, refine)
    # float64 signals: the rare family's tile, refine_f64
    i64 = E.sos_route_info(sos, ROWS, T, torch.float64, wave_slots=SLOTS)
    assert i64["route"] == "handoff" and i64["seg_len"] % 2048 == 0, i64
    assert i64["passes"] == (3 if E.sos_plan_info(sos)["refine_f64"] else 2), i64
    # TFX_SOS_HANDOFF=0: today's plan
    monkeypatch.setenv("TFX_SOS_HANDOFF", "0")
    off = E.sos_route_info(sos, ROWS, T, wave_slots=SLOTS)
    assert off["route"] in ("sequential", "halo") and off["passes"] == 1 and today(off) == halo_plan(ROWS, T, warm), off
    monkeypatch.delenv("TFX_SOS_HANDOFF")
    # float32 arithmetic never hands off
    f32 = E.sos_route_info(sos, ROWS, T, precision="f32", wave_slots=SLOTS)
    assert f32["route"] != "handoff" and today(f32) == halo_plan(ROWS, T, warm, tile=2048), f32


@pytest.mark.parametrize("n", [2, 3, 5, 40])
def test_nseg_alone_never_hands_off(n, monkeypatch):
    monkeypatch.setenv("TFX_SOS_NSEG", str(n))
    for name, sos in list(HARD.items()) + [("lp2k_butter4", R.design("lp2k_butter4", FS))]:
        warm = E.sos_plan_info(sos, refine=False)["warmup"]
        info = E.sos_route_info(sos, ROWS, T, wave_slots=SLOTS)
        assert info["route"] != "handoff" and today(info) == halo_plan(ROWS, T, warm, nseg=n), (name, info)


@pytest.mark.parametrize("n", [0, 2, 3, 5])
def test_handoff_forced(n, monkeypatch):
    """TFX_SOS_HANDOFF=1: every eligible call, with TFX_SOS_NSEG segments (rounded to whole tiles) when that is set too."""
    monkeypatch.setenv("TFX_SOS_HANDOFF", "1")
    if n:
        monkeypatch.setenv("TFX_SOS_NSEG", str(n))
    for sos in (R.design("lp2k_butter4", FS), PLANT_SOS, HARD["notch50_q30"]):
        info = E.sos_route_info(sos, 3, 65_536, wave_slots=SLOTS)
        assert info["route"] == "handoff" and info["seg_len"] % 4096 == 0, info
        want = -(-16 // -(-16 // n)) if n else 65_536 // 8192
        assert info["nseg"] == want, (info, want)
    assert E.sos_route_info(HARD["notch50_q30"], 3, 65_536, precision="f32", wave_slots=SLOTS)["route"] != "handoff"
    assert E.sos_route_info(PLANT_SOS, 3, 4096, wave_slots=SLOTS)["route"] != "handoff"       # one tile: nothing to cut


def test_an_unstable_cascade_never_hands_off(monkeypatch):
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv("TFX_SOS_HANDOFF", knob)
        info = E.sos_route_info(UNSTABLE, ROWS, T, wave_slots=SLOTS)
        assert info["route"] == "sequential" and info["nseg"] == 1 and info["passes"] == 1, info


def test_many_sections_and_bad_arguments():
    many = np.tile(R.design("hp20_butter4", FS), (17, 1))            # 34 sections: past the route's limit
    assert E.sos_route_info(many, ROWS, T, wave_slots=SLOTS)["route"] != "handoff"
    with pytest.raises(RuntimeError, match="wave_slots"):
        E.sos_route_info(PLANT_SOS, 3, 1000, wave_slots=-1)
    with pytest.raises(RuntimeError):
        E.sos_route_info(PLANT_SOS, -3, 1000, wave_slots=SLOTS)
    assert E.sos_route_info(PLANT_SOS, 3, 0, wave_slots=SLOTS)["route"] == "sequential"
