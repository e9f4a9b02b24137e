"""Writes tests/golden/delay_fx.npz: the reference's BPM-synced multi-tap ``Delay`` (``torchfx.effect.Delay``, mono and
ping-pong strategies) on the CPU, run by the reference itself.  Needs the reference's extension that ``build()`` compiles
into ``oracle/_ref``; loads it through ``oracle.make_golden.import_reference`` and changes nothing there.

Every case stores ``<name>/x``, ``<name>/y`` and ``<name>/params`` (float64: delay_samples as the effect resolved it, taps,
feedback, mix, pingpong, fs or 0, bpm or 0) plus ``<name>/delay_time`` (the note value string, "" when the delay was
given in samples)."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "delay_fx.npz")

# name: (shape, dtype, seed, kwargs of Delay, pingpong)
CASES = {
    "mono_1d_f32": ((400,), "float32", 1, dict(delay_samples=150, taps=3, feedback=0.4, mix=0.3), False),
    "mono_2d_f64": ((3, 120), "float64", 2, dict(delay_samples=37, taps=4, feedback=0.5, mix=0.6), False),
    "mono_b3t_f32": ((2, 3, 200), "float32", 3, dict(delay_samples=70, taps=3, feedback=0.3, mix=0.2), False),
    "pingpong_2d_f32": ((2, 300), "float32", 4, dict(delay_samples=60, taps=5, feedback=0.6, mix=0.5), True),
    "pingpong_b2t_f64": ((2, 2, 100), "float64", 5, dict(delay_samples=53, taps=4, feedback=0.7, mix=0.8), True),
    "pingpong_b3t_f32": ((2, 3, 150), "float32", 6, dict(delay_samples=77, taps=3, feedback=0.5, mix=0.4), True),
    "short_t_le_d_f32": ((2, 100), "float32", 7, dict(delay_samples=1500, taps=3, feedback=0.5, mix=0.5), False),
    "bpm_dotted_f32": ((2, 200), "float32", 8, dict(bpm=140, delay_time="1/16d", fs=1000, taps=3, feedback=0.45, mix=0.35), False),
    "bpm_triplet_pp_f64": ((2, 150), "float64", 9, dict(bpm=128, delay_time="1/8t", fs=1000, taps=4, feedback=0.3, mix=0.25), True),
    "bpm_zero_delay_f32": ((2, 300), "float32", 10, dict(bpm=120, delay_time="1/1024", fs=100, taps=3, feedback=0.5, mix=0.5), False),
    "taps1_f32": ((2, 300), "float32", 11, dict(delay_samples=200, taps=1, feedback=0.9, mix=1.0), False),
    "taps70_f64": ((2, 150), "float64", 12, dict(delay_samples=5, taps=70, feedback=0.95, mix=0.7), False),
    "taps70_pp_f32": ((2, 200), "float32", 13, dict(delay_samples=3, taps=70, feedback=0.9, mix=0.45), True),
}


def main() -> None:
    sys.path.insert(0, ROOT)
    import torch

    from oracle.make_golden import import_reference

    import_reference()
    from torchfx.effect import Delay, PingPongDelayStrategy

    out: dict[str, np.ndarray] = {}
    for name, (shape, dt, seed, kw, pp) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        x = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).to(getattr(torch, dt))
        d = Delay(**kw, strategy=PingPongDelayStrategy() if pp else None)
        y = d(x)
        out[f"{name}/x"] = x.numpy()
        out[f"{name}/y"] = y.numpy()
        out[f"{name}/params"] = np.array([d.delay_samples, d.taps, d.feedback, d.mix, float(pp), kw.get("fs") or 0,
                                          kw.get("bpm") or 0], dtype=np.float64)
        out[f"{name}/delay_time"] = np.array(kw.get("delay_time", "") if "bpm" in kw else "")
        print(f"{name:22s} x {tuple(x.shape)} {dt} D={d.delay_samples} taps={d.taps} -> {tuple(y.shape)}")
    assert out["bpm_zero_delay_f32/params"][0] == 0
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
