"""The one-launch Delay (csrc/delay.hip) on the device against the reference's composition run by torch on the same device
(MonoDelayStrategy / PingPongDelayStrategy.apply_delay, zero pad, torch.lerp -- tests/test_delay_host.py checks that
composition against the reference bit for bit on the CPU).  Bar: bit-identical is expected; the asserted bound is
2^-22 (float32) / 1e-15 (float64) of 1 + max|ref|."""
import numpy as np
import pytest
import torch

from tests.gpu_common import DEV, dev, ext

pytestmark = pytest.mark.gpu


def composition(x, D, taps, feedback, mix, pingpong):
    from torchfx_amd.effect import MonoDelayStrategy, PingPongDelayStrategy
    strat = PingPongDelayStrategy() if pingpong else MonoDelayStrategy()
    delayed = strat.apply_delay(x, D, taps, feedback)
    if x.size(-1) < delayed.size(-1):
        pad = torch.zeros(*x.shape[:-1], delayed.size(-1), dtype=x.dtype, device=x.device)
        pad[..., :x.size(-1)] = x
        x = pad
    return torch.lerp(x, delayed, mix)


def check(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if torch.equal(got, ref):
        return True
    tol = (2.0 ** -22 if ref.dtype == torch.float32 else 1e-15) * (1 + float(ref.abs().max()))
    err = float((got.double() - ref.double()).abs().max())
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"
    return False


SHAPES = {"1d": (4099,), "2d": (3, 4099), "b2t": (2, 2, 4099), "b3t": (2, 3, 4099)}
DT = [(0, 3), (1, 5), (37, 4), (300, 16), (12000, 8), (3, 5000)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("pingpong", [False, True])
@pytest.mark.parametrize("D,taps", DT)
def test_parity_grid(dtype, shape, pingpong, D, taps):
    g = torch.Generator().manual_seed(D * 7 + taps)
    x = (torch.rand(SHAPES[shape], generator=g, dtype=torch.float64) * 2 - 1).to(dtype).to(DEV)
    fb, mix = 0.7, (0.3 if taps % 2 else 0.65)          # both lerp branches
    y = ext().delay_forward(x, D, taps, fb, mix, pingpong)
    check(y, composition(x, D, taps, fb, mix, pingpong), f"{dtype} {shape} pp={pingpong} D={D} taps={taps}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("pingpong", [False, True])
def test_parity_edges(dtype, pingpong):
    E = ext()
    g = torch.Generator().manual_seed(5)
    base = (torch.rand(2, 20011, generator=g, dtype=torch.float64) * 2 - 1).to(dtype).to(DEV)
    cases = {
        "T <= D": (base[:, :300].contiguous(), 1000, 3),
        "T == D": (base[:, :1000].contiguous(), 1000, 2),
        "T odd": (base[:, :20011], 37, 4),
        "offset 3 view": (base.reshape(-1)[3:3 + 2 * 9001].view(2, 9001), 2000, 3),
        "non-contiguous": (base[:, ::2], 300, 5),
        "transposed pair": (base[:, :4000].t().contiguous().t(), 12000, 2),
        "lattice tail": (base[:, :20011], 4097, 8),
        "> 64 taps": (base[:, :3000], 20, 70),
    }
    for what, (x, D, taps) in cases.items():
        for mix in (0.2, 0.5, 1.0, 0.0):
            y = E.delay_forward(x, D, taps, 0.9, mix, pingpong)
            check(y, composition(x, D, taps, 0.9, mix, pingpong), f"{what} mix={mix}")
    x1 = base[0, 3:3 + 8191]                                   # 1-D view at element offset 3
    check(E.delay_forward(x1, 12000, 3, 0.5, 0.4, False), composition(x1, 12000, 3, 0.5, 0.4, False), "1-d offset view")


@pytest.mark.parametrize("D,taps", [(37, 4), (12000, 3), (3, 70)])
def test_nan_inf_reach_only_their_taps(D, taps):
    x = torch.zeros(2, 30000, device=DEV)
    x += torch.linspace(-0.5, 0.5, 30000, device=DEV)
    j, k = 1234, 20000
    x[0, j] = float("nan")
    x[1, k] = float("inf")
    for pp in (False, True):
        y = ext().delay_forward(x, D, taps, 0.5, 0.3, pp)
        ref = composition(x, D, taps, 0.5, 0.3, pp)
        assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.isinf(y), torch.isinf(ref))
        fin = torch.isfinite(ref)
        check(torch.where(fin, y, 0), torch.where(fin, ref, 0), f"finite part D={D} pp={pp}")
        bad = (~torch.isfinite(y)).nonzero().tolist()
        want = set()
        for r, n0 in ((0, j), (1, k)):
            want.add((r, n0))
            for i in range(1, taps + 1):
                dst = (1 - r if (i % 2 == 1) == (r == 0) else None) if pp else r
                if dst is not None and n0 + i * D < y.shape[1]:
                    want.add((dst, n0 + i * D))
        assert {tuple(b) for b in bad} == want, (D, pp)


def test_golden_fixture(golden):
    from tests.test_delay_host import golden_delay
    g = golden("delay_fx")
    names = sorted({k.split("/")[0] for k in g.files})
    for name in names:
        x, y, d = golden_delay(g, name)
        got = d(dev(x))
        assert d.native_refusal(dev(x)) is None
        check(got, torch.from_numpy(y).to(DEV), name)


def _tails():
    from torchfx_amd import effect as E
    return {"gain": lambda: [E.Gain(0.7)], "gain clamp": lambda: [E.Gain(2.5, clamp=True)],
            "clamp peak": lambda: [E.Gain(2.5, clamp=True), E.Normalize(0.9)],
            "rms": lambda: [E.Normalize(0.5, E.RMSNormalizationStrategy())],
            "gain per_channel": lambda: [E.Gain(1.3), E.Normalize(0.8, E.PerChannelNormalizationStrategy())]}


@pytest.mark.parametrize("tail", list(_tails()))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("D,taps,pp", [(12000, 3, False), (37, 4, True), (3, 70, False)])
def test_epilogue_equals_staged_passes(tail, dtype, D, taps, pp):
    """Delay | Gain | Normalize as the Delay's launch with an epilogue (+ one apply pass) against the same modules staged:
    bit-identical for gain, clamp and the max|y| statistics; the RMS statistic is summed in another order (1e-6 / 1e-13)."""
    import torchfx_amd as fx
    from torchfx_amd.effect import PingPongDelayStrategy
    x = (torch.rand(2, 2, 25001, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 1.8 - 0.9).to(dtype).to(DEV)
    outs = []
    for ep in (False, True):
        w = fx.Wave(x, 48000, device=DEV)
        w.fuse_epilogue = ep
        w = w | fx.Delay(delay_samples=D, taps=taps, feedback=0.8, mix=0.6, strategy=PingPongDelayStrategy() if pp else None)
        for m in _tails()[tail]():
            w = w | m
        if ep:
            assert [type(m).__name__ for m in w.plan()] == ["Epilogued"]
            assert w.explain()[0].startswith("Epilogued[Delay]: native (")
        outs.append(w.ys)
    staged, fused = outs
    assert fused.dtype == staged.dtype and fused.shape == staged.shape
    if tail == "rms":
        tol = 1e-6 if dtype == torch.float32 else 1e-13
        assert float((fused.double() - staged.double()).abs().max()) <= tol * max(1.0, float(staged.abs().max()))
    else:
        assert torch.equal(fused, staged), tail


def test_one_launch_and_hip_graph():
    E = ext()
    x = torch.rand(4, 50000, device=DEV) - 0.5
    for D, taps in ((12000, 8), (37, 4)):
        E.delay_forward(x, D, taps, 0.5, 0.3, False)           # warm: nothing to upload (taps <= 64)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y = E.delay_forward(x, D, taps, 0.5, 0.3, False)
        torch.cuda.current_stream().wait_stream(s)
        for seed in (1, 2):
            x.copy_(torch.rand(4, 50000, generator=torch.Generator().manual_seed(seed)).to(DEV) - 0.5)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, E.delay_forward(x, D, taps, 0.5, 0.3, False)), (D, seed)


def test_explain_routes():
    import torchfx_amd as fx
    from torchfx_amd.effect import PingPongDelayStrategy
    w = fx.Wave(torch.zeros(2, 1000, device=DEV), 48000, device=DEV)
    assert (w | fx.Delay(delay_samples=12000)).explain() == ["Delay: native (lattice)"]
    assert (w | fx.Delay(delay_samples=37, taps=4, strategy=PingPongDelayStrategy())).explain() == ["Delay: native (span)"]
    assert (w | fx.Delay(bpm=120, delay_time="1/8")).explain() == ["Delay: native (lattice)"]
    w16 = fx.Wave(torch.zeros(2, 1000, device=DEV, dtype=torch.float16), 48000, device=DEV)
    assert (w16 | fx.Delay(delay_samples=5)).explain() == ["Delay: torch composition -- torch.float16 signal"]
    y = (w16 | fx.Delay(delay_samples=5)).ys
    assert y.shape == (2, 1015) and y.dtype == torch.float16


@pytest.mark.parametrize("pp", [False, True])
def test_full_size(pp):
    """64 rows x 60 s at 48 kHz (bpm=120, "1/8": D = 12000, 8 taps), mono; or 32 stereo pairs ping-pong."""
    import torchfx_amd as fx
    from torchfx_amd.effect import PingPongDelayStrategy
    T = 60 * 48000
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.rand((32, 2, T) if pp else (64, T), generator=g, device=DEV) * 2 - 1
    d = fx.Delay(bpm=120, delay_time="1/8", fs=48000, taps=8, feedback=0.6, mix=0.35,
                 strategy=PingPongDelayStrategy() if pp else None)
    assert d.delay_samples == 12000
    y = d(x)
    ref = composition(x, 12000, 8, 0.6, 0.35, pp)
    check(y, ref, f"full size pp={pp}")
