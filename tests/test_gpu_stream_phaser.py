"""StatefulPhaser on the device: chunkings of sizes 1, 8, 513 and ragged over (2, 3 tile + 17) against the one-shot call -- the
coefficient track bit for bit, the outputs within 16 E_REF of the long-double loop fed that track (tests/phaser_reference.py), not
bit for bit: the scan's association follows the cut --, StreamProcessor eager and as a replayed HIP graph, a parameter change
mid-stream and a row-count change, which restarts the stream."""
import numpy as np
import pytest
import torch

from tests import phaser_reference as R
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 48000
KW = dict(rate=3.0, min_freq=200.0, max_freq=2000.0, stages=4, mix=0.5, spread=0.25)
DTYPES = {"f32": torch.float32, "f64": torch.float64}


def tile():
    return ext().phaser_plan_info(1, 1, 1, 1)["tile"]


def signal(shape, seed, dtype=torch.float32):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)).to(dtype)


def cuts(n, size):
    if size == "ragged":
        steps, out, k = [300, 1, 2049, 7, 1000, 64], [0], 0
        while out[-1] < n:
            out.append(min(n, out[-1] + steps[k % len(steps)]))
            k += 1
        return out
    return list(range(0, n, size)) + [n]


_ONE = {}


def one_shot(dt):
    """x, the one-shot call's (y, coef) on the device and the long-double reference fed that coef, once per dtype."""
    if dt not in _ONE:
        from torchfx_amd.effect import Phaser
        from torchfx_amd.phaser import phase_shift_run

        x = signal((2, 3 * tile() + 17), 3, DTYPES[dt])
        P = Phaser(fs=FS, **KW).params(DTYPES[dt])
        y, coef, st, _ = phase_shift_run(x.to(DEV), P, 0, None, True)
        yld, _, e_ref = R.reference(x.double().numpy(), coef.cpu().numpy(), P.stages, P.dry, P.wet, 2)
        R.check(y.cpu().numpy(), yld, e_ref, f"one-shot {dt}")
        _ONE[dt] = (x, P, y, coef, yld, e_ref)
    return _ONE[dt]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("size", [1, 8, 513, "ragged"])
def test_chunks_against_the_one_shot_call(size, dt):
    from torchfx_amd.phaser import phase_shift_run
    from torchfx_amd.realtime import StatefulPhaser

    x, P, y1, coef1, yld, e_ref = one_shot(dt)
    xd, n = x.to(DEV), x.shape[-1]
    edges = cuts(n, size)
    st, pos, ys, cs = None, torch.zeros(1, dtype=torch.int64, device=DEV), [], []
    for a, b in zip(edges[:-1], edges[1:]):
        y, c, st, pos = phase_shift_run(xd[:, a:b], P, 0, st, True, pos)
        ys.append(y)
        cs.append(c)
    assert int(pos) == n and torch.equal(torch.cat(cs, -1), coef1)
    got = torch.cat(ys, -1)
    R.check(got.cpu().numpy(), yld, e_ref, f"chunks of {size} {dt}")
    if size != 1:                                             # the class makes the same calls
        eff = StatefulPhaser(fs=FS, **KW)
        cls = torch.cat([eff(xd[:, a:b]) for a, b in zip(edges[:-1], edges[1:])], -1)
        assert torch.equal(cls, got) and int(eff._pos) == n and eff._pos.is_cuda and eff._hist.shape == (2, 5)
        assert eff._hist.dtype == torch.float64 and torch.equal(eff._hist, st)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_stream_processor_graph_against_eager(dt):
    from torchfx_amd.realtime import StatefulPhaser, StreamProcessor

    x = signal((2, 512 * 9 + 100), 4, DTYPES[dt])
    out = {}
    for use_graph in (False, True):
        eff = StatefulPhaser(**KW)
        proc = StreamProcessor([eff], chunk_size=512, device=DEV, use_graph=use_graph)
        out[use_graph] = proc.process_tensor(x, FS)
        assert (proc._graph is not None) == use_graph
        assert int(eff._pos) == x.shape[-1] and eff.fs == FS
    assert torch.equal(out[True], out[False])                  # the same launches on the same cut
    from torchfx_amd.effect import Phaser

    P = Phaser(fs=FS, **KW).params(DTYPES[dt])
    _, coef, *_ = ext().phaser_forward(x.to(DEV), P.stages, FS, P.rate, P.min_freq, P.max_freq, 0.0, P.spread, P.dry, P.wet, "sine",
                                       return_coef=True)
    yld, _, e_ref = R.reference(x.double().numpy(), coef.cpu().numpy(), P.stages, P.dry, P.wet, 2)
    R.check(out[True].cpu().numpy(), yld, e_ref, f"StreamProcessor graph {dt}")


def test_a_parameter_change_applies_from_the_next_chunk_on():
    from torchfx_amd.phaser import phase_shift
    from torchfx_amd.realtime import StatefulPhaser

    x = signal((2, 1500), 5, torch.float64).to(DEV)
    eff = StatefulPhaser(fs=FS, **KW)
    a = eff(x[:, :700])
    state, pos = eff._hist.clone(), int(eff._pos)
    eff.rate, eff.max_freq, eff.mix = 5.0, 3000.0, 0.8
    b = eff(x[:, 700:])
    assert pos == 700 and int(eff._pos) == 1500
    want = phase_shift(x[:, 700:], FS, 4, 200.0, 3000.0, 5.0, 0.0, 1.0 - 0.8, 0.8, 0.25, position=700, state=state)
    assert torch.equal(b, want)                                # the sections' states and the position carried over
    assert torch.equal(a, phase_shift(x[:, :700], FS, 4, 200.0, 2000.0, 3.0, 0.0, 0.5, 0.5, 0.25))


def test_a_row_count_or_stage_change_restarts_the_stream():
    from torchfx_amd import Phaser
    from torchfx_amd.realtime import StatefulPhaser

    eff = StatefulPhaser(fs=FS, **KW)
    a, b = signal((2, 700), 6).to(DEV), signal((3, 500), 7).to(DEV)
    eff(a)
    assert int(eff._pos) == 700 and eff._hist.shape == (2, 5)
    assert torch.equal(eff(b), Phaser(fs=FS, **KW)(b)) and int(eff._pos) == 500 and eff._hist.shape == (3, 5)
    eff.stages = 6
    assert torch.equal(eff(b), Phaser(fs=FS, **dict(KW, stages=6))(b)) and int(eff._pos) == 500 and eff._hist.shape == (3, 7)
    eff.reset_state()
    assert eff._hist is None and eff._pos is None
    first = eff(a[:, :300].contiguous())
    empty = eff(a[:, 300:300])                                 # an empty chunk moves nothing
    assert empty.shape == (2, 0) and int(eff._pos) == 300
    rest = eff(a[:, 300:].contiguous())
    whole = Phaser(fs=FS, **dict(KW, stages=6))(a)
    assert torch.allclose(torch.cat([first, rest], -1), whole, rtol=0, atol=2e-7)


def test_zz_report():
    for name, ratio in sorted(R.RATIOS.items()):
        print(f"phaser streams on the device, {name}: largest deviation / bound {ratio:.3f}")
    assert all(r <= 1.0 for r in R.RATIOS.values())
