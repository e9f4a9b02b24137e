"""StatefulPhaser without a device: CPU chunks of sizes 1, 7 and 512 against the one-shot call (the coefficient track bit for bit,
the outputs within 16 E_REF of the long-double loop of tests/phaser_reference.py), inside StreamProcessor, the refusal of a plain
Phaser by both processors, and reset_state."""
import numpy as np
import pytest
import torch

from tests import phaser_reference as R

FS = 48000
KW = dict(rate=30.0, min_freq=200.0, max_freq=2000.0, stages=4, mix=0.5, spread=0.25)


def signal(shape, seed=0, dtype=np.float32):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_stateful_chunks_against_the_one_shot_call(dtype):
    from torchfx_amd import Phaser
    from torchfx_amd import realtime as RT
    from torchfx_amd.phaser import phase_shift_run

    x = torch.from_numpy(signal((2, 2600), 13)).to(dtype)
    P = Phaser(fs=FS, **KW).params(dtype)
    whole, coef, state, _ = phase_shift_run(x, P, 0, None, True)
    assert torch.equal(whole, Phaser(fs=FS, **KW)(x)) and not torch.equal(whole, 0.5 * x)
    yld, sld, e_ref = R.reference(x.double().numpy(), coef.numpy(), 4, 0.5, 0.5, 2)
    eff = RT.StatefulPhaser(fs=FS, **KW)
    for size in (1, 7, 512):                                            # the last chunk is ragged
        eff.reset_state()
        n = 2600 if size > 1 else 300
        cuts = list(range(0, n, size)) + [n]
        y = torch.cat([eff(x[:, a:b].contiguous()) for a, b in zip(cuts, cuts[1:])], -1)
        assert y.dtype == dtype and y.shape == (2, n)
        R.check(y.numpy(), yld[:, :n], e_ref, f"StatefulPhaser chunks of {size} {dtype}")
        assert eff._hist.shape == (2, 5) and eff._hist.dtype == torch.float64 and int(eff._pos) == n and eff._pos.dtype == torch.int64
        assert torch.equal(eff._hist[:, 0], x[:, n - 1].double())
        # the coefficient track of the chunks is the one-shot call's, bit for bit
        pos, cs = 0, []
        for a, b in zip(cuts, cuts[1:]):
            cs.append(phase_shift_run(x[:, a:b], P, a, None, True)[1])
        assert torch.equal(torch.cat(cs, -1), coef[:, :n])
    assert np.abs(eff._hist.numpy() - sld.astype(np.float64)).max() < 1e-13
    eff(x[:1, :10].contiguous())                                        # another row count: a new stream from position 0
    assert eff._hist.shape == (1, 5) and int(eff._pos) == 10
    eff.stages = 6                                                      # another stage count likewise
    eff(x[:1, :10].contiguous())
    assert eff._hist.shape == (1, 7) and int(eff._pos) == 10
    eff.reset_state()
    assert eff._hist is None and eff._pos is None


def test_reset_state_and_a_parameter_change():
    from torchfx_amd import Phaser, phase_shift
    from torchfx_amd import realtime as RT

    x = torch.from_numpy(signal((2, 900), 14, np.float64))
    eff = RT.StatefulPhaser(fs=FS, **KW)
    first = eff(x)
    again = eff(x)                                                      # the stream goes on: another position, another state
    assert not torch.equal(first, again) and int(eff._pos) == 1800
    state = eff._hist.clone()
    eff.rate, eff.mix = 40.0, 0.7                                       # applies from the next chunk on, state and position kept
    assert torch.equal(eff(x), phase_shift(x, FS, 4, 200.0, 2000.0, 40.0, 0.0, 1.0 - 0.7, 0.7, 0.25, position=1800, state=state))
    eff.reset_state()
    eff.rate, eff.mix = KW["rate"], KW["mix"]
    assert torch.equal(eff(x), first) and torch.equal(first, Phaser(fs=FS, **KW)(x))
    empty = eff(x[:, :0])                                               # an empty chunk moves nothing
    assert empty.shape == (2, 0) and int(eff._pos) == 900


def test_stream_processor_runs_the_stateful_phaser_over_cpu_chunks():
    from torchfx_amd import Phaser
    from torchfx_amd import realtime as RT

    x = torch.from_numpy(signal((2, 4000), 15))
    eff = RT.StatefulPhaser(**KW)
    y = RT.StreamProcessor([eff], chunk_size=512, device="cpu").process_tensor(x, FS)
    assert eff.fs == FS and y.shape == x.shape
    P = Phaser(fs=FS, **KW).params(torch.float32)
    from torchfx_amd.phaser import phase_shift_run

    _, coef, *_ = phase_shift_run(x, P, 0, None, True)
    yld, _, e_ref = R.reference(x.double().numpy(), coef.numpy(), 4, 0.5, 0.5, 2)
    R.check(y.numpy(), yld, e_ref, "StreamProcessor over CPU chunks")


def test_stream_processors_refuse_the_plain_effect():
    import torchfx_amd as f
    from torchfx_amd import realtime as RT

    class NoBackend(RT.AudioBackend):
        def open_stream(self, config, callback=None):
            raise AssertionError("the refusal comes before a stream is opened")

        def start(self):
            pass

        def stop(self):
            pass

        def close(self):
            pass

    with pytest.raises(TypeError, match="StatefulPhaser"):
        RT.StreamProcessor([f.Phaser()], chunk_size=256, device="cpu")
    with pytest.raises(TypeError, match="restart the sweep and the filter states"):
        RT.StreamProcessor([f.Gain(0.5), f.Phaser(), f.Gain(2.0)], chunk_size=256, device="cpu")
    with pytest.raises(TypeError, match="StatefulPhaser"):
        RT.RealtimeProcessor([f.Phaser()], NoBackend(), RT.StreamConfig(), device="cpu")
    RT.StreamProcessor([RT.StatefulPhaser()], chunk_size=256, device="cpu")
    RT.RealtimeProcessor([RT.StatefulPhaser()], NoBackend(), RT.StreamConfig(), device="cpu")
    assert RT._REFUSALS[-1].plain is f.Phaser and RT._REFUSALS[-1].stream is RT.StatefulPhaser
