"""StatefulChorus / StatefulFlanger / StatefulVibrato on the device inside StreamProcessor: chunk sizes 1, 7, 512 and tile + 1
(all below the history H = 1106 of a chorus; the flanger's 256 is above its H), eager and as a replayed HIP graph, float32 and
float64, against the one-shot effect on the whole signal on the device -- torch.equal, the stream is exact; the device position
counter; and the chain HiButterworth | StatefulChorus | StatefulLimiter against the staged one-shot chain."""
import numpy as np
import pytest
import torch

from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 48000


def tile():
    return ext().modulated_delay_plan_info(1, [(1.0, 0.0, 0.1, 0.0, 1.0)])["tile"]


def signal(shape, seed, dtype=torch.float32, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-scale, scale, shape)).to(dtype)


def chunk_cases():
    t = tile()
    return {1: 1300, 7: 7 * 200 + 3, 512: 512 * 9 + 100, t + 1: 3 * (t + 1) + 50}      # every length is past the chorus's delay


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["1", "7", "512", "tile+1"])
def test_stream_processor_chunks_equal_the_one_shot_call(case, dtype, use_graph):
    from torchfx_amd import Chorus
    from torchfx_amd.realtime import StatefulChorus, StreamProcessor

    B, n = list(chunk_cases().items())[case]
    x = signal((2, n), case, dtype)
    ref = Chorus(fs=FS)(x.to(DEV))
    assert not torch.equal(ref, 0.5 * x.to(DEV))                      # the wet part is at work
    eff = StatefulChorus()
    proc = StreamProcessor([eff], chunk_size=B, device=DEV, use_graph=use_graph)
    got = proc.process_tensor(x, FS)
    assert (proc._graph is not None) == use_graph
    H = eff.params(dtype).history
    assert H == 1106 and B < H                                        # every chunk is shorter than the history
    assert got.dtype == dtype and torch.equal(got, ref)
    assert eff._pos.dtype == torch.int64 and eff._pos.is_cuda and int(eff._pos) == n
    want = torch.cat([torch.zeros(2, H, dtype=dtype), x], -1)[:, n:]
    assert torch.equal(eff._hist.cpu(), want)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["Flanger", "Vibrato"])
def test_flanger_and_vibrato_streams(name, use_graph):
    import torchfx_amd as fx
    from torchfx_amd import realtime as RT

    x = signal((3, 2, 7 * 256 + 11), 5)
    ref = getattr(fx, name)(fs=FS, spread=0.25)(x.to(DEV)) if name == "Flanger" else getattr(fx, name)(fs=FS)(x.to(DEV))
    eff = getattr(RT, "Stateful" + name)(spread=0.25) if name == "Flanger" else getattr(RT, "Stateful" + name)()
    proc = RT.StreamProcessor([eff], chunk_size=256, device=DEV, use_graph=use_graph)
    got = proc.process_tensor(x, FS)
    assert (proc._graph is not None) == use_graph
    assert torch.equal(got, ref) and not torch.equal(ref, x.to(DEV)) and int(eff._pos) == x.shape[-1]


def test_a_new_stream_starts_from_silence_and_position_zero():
    from torchfx_amd import Chorus
    from torchfx_amd.realtime import StatefulChorus

    eff = StatefulChorus(fs=FS)
    a, b = signal((2, 700), 6).to(DEV), signal((3, 500), 7).to(DEV)
    eff(a)
    assert int(eff._pos) == 700
    assert torch.equal(eff(b), Chorus(fs=FS)(b)) and int(eff._pos) == 500 and eff._hist.shape == (3, 1106)      # another row count
    eff.reset_state()
    assert eff._hist is None and eff._pos is None
    first = eff(a[:, :300].contiguous())
    empty = eff(a[:, 300:300])                                        # an empty chunk moves nothing
    assert empty.shape == (2, 0) and int(eff._pos) == 300
    assert torch.equal(torch.cat([first, eff(a[:, 300:].contiguous())], -1), Chorus(fs=FS)(a))


def test_chain_with_filter_and_limiter_equals_the_staged_one_shot_chain():
    from torchfx_amd import Chorus, limit
    from torchfx_amd.filter import HiButterworth
    from torchfx_amd.realtime import StatefulChorus, StatefulLimiter, StreamProcessor

    B, n = 512, 512 * 12 + 100
    x = signal((2, n), 8, scale=1.3)
    hp = lambda: HiButterworth(200, order=2)                          # noqa: E731
    h = StreamProcessor([hp()], chunk_size=B, device=DEV).process_tensor(x, FS)           # what the chain hands the chorus
    c = Chorus(fs=FS)(h)
    ref = limit(c, FS)
    assert not torch.equal(h, x.to(DEV)) and not torch.equal(c, 0.5 * h) and not torch.equal(ref, c)      # every stage is at work
    for use_graph in (False, True):
        got_c = StreamProcessor([hp(), StatefulChorus()], chunk_size=B, device=DEV, use_graph=use_graph).process_tensor(x, FS)
        assert torch.equal(got_c, c)
        got = StreamProcessor([hp(), StatefulChorus(), StatefulLimiter()], chunk_size=B, device=DEV,
                              use_graph=use_graph).process_tensor(x, FS)
        assert got.shape == ref.shape and torch.equal(got, ref)
