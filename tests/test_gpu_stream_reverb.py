"""StatefulFreeverb on the device inside StreamProcessor: chunks of 512 (shorter than every comb delay), eager and as a
replayed HIP graph, float32 and float64, against the one-shot reference of tests/reverb_reference.py within its measured
bound; the ring-out of flush(); reset_state() and a new stream."""
import numpy as np
import pytest
import torch

from tests import reverb_reference as R
from tests.gpu_common import DEV

pytestmark = pytest.mark.gpu

FS = 44100
TAIL = 300


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dt", [(torch.float32, np.float32), (torch.float64, np.float64)], ids=["f32", "f64"])
@pytest.mark.parametrize("width", [1.0, 0.3])
def test_stream_processor_chunks_match_the_one_shot_reference(width, dt, use_graph):
    from torchfx_amd.realtime import StatefulFreeverb, StreamProcessor

    tdt, ndt = dt
    x, ref, ref_state = R.freeverb_case((2, 6000), FS, width=width, tail=TAIL)
    t = torch.from_numpy(np.array(x)).to(tdt)
    eff = StatefulFreeverb(width=width, tail=TAIL / FS)
    proc = StreamProcessor([eff], chunk_size=512, device=DEV, use_graph=use_graph)
    got = proc.process_tensor(t, FS)
    assert (proc._graph is not None) == use_graph
    assert got.dtype == tdt and got.shape == t.shape and got.device.type == "cuda"
    R.check(got.cpu().numpy(), ref[:, :6000], f"stream width {width} {ndt.__name__} graph {use_graph}", ndt)
    assert eff._hist.dtype == torch.float64 and eff._hist.is_cuda and tuple(eff._hist.shape) == ref_state.shape
    ring = eff.flush()
    assert ring.shape == (2, TAIL) and ring.dtype == tdt
    R.check(ring.cpu().numpy(), ref[:, 6000:], f"ring-out width {width} {ndt.__name__} graph {use_graph}", ndt)
    R.check(np.concatenate([got.cpu().numpy(), ring.cpu().numpy()], -1), ref, "chunks then ring-out", ndt)
    assert eff._hist is None and eff.flush().numel() == 0


def test_state_after_the_stream_is_the_reference_lines():
    from torchfx_amd.realtime import StatefulFreeverb, StreamProcessor

    x, _, _ = R.freeverb_case((2, 6000), FS, tail=TAIL)
    comb, allpass = R.tunings(FS, 2)
    _, ref_state = R.freeverb_ref(x, comb, allpass, *R.freeverb_constants())
    eff = StatefulFreeverb()
    StreamProcessor([eff], chunk_size=512, device=DEV, use_graph=True).process_tensor(torch.from_numpy(np.array(x)).double(), FS)
    R.check(eff._hist.cpu().numpy(), ref_state, "state after a replayed stream")


def test_reset_state_and_a_new_stream_start_from_silence():
    from torchfx_amd import Freeverb
    from torchfx_amd.realtime import StatefulFreeverb

    eff = StatefulFreeverb(fs=FS)
    a = torch.from_numpy(np.array(R.signal((2, 1500), 21))).to(DEV)
    b = torch.from_numpy(np.array(R.signal((3, 2, 700), 22))).to(DEV)
    first = eff(a)
    assert torch.equal(first, Freeverb(fs=FS)(a))
    second = eff(a)
    assert not torch.equal(second, first)                               # the lines carried over
    eff.reset_state()
    assert eff._hist is None
    assert torch.equal(eff(a), first)
    assert torch.equal(eff(b), Freeverb(fs=FS)(b)) and eff._hist.shape[0] == 6      # another shape: a new stream
    assert eff(b[..., :0]).shape == (3, 2, 0)
