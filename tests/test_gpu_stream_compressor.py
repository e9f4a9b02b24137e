"""StatefulCompressor on the device inside StreamProcessor: chunk sizes 1, 7, 512 and tile + 1, eager and as a replayed HIP
graph, against compress() on the whole signal and against the definition (tests/compressor_reference.py); and the chain HiButterworth | StatefulCompressor | StatefulLimiter against the
staged one-shot chain.  Chunks equal the one-shot call within the accuracy bound of tests/test_gpu_compressor.py, not bit for
bit: the scan's association follows the cut."""
import functools

import numpy as np
import pytest
import torch

from tests import compressor_reference as R
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 48000
KW = dict(threshold_db=-18.0, ratio=3.0)


def tile():
    return ext().compressor_plan_info(1, 1, 2)["tile"]


def bound(got, ref, dtype):
    """|got - ref| <= 2^-23 |ref| + 1e-11 max|ref| (float32: the rounding of the product) or 1e-11 max|ref| (float64)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    tol = (2.0 ** -23 * ref.abs() if dtype == torch.float32 else 0.0) + 1e-11 * float(ref.abs().max())
    worst = float(((got - ref).abs() - tol).max())
    print(f"largest excess over the bound: {worst:.3e} (<= 0 passes); largest deviation {float((got - ref).abs().max()):.3e}")
    assert got.shape == ref.shape and worst <= 0.0


def chunk_cases():
    t = tile()
    return {1: 300, 7: 7 * 60 + 3, 512: 512 * 9 + 100, t + 1: 3 * (t + 1) + 50}


def stream_signal(case, dtype):
    B, n = list(chunk_cases().items())[case]
    return B, torch.from_numpy(R.bursty(np.random.default_rng(case), (2, n), burst=n // 5, gap=n // 4)).to(dtype)


@functools.lru_cache(maxsize=None)
def definition(case, dtype):
    """``compress_ref`` (the per-sample float64 loop) on a case's whole signal, computed once for the eager and the graph run."""
    return R.compress_ref(stream_signal(case, dtype)[1].numpy(), FS, **KW)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["1", "7", "512", "tile+1"])
def test_stream_processor_chunks_equal_the_one_shot_call(case, dtype, use_graph):
    from torchfx_amd import compress
    from torchfx_amd.realtime import StatefulCompressor, StreamProcessor

    B, x = stream_signal(case, dtype)
    ref, g = compress(x.to(DEV), FS, return_gain=True, **KW)
    assert float(g.min()) < 0.7                                       # the compressor is at work
    comp = StatefulCompressor(**KW)
    proc = StreamProcessor([comp], chunk_size=B, device=DEV, use_graph=use_graph)
    got = proc.process_tensor(x, FS)
    assert (proc._graph is not None) == use_graph
    bound(got, ref, dtype)
    st = compress(x.to(DEV), FS, return_state=True, **KW)[1]
    assert comp._hist.shape == (1, 2) and float((comp._hist - st).abs().max()) <= 1e-10
    y_def, _, st_def = definition(case, dtype)                        # and with the definition itself, under the same bound
    bound(got, torch.from_numpy(y_def), dtype)
    assert float((comp._hist.cpu() - torch.from_numpy(st_def)).abs().max()) <= 1e-10


def test_chain_with_filter_and_limiter_equals_the_staged_one_shot_chain():
    from torchfx_amd import compress, limit
    from torchfx_amd.filter import HiButterworth
    from torchfx_amd.realtime import StatefulCompressor, StatefulLimiter, StreamProcessor

    B, n = 512, 512 * 12 + 100
    x = torch.from_numpy(R.bursty(np.random.default_rng(7), (2, n), loud=1.2, burst=700, gap=1300, dtype=np.float32))
    hp = lambda: HiButterworth(200, order=2)                          # noqa: E731
    h = StreamProcessor([hp()], chunk_size=B, device=DEV).process_tensor(x, FS)           # what the chain hands the compressor
    c = compress(h, FS, **KW)
    ref = limit(c, FS)
    assert not torch.equal(ref, c) and not torch.equal(c, h)          # both stages are at work
    for use_graph in (False, True):
        got_c = StreamProcessor([hp(), StatefulCompressor(**KW)], chunk_size=B, device=DEV, use_graph=use_graph).process_tensor(x, FS)
        bound(got_c, c, torch.float32)
        got = StreamProcessor([hp(), StatefulCompressor(**KW), StatefulLimiter()], chunk_size=B, device=DEV,
                              use_graph=use_graph).process_tensor(x, FS)
        assert torch.equal(got, limit(got_c, FS))                     # the limiter's stream is its one-shot call, bit for bit
        bound(got, ref, torch.float32)


def test_explain_and_route_name_the_native_kernel():
    from torchfx_amd import Compressor, Wave

    x = torch.zeros(2, 3 * tile() + 17)
    lines = (Wave(x, FS, device=DEV) | Compressor(**KW)).explain()
    assert lines == [f"Compressor: native (compressor_kernel, log-domain decoupled peak detector, 4 tile(s) of {tile()} per group in "
                     "4 segment(s); three launches)"]
