"""StatefulGate on the device inside StreamProcessor: chunk sizes 1, 7, 512 and tile + 1, eager and as a replayed HIP graph,
against gate() on the whole signal and against the definition (tests/gate_reference.py): the decision -- seen through the end
state's (open, c) and through the one-shot call's open track -- is exact, the outputs stay within gate_reference.within's
bound, not bit for bit: the scan's association follows the cut.  And the chain StatefulGate | StatefulCompressor against the
staged one-shot chain, and what Wave.explain() says on the device."""
import functools

import numpy as np
import pytest
import torch

from tests import gate_reference as R
from tests.gpu_common import DEV, ext

pytestmark = pytest.mark.gpu

FS = 48000
KW = dict(threshold_db=-30.0, hysteresis_db=4.0, range_db=24.0, attack=0.5e-3, hold=1e-3, release=5e-3)


def tile():
    return ext().gate_plan_info(1, 1, 2)["tile"]


def chunk_cases():
    t = tile()
    return {1: 300, 7: 7 * 60 + 3, 512: 512 * 9 + 100, t + 1: 3 * (t + 1) + 50}


def stream_signal(case, dtype):
    """Phrases with quiet stretches of H - 1, H, H + 1 and 3 H samples (H = 48), the first ones inside the first chunks."""
    B, n = list(chunk_cases().items())[case]
    K = R.constants(FS, **KW)
    H = K["H"]
    runs = [(20, H - 1), (90, H), (160, H + 1), (230, 60)] + [(k, 3 * H) for k in range(400, n, 700)]
    x = R.phrases(np.random.default_rng(case), (2, n), K, runs, np.float64)
    return B, K, torch.from_numpy(x).to(dtype)


@functools.lru_cache(maxsize=None)
def definition(case, dtype):
    """``gate_ref`` (the per-sample loop) on a case's whole signal, computed once for the eager and the graph run."""
    _, K, x = stream_signal(case, dtype)
    return R.gate_ref(x.numpy(), K)


def bounded(y, ref, x, K):
    """|y - g_ld x| <= (b + eps |g_ld|) |x| with eps the rounding of the product in y's dtype."""
    y, x = y.cpu().numpy(), x.cpu().numpy()
    b = R.gain_bound(K, x.shape[-1])
    eps = 2.0 ** -24 if y.dtype == np.float32 else 2.0 ** -53
    gl = ref["g_ld"]
    xg = x.reshape(gl.shape[0], -1, x.shape[-1]).astype(np.longdouble)
    err = np.abs(y.reshape(xg.shape).astype(np.longdouble) - gl[:, None, :] * xg)
    tol = (b + eps * np.abs(gl))[:, None, :] * np.abs(xg)
    print(f"largest excess over the bound: {float((err - tol).max()):.3e} (<= 0 passes); largest deviation {float(err.max()):.3e}")
    assert y.shape == x.shape and np.all(err <= tol)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["1", "7", "512", "tile+1"])
def test_stream_processor_chunks_equal_the_one_shot_call(case, dtype, use_graph):
    from torchfx_amd import gate
    from torchfx_amd.realtime import StatefulGate, StreamProcessor

    B, K, x = stream_signal(case, dtype)
    ref = definition(case, dtype)
    assert 0.2 < ref["open"].mean() < 0.98                             # the gate is at work
    _, o, st = gate(x.to(DEV), FS, return_open=True, return_state=True, **KW)
    assert np.array_equal(o.cpu().numpy(), ref["open"])
    gt = StatefulGate(**KW)
    proc = StreamProcessor([gt], chunk_size=B, device=DEV, use_graph=use_graph)
    got = proc.process_tensor(x, FS)
    assert (proc._graph is not None) == use_graph
    bounded(got, ref, x, K)
    assert gt._hist.shape == (1, 3) and gt._hist.dtype == torch.float64
    assert torch.equal(gt._hist[:, 1:], st[:, 1:]) and np.array_equal(gt._hist.cpu().numpy()[:, 1:], ref["state"][:, 1:])
    assert abs(float(gt._hist[0, 0]) - float(ref["g_ld"][0, -1])) <= R.gain_bound(K, x.shape[-1])


def test_chain_with_a_compressor_equals_the_staged_one_shot_chain():
    from torchfx_amd import compress, gate
    from torchfx_amd.realtime import StatefulCompressor, StatefulGate, StreamProcessor

    B, K, x = stream_signal(2, torch.float32)
    x = x * 40.0                                                       # up to the compressor's threshold
    kw = dict(KW, threshold_db=KW["threshold_db"] + 20.0 * np.log10(40.0))
    g = gate(x.to(DEV), FS, **kw)
    ref = compress(g, FS, -18.0, 3.0)
    assert not torch.equal(g, x.to(DEV)) and not torch.equal(ref, g)   # both stages are at work
    for use_graph in (False, True):
        got = StreamProcessor([StatefulGate(**kw), StatefulCompressor(-18.0, 3.0)], chunk_size=B, device=DEV,
                              use_graph=use_graph).process_tensor(x, FS)
        # the gate's float32 output may round the other way where its gain differs in the last bits (2^-23 relative); the
        # compressor's gain follows its input with slope 1 - 1/ratio < 1, and its product is rounded once more: < 2^-21 in all
        err = (got.double() - ref.double()).abs()
        assert float((err - 2.0 ** -21 * ref.double().abs() - 1e-10 * float(ref.abs().max())).max()) <= 0.0


def test_explain_and_route_name_the_native_kernel():
    from torchfx_amd import Gate, Wave

    x = torch.zeros(2, 3 * tile() + 5)
    lines = (Wave(x, FS, device=DEV) | Gate(**KW)).explain()
    assert lines == [f"Gate: native (gate_kernel, hysteresis decision and gain smoother as scans, hold H = 48 samples, 4 tile(s) of "
                     f"{tile()} per group in 4 segment(s); three launches)"]
    lines = (Wave(torch.zeros(2, 100), FS, device=DEV) | Gate(**KW)).explain()
    assert lines[0].endswith("1 tile(s) of 2048 per group in 1 segment(s); one launch)")
