"""StatefulResample on the device (csrc/resample.hip, the stream variants of resample_kernel): all chunk outputs plus flush()
are torch.equal to resample_poly on the whole signal, on the same device and dtype, for every ratio of
tests/test_gpu_resample.py, every chunking, every input shape, misaligned rows and each of the three kernels; non-finite
samples poison what the contract says; one launch per chunk; StreamProcessor with a resampler in the chain."""
import json
import math

import numpy as np
import pytest
import scipy.signal as ss
import torch

from tests.gpu_common import DEV, close
from tests.test_gpu_resample import EXTRA, TABLE
from tests.test_stream_resample_host import random_sizes

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def stateful(up, down, **kw):
    from torchfx_amd.realtime import StatefulResample
    return StatefulResample(up * 100, down * 100, **kw)


def one_shot(x, up, down, **kw):
    from torchfx_amd import resample_poly
    return resample_poly(x, up, down, **kw)


def signal(shape, dtype, seed, offset=0):
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    base = (torch.rand(n + offset, generator=g, dtype=torch.float64) * 2 - 1).to(dtype).to(DEV)
    return base[offset:].view(*shape)                  # offset 1: rows that start off any 16-byte boundary


def chunked(r, x, sizes):
    outs, o, n, sizes = [], 0, x.shape[-1], list(sizes)
    while o < n:
        k = sizes.pop(0) if sizes else n - o
        outs.append(r(x[..., o:o + k]))
        o += k
    outs.append(r.flush())
    return torch.cat(outs, dim=-1)


def length(up, down):
    """140 000 inputs, fewer where the output would pass ~4 M samples per row."""
    return min(140_000, 4_000_000 * down // up)


CHUNKINGS = {"rt512": lambda n, s: [512] * (n // 512 + 1), "large": lambda n, s: [65536] * (n // 65536 + 1),
             "random": lambda n, s: random_sizes(n, s, 9000)}


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", TABLE + EXTRA)
def test_chunks_equal_one_shot(up, down, dtype, chunking):
    T = length(up, down)
    x = signal((2, T), dtype, up * 31 + down)
    got = chunked(stateful(up, down), x, CHUNKINGS[chunking](T, up + down))
    ref = one_shot(x, up, down)
    assert got.shape == ref.shape == (2, math.ceil(T * up / down)) and got.dtype == dtype and got.is_cuda
    assert torch.equal(got, ref), f"{up}/{down} {chunking}: max diff {(got - ref).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", TABLE + EXTRA)
def test_one_sample_chunks(up, down, dtype):
    x = signal((2, 300), dtype, 7)
    r = stateful(up, down)
    outs = [r(x[:, i:i + 1]) for i in range(300)]
    pre = r.latency
    assert [o.shape[-1] for o in outs] == [max(0, math.ceil((i + 1) * up / down) - pre) - max(0, math.ceil(i * up / down) - pre)
                                           for i in range(300)]
    assert torch.equal(torch.cat([*outs, r.flush()], dim=-1), one_shot(x, up, down))


@pytest.mark.parametrize("shape", [(20011,), (3, 20011), (2, 3, 20011)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_shapes(shape, dtype):
    x = signal(shape, dtype, 11)
    got = chunked(stateful(160, 147), x, random_sizes(20011, 5, 3000))
    assert got.shape[:-1] == shape[:-1]
    assert torch.equal(got, one_shot(x, 160, 147))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_misaligned_and_strided_rows(dtype):
    x = signal((3, 30001), dtype, 12, offset=1)
    assert torch.equal(chunked(stateful(147, 160), x, [4097] * 8), one_shot(x, 147, 160))
    base = signal((4, 3, 10007), dtype, 13)
    view = base[:, 1, :]                                   # rows 3 * 10007 apart
    assert torch.equal(chunked(stateful(160, 147), view, [1000] * 11), one_shot(view.contiguous(), 160, 147))


@pytest.mark.parametrize("up,down,dtype,kernel", [
    (160, 147, torch.float32, "resample_stream_reg_kernel"), (997, 1000, torch.float64, "resample_stream_reg_kernel"),
    (1, 6, torch.float32, "resample_stream_lds_kernel"), (1, 480, torch.float32, "resample_stream_lds_kernel"),
    (1, 480, torch.float64, "resample_stream_gather_kernel"), (1, 8000, torch.float32, "resample_stream_gather_kernel"),
    # more than one phase in the gather kernel (most 512-sample chunks complete no output: the history-only launch), G halved
    # to an odd count in the lds kernel, G halved in the reg kernel (the 41-tap window of tests/test_gpu_resample_edges.py)
    (3, 4000, torch.float32, "resample_stream_gather_kernel"), (3, 200, torch.float32, "resample_stream_lds_kernel"),
    (3, 200, torch.float64, "resample_stream_lds_kernel"), (2, 75, torch.float32, "resample_stream_reg_kernel")])
def test_each_kernel(up, down, dtype, kernel):
    kw = {}
    if (up, down) == (2, 75):
        from tests.test_gpu_resample_edges import CASES, window_of
        kw["window"] = window_of(next(c for c in CASES if (c.up, c.down) == (2, 75)))
        assert len(kw["window"]) == 41
    r = stateful(up, down, **kw)
    T = 200_000 if down >= 480 else 50_000
    x = signal((2, T), dtype, up + down)
    assert r.route(x, 4096) == f"native ({kernel})"
    # a stream tile of these short chunks is up * G outputs (E halved down to 1): 3 at 3/4000, at most 129 at 3/200 and 256 at
    # 2/75, so the rows (150, 750 and 1334 outputs) and the longest chunks span several tiles
    assert torch.equal(chunked(r, x, [512] * 20 + random_sizes(T, 3, 30000)), one_shot(x, up, down, **kw))


def _poisoned(x_len, bad, up, down, h):
    """The outputs whose non-zero taps touch input `bad`: h_padded[(m + pre)*down - up*bad] != 0."""
    nh = h.numel()
    half_len = (nh - 1) // 2
    pre_pad = down - half_len % down
    pre = (half_len + pre_pad) // down
    m = np.arange(math.ceil(x_len * up / down))
    k = (m + pre) * down - up * bad - pre_pad
    hit = np.zeros(m.shape, bool)
    ok = (k >= 0) & (k < nh)
    hit[ok] = h.numpy()[k[ok]] != 0
    return hit


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", [(160, 147), (147, 160), (1, 3), (3, 1), (1, 6), (1, 480)])
def test_non_finite_samples(up, down, dtype):
    from torchfx_amd.resample import design_taps
    T, C = 6000, 512
    x = signal((3, T), dtype, 14)
    x[1, 2 * C + C // 2] = float("nan")                    # the middle of a chunk
    x[1, 2 * C - 1] = float("inf")                         # the last sample of a chunk: the next one's history
    x[2, 5 * C - 3] = float("-inf")
    got = chunked(stateful(up, down), x, [C] * 12).cpu().numpy()
    ref = one_shot(x, up, down).cpu().numpy()
    fin = np.isfinite(ref)
    assert np.array_equal(got[fin], ref[fin])               # bit for bit wherever the one-shot is finite
    assert not (~np.isfinite(got) & fin).any()               # its non-finite outputs are a subset of the one-shot's
    assert np.isfinite(got[0]).all()
    h = design_taps(up, down, dtype=dtype)
    for row, bad in ((1, 2 * C + C // 2), (1, 2 * C - 1), (2, 5 * C - 3)):
        hit = _poisoned(T, bad, up, down, h)
        assert hit.any() and not np.isfinite(got[row][hit]).any(), (row, bad)


def test_one_launch_per_chunk():
    from torchfx_amd import _lib
    lib = _lib.load()
    for up, down, dtype, name in ((160, 147, torch.float32, "resample_stream_reg_kernel"),
                                  (1, 6, torch.float32, "resample_stream_lds_kernel"),
                                  (1, 480, torch.float64, "resample_stream_gather_kernel")):
        r = stateful(up, down)
        x = signal((2, 512 * 20), dtype, 15)
        blocks = [x[:, 512 * i:512 * (i + 1)].contiguous() for i in range(20)]
        r(blocks[0][:, :0])                                  # the taps and the polyphase table exist before the count starts
        lib.tfx_prof_enable(1)
        lib.tfx_prof_collect()
        for b in blocks:
            r(b)
        torch.cuda.synchronize()
        prof = json.loads(lib.tfx_prof_collect().decode())
        lib.tfx_prof_enable(0)
        assert set(prof) == {name} and prof[name]["calls"] == 20, prof


def test_device_change_restarts():
    x = signal((2, 5000), torch.float64, 16)
    r = stateful(160, 147)
    r(x[:, :2000])
    tail = x[:, 2000:].cpu()                                 # the same rows on the host: a new stream from silence
    got = chunked(r, tail, [700] * 5)
    assert not got.is_cuda
    close(got, ss.resample_poly(tail.numpy(), 160, 147, axis=-1), 1e-11, "restart on the host")
    assert torch.equal(chunked(r, x, [999] * 6), one_shot(x, 160, 147))   # and back on the device


@pytest.mark.parametrize("use_graph", [False, True])
def test_stream_processor_single_resampler_is_exact(use_graph):
    from torchfx_amd.realtime import StatefulResample, StreamProcessor
    x = signal((2, 100_000), torch.float32, 17).cpu()
    for chunk in (512, 4096, 65536):
        proc = StreamProcessor([StatefulResample(48000)], chunk_size=chunk, device=DEV, use_graph=use_graph)
        got = proc.process_tensor(x, 44100)
        assert torch.equal(got, one_shot(x.to(DEV), 160, 147)), chunk


def test_stream_processor_chain_matches_one_shot():
    from scipy.signal import firwin

    from torchfx_amd import filter as F
    from torchfx_amd.realtime import StatefulFIR, StatefulResample, StreamProcessor
    x = signal((4, 300_000), torch.float32, 18).cpu()
    taps = firwin(513, 5000, fs=48000)

    def effects():
        return [F.LoButterworth(8000, order=6), StatefulResample(48000), StatefulFIR(taps)]
    lo, fir = F.LoButterworth(8000, order=6, fs=44100), StatefulFIR(taps)
    whole = fir(one_shot(lo(x.to(DEV)), 160, 147))
    for chunk in (65536, 4096, 1000):
        chain = effects()
        out = StreamProcessor(chain, chunk_size=chunk, device=DEV).process_tensor(x, 44100)
        assert chain[0].fs == chain[1].fs == 44100
        close(out, whole.cpu().numpy(), 2e-6, f"chunk={chunk}")
