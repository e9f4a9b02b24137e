"""StatefulGate without a device: chunks against the per-sample loop of tests/gate_reference.py on the whole signal (open track
and the (open, c) of the state exact, outputs within the derived bound), inside StreamProcessor, the refusal of a plain Gate by
both processors with its full text, top-level and nested, and reset_state."""
import numpy as np
import pytest
import torch

from tests import gate_reference as R

FS = 48000
KW = dict(threshold_db=-30.0, hysteresis_db=4.0, range_db=24.0, attack=0.5e-3, hold=4e-3, release=20e-3)
TEXT = ("Gate cannot run in {who}: every call starts closed with its hold counter at zero, so a chunked stream would shut the gate at "
        "every chunk start; use StatefulGate(...) in its place, or gate the whole signal (wave | Gate(...)) before or after streaming")


def signal(lead, T, seed, dtype):
    K = R.constants(FS, **KW)
    H = K["H"]                                                         # 192
    rng = np.random.default_rng(seed)
    runs = [(100, H - 1), (400, H), (700, H + 1), (1100, 3 * H), (T - 150, 100)]
    return K, R.phrases(rng, tuple(lead) + (T,), K, runs, dtype)


def bounded(y, ref, x, K):
    """|y - g_ld x| <= (b + eps |g_ld|) |x| with eps the rounding of the product in y's dtype."""
    b = R.gain_bound(K, x.shape[-1])
    eps = 2.0 ** -24 if y.dtype == np.float32 else 2.0 ** -53
    gl = ref["g_ld"]
    xg = x.reshape(gl.shape[0], -1, x.shape[-1]).astype(np.longdouble)
    err = np.abs(y.reshape(xg.shape).astype(np.longdouble) - gl[:, None, :] * xg)
    assert np.all(err <= (b + eps * np.abs(gl))[:, None, :] * np.abs(xg))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("link", [True, False], ids=["linked", "unlinked"])
def test_stateful_gate_chunks_equal_the_loop_on_the_whole_signal(dtype, link):
    from torchfx_amd import gate
    from torchfx_amd.realtime import StatefulGate

    K, x = signal((2,), 2600, 1, dtype)
    ref = R.gate_ref(x, K, link)
    assert 0.3 < ref["open"].mean() < 0.95
    g = StatefulGate(link=link, fs=FS, **KW)
    cuts = [0, 1, 8, 290, 291, 292, 1000, 1001, 2599, 2600]           # 291 = 100 + H - 1: a cut inside every hold
    y = np.concatenate([g(torch.from_numpy(x[:, a:b].copy())).numpy() for a, b in zip(cuts, cuts[1:])], -1)
    bounded(y, ref, x, K)
    assert g._hist.shape == (ref["state"].shape[0], 3) and g._hist.dtype == torch.float64
    assert np.array_equal(g._hist.numpy()[:, 1:], ref["state"][:, 1:])
    assert np.abs(g._hist.numpy()[:, 0] - ref["state"][:, 0]).max() <= R.gain_bound(K, 2600)
    g.reset_state()
    assert g._hist is None and g._key is None
    first = g(torch.from_numpy(x[:, :700].copy()))
    assert torch.equal(first, gate(torch.from_numpy(x[:, :700].copy()), FS, link=link, **KW))     # from the closed gate again
    g(torch.from_numpy(x[:1, :10].copy()))                             # another row count: a new stream
    assert g._hist.shape == (1, 3)


def test_a_plain_gate_per_chunk_would_differ():
    """What the refusal is about: the stateless effect shuts at a chunk start inside a hold."""
    from torchfx_amd import gate

    K, x = signal((1,), 2600, 2, np.float64)
    xt = torch.from_numpy(x)
    whole = gate(xt, FS, return_open=True, **KW)[1]
    cut = 100 + K["H"] // 2                                            # inside the first hold
    pieces = torch.cat([gate(xt[:, :cut], FS, return_open=True, **KW)[1], gate(xt[:, cut:], FS, return_open=True, **KW)[1]], -1)
    assert whole[0, cut] == 1 and pieces[0, cut] == 0


@pytest.mark.parametrize("chunk", [1, 7, 512, 2049])
def test_stream_processor_runs_stateful_gate_over_cpu_chunks(chunk):
    from torchfx_amd import realtime as RT

    K, x = signal((2,), 1500 if chunk == 1 else 2 * 2049 + 77, 3, np.float32)
    gt = RT.StatefulGate(**KW)
    sp = RT.StreamProcessor([gt], chunk_size=chunk, device="cpu")
    y = sp.process_tensor(torch.from_numpy(x), FS).numpy()
    ref = R.gate_ref(x, K)
    bounded(y, ref, x, K)
    assert np.array_equal(gt._hist.numpy()[:, 1:], ref["state"][:, 1:])


def _no_backend(RT):
    class Backend(RT.AudioBackend):
        def open_stream(self, config, callback=None):
            raise AssertionError("the refusal comes before a stream is opened")

        def start(self):
            pass

        def stop(self):
            pass

        def close(self):
            pass
    return Backend()


def test_stream_processors_refuse_the_plain_gate_with_the_full_text():
    import torchfx_amd as f
    from torchfx_amd import realtime as RT

    class Wrap(f.FX):
        """An effect that holds another one inside an ``nn.Sequential``: not a top-level effect of the chain."""

        def __init__(self, *inner):
            super().__init__()
            self.inner = torch.nn.Sequential(f.Gain(0.5), *inner)

        def forward(self, x):
            return self.inner(x)

    for chain in ([f.Gate()], [f.Gain(0.5), f.Gate(-45), f.Gain(2.0)], [Wrap(f.Gate(-45))], [f.Gain(0.5), Wrap(f.Gate(fs=FS))]):
        with pytest.raises(TypeError) as e:
            RT.StreamProcessor(chain, chunk_size=256, device="cpu")
        assert str(e.value) == TEXT.format(who="StreamProcessor")
        with pytest.raises(TypeError) as e:
            RT.RealtimeProcessor(chain, _no_backend(RT), RT.StreamConfig(), device="cpu")
        assert str(e.value) == TEXT.format(who="RealtimeProcessor")
    RT.StreamProcessor([RT.StatefulGate()], chunk_size=256, device="cpu")
    RT.StreamProcessor([Wrap(RT.StatefulGate())], chunk_size=256, device="cpu")
    RT.RealtimeProcessor([RT.StatefulGate()], _no_backend(RT), RT.StreamConfig(), device="cpu")
    gates = [r for r in RT._REFUSALS if r.plain is f.Gate]
    assert len(gates) == 1 and gates[0].stream is RT.StatefulGate
    # the families that were there keep their order; a compressor next to a gate in one effect raises the compressor's text
    assert [r.plain.__name__ for r in RT._REFUSALS if r.plain is not f.Gate] == [
        "ZeroPhase", "LoudnessNormalize", "Limiter", "Compressor", "ModulatedDelay", "Freeverb", "Waveshaper", "Resample", "Phaser"]
    with pytest.raises(TypeError, match="^Compressor cannot run in StreamProcessor"):
        RT.StreamProcessor([Wrap(f.Gate(), f.Compressor())], chunk_size=256, device="cpu")


def test_stateful_gate_needs_the_sample_rate_and_takes_it_from_the_processor():
    from torchfx_amd import realtime as RT

    g = RT.StatefulGate()
    with pytest.raises(ValueError, match="StatefulGate needs the sample rate"):
        g(torch.zeros(2, 16))
    RT.StreamProcessor([g], chunk_size=8, device="cpu").process_tensor(torch.zeros(2, 16), FS)
    assert g.fs == FS
    assert g._capture_key() == (-40.0, 6.0, float("inf"), 1e-3, 50e-3, 100e-3, True, FS)
