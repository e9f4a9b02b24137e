"""StreamProcessor's HIP-graph capture keeps Python's cyclic collector out: it collects before the capture (a dead cycle may hold
an earlier processor's CUDAGraph) and holds the collector off until the capture has ended."""
import gc

import numpy as np
import pytest
import torch

from tests.gpu_common import DEV

pytestmark = pytest.mark.gpu


def test_no_cyclic_collection_falls_into_a_capture():
    from torchfx_amd.realtime import StatefulDelay, StatefulReverb, StreamProcessor
    seen = []

    class Probe(StatefulDelay):
        def forward(self, x):
            seen.append((torch.cuda.is_current_stream_capturing(), gc.isenabled()))
            return super().forward(x)

    x = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 512 * 6)).astype(np.float32))
    chain = lambda cls: [cls(delay_samples=700, taps=2), StatefulReverb(delay=300)]      # noqa: E731
    eager = StreamProcessor(chain(StatefulDelay), chunk_size=512, device=DEV).process_tensor(x, 48000)
    assert gc.isenabled()
    sp = StreamProcessor(chain(Probe), chunk_size=512, device=DEV, use_graph=True)
    got = sp.process_tensor(x, 48000)
    assert gc.isenabled() and sp._graph is not None
    captured = [on for capturing, on in seen if capturing]
    assert captured and not any(captured)            # the collector was off for every call inside the capture ...
    assert all(on for capturing, on in seen if not capturing)                            # ... and on for every other
    assert torch.equal(got, eager)
