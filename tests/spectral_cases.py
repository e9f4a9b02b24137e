"""The cases of the spectral edge tests (tests/test_gpu_istft_edges.py, tests/test_gpu_stft_edges.py,
tests/test_spectral_cases_host.py): asymmetric windows, the wrong windows a kernel could apply in their place, Gaussian complex
bins, frame counts and lone-frame placements.  NumPy, CPU torch and the host-only plan queries: nothing here needs a device.

Geometry is looked up from ``istft_plan_info`` / ``stft_plan_info`` (through the helpers of tests/test_gpu_istft.py and
tests/test_gpu_stft.py) and compared with what the GPU tests assume by tests/test_spectral_cases_host.py, never written down.

The windows.  ``ramp(n) = (i + 1) / n`` and ``falling(n) = (n - 1 - i) / n`` are exact in float32 for every n_fft up to 4096 (n a
power of two) and read differently from either end, so reversed or shifted indexing shows.  A short window has ``n_fft - 55``
values: the zeros around it split 27 | 28, so rounding the left padding up instead of down shows as well.

The one-tap probe.  With hop = 1 and win_length = 1 the single tap sits at sample ``(n_fft - 1) // 2 = 127`` of every frame (256)
and the result is cut by n_fft / 2 = 128 at the start: output t is the padded position t + 128, which only frame t + 1 reaches
with its tap.  A tap of 1 squares to 1, a tap of 2 gives 2 s / 4 and a tap of 0.5 gives 0.5 s / 0.25: one exact scaling each.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import istft_reference as IR
from tests.test_gpu_istft import CDT, RDT, plan, three_tiles
from tests.test_gpu_stft import plan_g

NP = {"f32": np.float32, "f64": np.float64}
DTS = ("f32", "f64")
ODD = 55                                                 # n_fft - win_length of the short windows: 27 zeros left, 28 right


def ramp(n):
    return (np.arange(n) + 1.0) / n


def falling(n):
    return (n - 1.0 - np.arange(n)) / n


@functools.lru_cache(maxsize=None)
def _bins(n, frames, rows, dt, seed):
    g = np.random.default_rng(7919 * seed + n + frames)
    shape = (rows, n // 2 + 1, frames)
    return torch.from_numpy(g.standard_normal(shape) + 1j * g.standard_normal(shape)).to(CDT[dt])


def bins(n, frames, rows, dt, seed=0):
    """Gaussian complex bins ``[rows, n / 2 + 1, frames]`` on the CPU, drawn in float64 and rounded once: an arbitrary spectrum,
    no STFT of anything, the imaginary parts of bins 0 and n / 2 included (no inverse reads them).  Shared: do not write to it."""
    return _bins(n, frames, rows, dt, seed)


# ---- A: window orientation and placement -----------------------------------------------------------------------------------
Placed = namedtuple("Placed", "n wl hop normalized")
A_SIZES = (256, 1024, 4096)
A_ROWS = 3
A_CASES = [Placed(n, wl, wl // 4, False) for n in A_SIZES for wl in (n, n - ODD)] + [Placed(256, 256 - ODD, (256 - ODD) // 4, True)]
F_CASES = [Placed(n, n - ODD, (n - ODD) // 4, False) for n in (256, 4096)]


def placed_id(c):
    return "n%d-wl%d-hop%d%s" % (c.n, c.wl, c.hop, "-normalized" if c.normalized else "")


def placed_frames(c, dt):
    return three_tiles(c.n, c.hop, dt, c.wl)


def placed_input(c, dt):
    return bins(c.n, placed_frames(c, dt), A_ROWS, dt, 1)


def full(w, n):
    """``w`` centred in n zeros as the contract has it: (n - len(w)) // 2 zeros on the left."""
    out = np.zeros(n)
    left = (n - len(w)) // 2
    out[left:left + len(w)] = w
    return out


def placed_window(c, dt):
    """The case's window as the transform gets it: the ramp over win_length, rounded once to the dtype."""
    return ramp(c.wl).astype(NP[dt])


def wrong_windows(c, dt):
    """The full-length windows a wrong kernel would apply instead of ``full(window, n)``: read from the other end, the short
    window reversed before it is padded, and the padding rounded up (every tap one sample late)."""
    w = placed_window(c, dt).astype(np.float64)
    return {"reversed": full(w, c.n)[::-1].copy(), "short reversed": full(w[::-1], c.n), "late by one": np.roll(full(w, c.n), 1)}


def placed_reference(c, dt, window=None):
    """(y, bound) of tests/istft_reference.py for the case's input; ``window``: a full-length window in place of the ramp."""
    X = placed_input(c, dt).numpy()
    if window is None:
        return IR.reference(X, c.n, c.hop, c.n // 2, placed_window(c, dt), c.wl, None, c.normalized)
    return IR.reference(X, c.n, c.hop, c.n // 2, window, c.n, None, c.normalized)


# ---- B: one tap, hop 1 --------------------------------------------------------------------------------------------------------
TAP_N = 256
TAP_AT = (TAP_N - 1) // 2
TAPS = ((1.0, 1.0), (2.0, 0.5), (0.5, 2.0))              # (the tap, what the result is multiplied by)


def tap_frames(dt):
    return three_tiles(TAP_N, 1, dt, 1)


def tap_input(dt):
    return bins(TAP_N, tap_frames(dt), 2, dt, 2)


def tap_expected(frames_flat):
    """``frames_flat [rows, F n]``, the frames side by side (hop = n, rectangular, not centred) -> what hop = 1 with one tap of 1
    returns: sample 127 of frames 1 ... F - 1."""
    rows = frames_flat.shape[0]
    return frames_flat.reshape(rows, -1, TAP_N)[:, 1:, TAP_AT]


def scales_exactly(v):
    """Whether halving and doubling every value of ``v`` is exact in its dtype: no value is lost to underflow or overflow."""
    a = np.abs(np.asarray(v))
    f = np.finfo(a.dtype)
    return bool(np.isfinite(a).all() and ((a == 0) | ((a >= 4 * f.tiny) & (a <= f.max / 4))).all())


# ---- C: a lone frame ----------------------------------------------------------------------------------------------------------
def lone_geometry(n, hop, dt):
    """(frames, G, tile, the placements) of a lone frame at n_fft n, not centred: three tiles' worth of frames, or G + 2 where
    that is fewer (n_fft 256 holds 32 frames a batch), so that frames G - 1, G and the last one exist and differ."""
    p = plan(n, hop, 8, dt, center=False)
    G, tile = p["frames_per_batch"], p["tile"]
    assert tile % hop == 0
    frames = max(three_tiles(n, hop, dt), G + 2)
    at = sorted({0, G - 1, G, tile // hop - 1, tile // hop, frames - 1})
    assert at[0] == 0 and at[-1] == frames - 1
    return frames, G, tile, at


def lone_blocks(n, dt):
    """The two rows' frames: bins ``[2, n / 2 + 1]``."""
    return bins(n, 1, 2, dt, 3)[..., 0]


def lone_cover(n, hop, frames, f):
    """What a lone frame at index f is divided by, per sample of its block: the count of rectangular windows over it."""
    L = (frames - 1) * hop + n
    cnt = np.zeros(L)
    for k in range(frames):
        cnt[k * hop:k * hop + n] += 1
    return cnt[f * hop:f * hop + n]


# ---- D: the flag's reach ------------------------------------------------------------------------------------------------------
NEAR = ((1e-5, True), (1e-6, False))                     # a constant window and whether its envelope exceeds 1e-11
NEAR_GEOMETRIES = ((256, 256, False), (256, 64, True))   # (n_fft, hop, centred)


def near_envelope(value, n, hop):
    """The float32 overlap-add envelope of a constant window: n / hop squares added in order."""
    sq = np.float32(value) * np.float32(value)
    env = np.float32(0)
    for _ in range(n // hop):
        env = np.float32(env + sq)
    return float(env)


# ---- G, H, I: the forward transform -------------------------------------------------------------------------------------------
APART_SIZES = (256, 4096)


def apart_hops(n):
    return (n - 1, n + 1, n + 3, 3 * n + 5)


def apart_lengths(n, hop, dt):
    """(G, T centred, T not centred): 2 G + 1 frames either way, so three workgroups share a row and the last holds one frame;
    both lengths are odd."""
    G = plan_g(n, NP[dt])
    return G, 2 * G * hop + 1, 2 * G * hop + n + 1


def short_rows(n):
    """The row lengths at and below the zero padding of n / 2."""
    pad = n // 2
    return (1, 2, pad - 1, pad, pad + 1)


def short_hops(n):
    return ((1,) if n == 256 else ()) + (n // 4,)


NOTHING_TO_PAD = ("constant", "replicate", "circular")
NOTHING_TO_PAD_SIZES = (256, 1024)
