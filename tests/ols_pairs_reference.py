"""Host model of PAIRED overlap-save (two real frames per complex transform) and of where a non-finite sample may come out.

The overlap-save kernels (olslds.hip, olsnative.hip, olsnative64.hip) cut every row of a ``[C, T]`` signal into ``F`` frames of
``N`` points that advance by the hop ``S`` and transform the frames two at a time as ``z = frame_a + 1j * frame_b``, pairing the
GLOBAL frames ``2p`` and ``2p + 1`` of the ``C * F`` frames.  With an odd ``F`` the last frame of row ``c`` therefore rides with
the first frame of row ``c + 1``.  Rows are independent signals: a non-finite sample may widen to the frames that share a
transform with it INSIDE its row, never into another row.

``poisoned_mask`` states which outputs must be non-finite; ``paired_ols`` is a float64 NumPy emulation of the kernels' geometry
that the mask is proven against (tests/test_ols_pairs_host.py); the GPU tests (tests/test_gpu_ols_rows.py) hold the kernels to
the mask.  Nothing here touches the code under test.
"""
import numpy as np


def poisoned_mask(row, n, C, Tout, K, pl, N, S, F, lead):
    """Boolean ``[C, Tout]``: the outputs that must be non-finite when sample ``n`` of row ``row`` is NaN / Inf.

    Frame ``f`` of the row is hit when its window ``[f S - pl - lead, f S - pl - lead + N)`` holds ``n``; a hit frame's hop
    ``[f S, min((f + 1) S, Tout))`` is poisoned, and so is the hop of the frame it shares a transform with (global frame
    ``g ^ 1``, ``g = row F + f``) when that frame exists and lies in the same row.  Nothing in another row is."""
    mask = np.zeros((C, Tout), dtype=bool)
    for f in range(F):
        w0 = f * S - pl - lead
        if not (w0 <= n < w0 + N):
            continue
        g = row * F + f
        for h in (g, g ^ 1):
            if h < C * F and h // F == row:
                fh = h - row * F
                mask[row, fh * S:min((fh + 1) * S, Tout)] = True
    return mask


def paired_ols(x, k, pl, pr, N, S, F, lead, rule="two-sided"):
    """Float64 emulation of paired overlap-save: ``x [..., C, T]`` (leading dimensions are independent cases) correlated with the
    stored (flipped) kernel ``k [K]`` like ``fft_conv1d`` -- ``y[t] = sum_i k[i] xp[t + i]`` on the padded rows, ``Tout = T + pl +
    pr - K + 1`` -- in frames of ``N`` points at hop ``S``, the taps behind ``lead`` zeros, global frames ``2p`` / ``2p + 1`` in one
    complex FFT.

    rule "two-sided": in a pair that straddles two rows, non-finite samples of EITHER frame enter the transform as zeros and
    each frame that held one gets a NaN hop; the other frame keeps its own output.  "one-sided": only frame b (the later row's
    first frame) is treated so.  Pairs inside a row are transformed as they are."""
    assert rule in ("two-sided", "one-sided")
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    *batch, C, T = x.shape
    K = k.shape[0]
    Tout = T + pl + pr - K + 1
    assert 1 <= S <= N - (K + lead) + 1 and F * S >= Tout, "a hop holds only valid block outputs and the frames cover the row"
    x = x.reshape((-1, C, T))
    B = x.shape[0]
    # frames: window m of frame f is sample f S - pl - lead + m of the row, zero outside [0, T)
    idx = (np.arange(F)[:, None] * S - pl - lead) + np.arange(N)[None, :]            # [F, N]
    inside = (idx >= 0) & (idx < T)
    frames = np.where(inside[None, None], x[:, :, np.clip(idx, 0, max(T - 1, 0))], 0.0)   # [B, C, F, N]
    frames = frames.reshape(B, C * F, N)
    nfr = C * F
    if nfr & 1:
        frames = np.concatenate([frames, np.zeros((B, 1, N))], axis=1)
    a, b = frames[:, 0::2].copy(), frames[:, 1::2].copy()                            # [B, P, N]
    P = a.shape[1]
    ga = 2 * np.arange(P)
    straddle = (ga + 1 < nfr) & (ga // F != (ga + 1) // F)                           # [P]
    bad_b = straddle[None] & ~np.isfinite(b).all(axis=-1)
    b[bad_b[..., None] & ~np.isfinite(b)] = 0.0
    bad_a = np.zeros_like(bad_b)
    if rule == "two-sided":
        bad_a = straddle[None] & ~np.isfinite(a).all(axis=-1)
        a[bad_a[..., None] & ~np.isfinite(a)] = 0.0
    h = np.zeros(N)
    h[lead:lead + K] = k
    with np.errstate(invalid="ignore", over="ignore"):
        o = np.fft.ifft(np.fft.fft(a + 1j * b, axis=-1) * np.conj(np.fft.fft(h)), axis=-1)
    ya, yb = o.real[..., :S].copy(), o.imag[..., :S].copy()
    ya[bad_a] = np.nan
    yb[bad_b] = np.nan
    hops = np.empty((B, 2 * P, S))
    hops[:, 0::2], hops[:, 1::2] = ya, yb
    y = hops[:, :nfr].reshape(B, C, F * S)[:, :, :Tout]
    return y.reshape((*batch, C, Tout))


def rowwise_reference(x, k, pl, pr):
    """Every row on its own in float64: ``y[c, t] = sum_i k[i] xp[c, t + i]`` (``np.convolve`` with the kernel turned round)."""
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    K = k.shape[0]
    out = []
    for r in x.reshape((-1, x.shape[-1])):
        xp = np.pad(r, (pl, pr))
        out.append(np.convolve(xp, k[::-1])[K - 1:xp.shape[0]])
    return np.stack(out).reshape((*x.shape[:-1], -1))
