"""Identity phase locking (``phase_vocoder(..., phase_lock="identity")``) as a plain loop over frames and bins: moduli in float64,
angles in longdouble quantised to Python integers mod 2^64.  The bound is tests/phasevocoder_reference.py's with another angle
count: U[t+1,k] = U[t,P] + A[i_t+1,k] - A[i_t,P] (the bin's own A[i_t,k] cancels as an integer), so a step adds two quantised
angles to the path and the lock two more: phi[t,k] rests on at most 2 t + 3 (4 t + 3 without the cancellation; plain: 2 t + 1).
:func:`reference` also returns the smallest |mag[k] - mag[j]| over the compared pairs that are no exact ties, over the largest
modulus, for the caller to assert the margin of the discrete peak decisions on."""
import math

import numpy as np

from tests import phasevocoder_reference as R

M64 = 1 << 64


def peaks(m):
    n = len(m)
    return [all(m[k] > m[j] for j in (k - 2, k - 1, k + 1, k + 2) if 0 <= j < n) for k in range(n)]


def nearest(pk, k):
    """The nearest peak, the lower at equal distance; ``k`` when there is none."""
    for d in range(len(pk)):
        for p in (k - d, k + d):
            if 0 <= p < len(pk) and pk[p]:
                return p
    return k


def reference(X, rate):
    """``(re, im, mag, margin)`` of the locked vocoder of ``X [rows, bins, F]`` (finite): longdouble parts, float64 mag."""
    real = np.float32 if X.dtype == np.complex64 else np.float64
    rows, bins, F = X.shape
    i, alpha = R.positions(F, rate, real)
    Xp = np.concatenate([X, np.zeros((rows, bins, 2), X.dtype)], axis=-1).astype(np.complex128)
    turns = np.where(Xp != 0, np.arctan2(Xp.imag.astype(R.LD), Xp.real.astype(R.LD)) / (2 * R.PI), R.LD(0)) * R.LD(2.0 ** 64)
    hi = turns.astype(np.float64)
    A = [[[(int(h) + int(l)) % M64 for h, l in zip(hr, lr)] for hr, lr in zip(hb, lb)]
         for hb, lb in zip(hi.tolist(), np.rint(turns - hi).astype(np.float64).tolist())]
    M = np.abs(Xp)
    mag = alpha.astype(np.float64) * M[..., i + 1] + (1 - alpha.astype(np.float64)) * M[..., i]
    phi = np.empty(mag.shape, R.LD)
    margin = math.inf
    for r in range(rows):
        U = [A[r][k][0] for k in range(bins)]
        for t in range(len(i)):
            m = mag[r, :, t].tolist()
            gaps = [abs(m[k] - m[j]) for k in range(bins) for j in (k + 1, k + 2) if j < bins and m[k] != m[j]]
            margin = min([margin] + gaps)
            pk = peaks(m)
            a0, a1 = [A[r][k][i[t]] for k in range(bins)], [A[r][k][i[t] + 1] for k in range(bins)]
            near = [nearest(pk, k) for k in range(bins)] if any(pk) else list(range(bins))
            ph = [(U[p] + a0[k] - a0[p]) % M64 for k, p in enumerate(near)]
            phi[r, :, t] = [R.LD(v) / R.LD(2.0 ** 64) for v in ph]
            U = [(ph[k] + a1[k] - a0[k]) % M64 for k in range(bins)]
    ang = 2 * R.PI * phi
    return mag * np.cos(ang), mag * np.sin(ang), mag.astype(R.LD), margin / float(mag.max() or 1.0)


def within(got, ref, what=""):
    """Assert the locked bound on ``got`` against ``ref = reference(...)``; returns the largest error / bound."""
    re, im, mag, _ = ref
    real = np.float32 if got.dtype == np.complex64 else np.float64
    bound = R.bound(mag, real) + mag.astype(np.float64) * (2 * math.pi * 2 * R.E_ANGLE * (1 + 2.0 ** -10))    # 2 t + 3 angles
    assert got.shape == mag.shape, (what, got.shape, mag.shape)
    err = np.maximum(np.abs(got.real.astype(R.LD) - re), np.abs(got.imag.astype(R.LD) - im)).astype(np.float64)
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


def ladder(rows, bins, F, dt, seed=0):
    """A spectrum whose peak decisions have margin at every rate n / d with d in {1, 2, 4, 5}: moduli 7 r + (k mod 5) + 1 with r
    random in 0 .. 3, so two bins less than 5 apart differ by 7 (n a + (d - n) b) / d + delta with delta in +-{1 .. 4}, which is
    no nearer to zero than 1 / d; phases uniform."""
    g = np.random.default_rng(seed + 1000 * bins + F)
    m = 7.0 * g.integers(0, 4, (rows, bins, F)) + (np.arange(bins) % 5)[:, None] + 1.0
    return (m * np.exp(2j * np.pi * g.uniform(0, 1, m.shape))).astype(np.complex64 if dt == "f32" else np.complex128)
