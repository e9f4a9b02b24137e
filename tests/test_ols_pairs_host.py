"""The host model of paired overlap-save (tests/ols_pairs_reference.py) against itself: `poisoned_mask` -- what the GPU tests
(tests/test_gpu_ols_rows.py) hold the kernels to -- is exactly the non-finite set of the float64 emulation with the two-sided
rule for pairs that straddle rows, for every position of the bad sample, and the emulation with the one-sided rule (only the
later row's first frame is checked) breaks the mask: the model can see the defect.  No GPU."""
import numpy as np
import pytest

from tests.ols_pairs_reference import paired_ols, poisoned_mask, rowwise_reference

N = 64


def _geometry(K, F, lead):
    S = N - (K + lead) + 1
    T = (F - 1) * S + S // 2                       # pl = K - 1, pr = 0: Tout = T, the last frame is half full
    assert -(-T // S) == F
    return S, T


def _cases(K, C, F, lead, row, bad, seed=0):
    """One case per position n of the bad sample in `row`: x [T, C, T], the masks [T, C, T] and the row-wise reference with the
    bad sample set to 0."""
    S, T = _geometry(K, F, lead)
    rng = np.random.default_rng(seed + 1000 * K + 10 * C + F)
    k = rng.standard_normal(K)
    k /= np.abs(k).sum()
    x = np.broadcast_to(rng.uniform(-1, 1, (C, T)), (T, C, T)).copy()
    n = np.arange(T)
    zeroed = x.copy()
    zeroed[n, row, n] = 0.0
    x[n, row, n] = bad
    mask = np.stack([poisoned_mask(row, i, C, T, K, K - 1, N, S, F, lead) for i in n])
    return x, k, S, T, mask, rowwise_reference(zeroed, k, K - 1, 0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("F", [1, 3, 5, 2, 4])
@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("K", [5, 9])
def test_mask_is_the_emulations_non_finite_set(K, C, F, bad):
    """Every n of every row, every lead in [0, 8): the two-sided emulation is non-finite exactly on the mask and equals the
    row-wise float64 convolution (bad sample = 0) everywhere else to 1e-12.  Even F (no pair straddles rows) is the control:
    both rules are the same computation there."""
    for lead in range(8):
        for row in range(C):
            x, k, S, T, mask, ref = _cases(K, C, F, lead, row, bad)
            y = paired_ols(x, k, K - 1, 0, N, S, F, lead)
            assert y.shape == mask.shape == ref.shape == (T, C, T)
            assert np.array_equal(~np.isfinite(y), mask), f"lead={lead} row={row}"
            assert mask[:, row].any(axis=-1).all() and not np.delete(mask, row, axis=1).any()
            assert np.abs(y[~mask] - ref[~mask]).max() <= 1e-12
            if F % 2 == 0:
                assert np.array_equal(paired_ols(x, k, K - 1, 0, N, S, F, lead, rule="one-sided"), y, equal_nan=True)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("F", [1, 3, 5])
@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("K", [5, 9])
def test_one_sided_rule_breaks_the_mask(K, C, F, bad):
    """The rule the kernels had -- only frame b of a straddling pair is checked: a bad sample in the LAST frame of row 2p comes
    out in the first hop of row 2p + 1 (outside the mask), while one in the first frame of row 2p + 1 stays where the mask says.
    With F = 1 every sample of an even row that has a partner row does this."""
    lead = 3
    for row in range(C):
        x, k, S, T, mask, _ = _cases(K, C, F, lead, row, bad)
        nonfinite = ~np.isfinite(paired_ols(x, k, K - 1, 0, N, S, F, lead, rule="one-sided"))
        assert not (mask & ~nonfinite).any()                               # what must be non-finite is
        leak = (nonfinite & ~mask).any(axis=(1, 2))                        # [n]: something outside the mask is non-finite
        last_is_frame_a = (row * F + F - 1) % 2 == 0 and row + 1 < C       # the row's last frame is the real part of a straddling pair
        in_last = np.arange(T) >= (F - 1) * S - (K - 1) - lead             # n inside the last frame's window
        assert np.array_equal(leak, in_last & last_is_frame_a), f"row={row}"
        if last_is_frame_a:
            assert nonfinite[in_last][:, row + 1, :S].all() and not nonfinite[in_last][:, row + 1, S:].any()
