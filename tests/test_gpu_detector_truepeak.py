"""true_peak_kernel<T, LP> (csrc/resample.hip) at every register-tap bucket, cell by cell.  peak[row] shows only the row's
maximum, so the rows of tests/detector_cases.truepeak_rows are built -- and checked against the float64 reference
tests/resample_reference.ref -- so that every (slot, phase) cell of a thread's 16 positions x up phases owns the maximum of some
row, as do the first thread (the loop with the bounds test when rem > 0), the thread of the last position, lane 63 of wave 0,
lane 0 of wave 1 and both sides of the first tile seam.  Every row is compared bit for bit with the composition
resample_forward(x, up, 1, h).abs().amax(-1) and, within max_n bound[n], with the reference; then the row lengths around the
kernel's seams at every bucket, and non-finite samples with the caller's taps."""
import math

import numpy as np
import pytest
import torch

from tests import detector_cases as D
from tests.gpu_common import DEV, dev, ext
from tests.test_gpu_truepeak import FS, fx, uniform

pytestmark = pytest.mark.gpu

IDS = [D.case_id(c) for c in D.CASES]
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("dtype", D.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("k", range(len(D.CASES)), ids=IDS)
def test_every_cell_owns_the_maximum_of_some_row(k, dtype):
    """Largest |peak - peak_ref| / max_n bound[n] measured: 0.29 in float32, 0.38 in float64 (reference in long double)."""
    c = D.CASES[k]
    geo = D.check(c, dtype)
    h = D.taps(c, dtype, scaled=False)
    rows = D.truepeak_rows(k, dtype, geo["tile_in"])
    assert rows["long"].shape[-1] == geo["tile_in"] + 100
    cov, worst = {}, 0.0
    for name, x in rows.items():
        peak_ref, P, ph, tol = D.truepeak_reference(c, x, h.numpy(), wide=dtype == F64)
        cov[name] = D.cell_coverage(c, P, ph, x.shape[-1], geo["tile_in"])
        xd = dev(np.array(x))                                                  # the shared rows stay read-only
        got = fx().true_peak_linear(xd, FS[c.up], oversample=c.up, taps=h)
        comp = ext().resample_forward(xd, c.up, 1, h).abs().amax(-1)
        assert got.shape == comp.shape == (len(x),) and got.dtype == dtype
        assert torch.equal(got, comp), (name, torch.nonzero(got != comp).flatten().tolist()[:8])
        ratio = np.abs(got.cpu().numpy().astype(np.float64) - peak_ref) / tol
        worst = max(worst, float(ratio.max()))
        assert k not in D.FULL or float(peak_ref.min()) > 20 * D.TP_NOISE      # the burst, not the noise, is what is read
    print(D.case_id(c), dtype, "rows %d + %d, err / tol %.3f" % (len(rows["short"]), len(rows["long"]), worst))
    assert worst <= 1.0, worst
    if k in D.FULL:
        D.assert_truepeak_coverage(c, cov)


LENGTH_CASES = [(F32, 8, 57), (F32, 4, 61), (F32, 4, 83), (F32, 2, 63), (F32, 8, 381), (F32, 4, 253), (F32, 2, 128),
                (F64, 4, 28), (F64, 8, 187), (F64, 4, 256)]


def test_the_length_cases_cover_every_bucket():
    assert [D.find(u, n).bucket for d, u, n in LENGTH_CASES if d == F32] == list(D.BUCKETS)
    assert [D.find(u, n).bucket for d, u, n in LENGTH_CASES if d == F64] == [8, 24, 72]


@pytest.mark.parametrize("dtype,up,nh", LENGTH_CASES,
                         ids=["%s-%s" % ("f32" if d == F32 else "f64", D.case_id(D.find(u, n))) for d, u, n in LENGTH_CASES])
def test_lengths_around_the_seams_at_every_bucket(dtype, up, nh):
    c = D.find(up, nh)
    geo = D.check(c, dtype)
    h = D.taps(c, dtype, scaled=False)
    tile = geo["tile_in"]
    for T in [1, 7, c.Lp - 1, c.Lp, tile - 1, tile, tile + 1, 2 * tile + 3, 15, 16, 17]:
        x = uniform(dtype, T, (3,)).to(DEV)
        got = fx().true_peak_linear(x, FS[up], oversample=up, taps=h)
        comp = ext().resample_forward(x, up, 1, h).abs().amax(-1)
        assert got.shape == comp.shape and torch.equal(got, comp), (T, (got - comp).abs().max().item())
        assert float(got.min()) > 0.0


@pytest.mark.parametrize("dtype,up,nh", [(F32, 4, 256), (F32, 4, 83), (F64, 4, 83)], ids=["f32-b72", "f32-rem2", "f64-rem2"])
def test_non_finite_samples_stay_in_their_row_with_the_callers_taps(dtype, up, nh):
    c = D.find(up, nh)
    tile = D.check(c, dtype)["tile_in"]
    h = D.taps(c, dtype, scaled=False)
    x = uniform(dtype, 2 * tile + 3, (3,)).clone()
    clean = fx().true_peak_linear(x.to(DEV), FS[up], oversample=up, taps=h)
    assert bool(torch.isfinite(clean).all())
    for bad in (math.nan, math.inf):
        for row, pos in ((1, tile + 5), (1, 0), (2, x.shape[-1] - 1)):
            xb = x.clone()
            xb[row, pos] = bad
            got = fx().true_peak_linear(xb.to(DEV), FS[up], oversample=up, taps=h)
            assert not bool(torch.isfinite(got[row])) and (bad != bad) <= bool(torch.isnan(got[row])), (bad, row, pos)
            others = [r for r in range(3) if r != row]
            assert torch.equal(got[others], clean[others]), (bad, row, pos)
