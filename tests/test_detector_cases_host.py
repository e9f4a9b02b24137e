"""The detector tests' cases without a GPU (tests/detector_cases.py): the table against the host-only plan functions of the C
ABI, the coverage the GPU tests rely on -- computed from the float64 references on the very signals and seeds they use -- and the
CPU path of limit() with every case's taps against the per-position bound.  This pins the cases and the reference before anything
runs on a device."""
import pytest
import torch

from tests import detector_cases as D

IDS = [D.case_id(c) for c in D.CASES]
DT = pytest.mark.parametrize("dtype", D.DTYPES, ids=["f32", "f64"])


@DT
def test_the_table_is_what_the_plans_say(dtype):
    for c in D.CASES:
        for A, H in ((1, 1), (5, 7), (72, 480)):
            g = D.check(c, dtype, A, H)
            assert g["history"] == g["latency"] + A + H - 2 + max(1, c.Lp - c.i_lo), (c, A, H, g)
            assert g["halo_left"] == A + H - 1 + c.bucket - 1 - c.i_lo and g["halo_right"] == A + c.i_lo
        assert D.geometry(c.up, c.nh, dtype)["tile"] == 8190 and D.LIMITER_T == 2 * 8190 + 3


def test_every_bucket_and_every_phase_split_has_a_case():
    full = [D.CASES[k] for k in D.FULL]
    for up in (2, 4, 8):
        assert {c.bucket for c in full if c.up == up} == set(D.BUCKETS), up       # every bucket at every factor
    rems = {up: {c.rem for c in full if c.up == up} for up in (2, 4, 8)}
    assert rems[2] == {0, 1} and rems[4] == {0, 1, 2, 3}
    assert {0, 1, 7} <= rems[8] and rems[8] & {2, 3, 4, 5, 6}
    assert {0} < {c.rem for c in full if c.bucket == 64} and max(c.rem for c in full if c.bucket == 64) >= 2
    assert {c.rem for c in full if c.bucket == 72} == {0}
    assert [D.CASES[k].Lp for k in D.SINGLE_TAP] == [2, 2] and len(D.FULL) == 26


def test_bucket_72_has_no_lo_phases():
    """Lp = 65 needs nh = 64 * up, whose n_pre_remove = 32 * up: bucket 72 exists with rem = 0 only."""
    for up in (2, 4, 8):
        for nh in range(1, 64 * up + 1):
            g = D.geometry(up, nh)
            assert (g["bucket"] == 72) == (nh == 64 * up), (up, nh, g)
            assert g["bucket"] < 72 or g["rem"] == 0
            assert g["latency"] == g["i_lo"] + (g["rem"] >= 2)


@DT
@pytest.mark.parametrize("k", D.FULL, ids=[IDS[k] for k in D.FULL])
def test_the_limiter_signal_shows_every_candidate(k, dtype):
    """In group 0 of the limiter's signal the maximum p[i] is an interpolator output at 90 % of the positions or more, and for
    every residue i mod 16 the sample, each of the up outputs of position i and each of position i - 1 owns it somewhere."""
    c = D.CASES[k]
    x, link = D.limiter_signal(k, dtype)
    cand = D.candidates(D.grouped(x, link)[0], D.taps(c, dtype).numpy(), c.up)
    share, missing = D.share_and_coverage(cand, c.up)
    print(D.case_id(c), "scale %g seed %d: an interpolator output owns p at %.2f %%" % (c.scale, c.seed, 100 * share))
    assert share >= 0.9 and not missing, (share, missing)
    assert float(cand.max(0).max(-1).min()) > 1.0                     # p > c everywhere: the gain shows every p[i]


@DT
@pytest.mark.parametrize("k", D.FULL, ids=[IDS[k] for k in D.FULL])
def test_the_true_peak_rows_give_every_cell_a_maximum(k, dtype):
    c = D.CASES[k]
    rows = D.truepeak_rows(k, dtype)
    h = D.taps(c, dtype, scaled=False).numpy()
    cov = {}
    for name, x in rows.items():
        _, P, ph, _ = D.truepeak_reference(c, x, h, wide=False)
        cov[name] = D.cell_coverage(c, P, ph, x.shape[-1])
    D.assert_truepeak_coverage(c, cov)
    assert len(rows["short"]) + len(rows["long"]) <= 1500


@DT
@pytest.mark.parametrize("k", range(len(D.CASES)), ids=IDS)
def test_the_cpu_path_meets_the_bound_at_every_position(k, dtype):
    """_limit_host multiplies and adds where the definition has one fma: (2A + 4) u = 6 u in place of the device's 2 u."""
    from torchfx_amd.limiter import limit
    c = D.CASES[k]
    st = D.limiter_statement(k, dtype)
    y, g = limit(torch.from_numpy(st["x"].copy()), D.FS, link=st["link"], return_gain=True, **D.limiter_kwargs(c, dtype))
    eg, ey = D.limiter_errors(st, g.numpy(), y.numpy(), dtype, 6 * D.U[dtype])
    print(D.case_id(c), dtype, "g err / tol %.3f, y err / tol %.3f" % (eg, ey))
    assert eg <= 1.0 and ey <= 1.0, (eg, ey)
    assert float(g.max()) < 0.9
