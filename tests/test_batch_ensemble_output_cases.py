"""The planted cases of tests/batch_ensemble_output_cases.py, proved on the CPU with the restatement alone: every resampling case the device tests use keeps
every comparison of weightedResample at least MARGIN = 1e-9 away from going the other way - the project's condition under which device and sequential indices
must agree - with the uniforms eqf_bens_resample_weighted_seeded is defined by, and is not a collapsed cloud; the planted underflow case underflows; the sizes
cover what the kernels' edges ask for. No case is skipped."""
import numpy as np
import pytest

from batch_ensemble_output_cases import (COV_CASES, FIVE, MARGIN, MAXP, OTHERS, PLANTED_UNDERFLOW, RESAMPLE, SEED, SIZES_M, SIZES_P, SMALL_M, STAT_STREAM, likelihood_cases,
                                         loglik_at, res_key, resample_case)
from ensemble_output_cases import get_case, log_weights, margin, stat_case
from ensemble_random_cases import cached_uniforms

# (margin, distinct sources) of every case as first checked with the restatement, seed 2026: a record, asserted within 1 % / exactly
SEEN = {(0, 2, 33, 33, 1, 400.0): (9.5e-5, 23), (1, 11, 257, 257, 2, 4000.0): (1.5e-5, 207), (1, 2, 257, 300, 5, 400.0): (1.3e-6, 160),
        (0, 2, 255, 256, 8, 400.0): (1.4e-6, 165), (0, 11, 16, 17, 10, 4000.0): (2.0e-4, 13), (0, 5, 257, 1, 4, 400.0): (2.0e-3, 1), (2, 1, 1, 33, 3, 4.0): (2.5e-2, 1),
        (2, 62, 31, 31, 7, 40000.0): (6.3e-4, 29)}


@pytest.mark.parametrize("case", RESAMPLE, ids=[res_key(*r) for r in RESAMPLE])
def test_resampling_case_has_the_margin_and_is_not_collapsed(case):
    rc = resample_case(*case)
    cam, M, P, Pn, stream, var = case
    distinct = len(set(rc.src.tolist()))
    print(f"[batch ensemble output case] {res_key(*case)} margin {rc.margin:.2e} distinct sources {distinct} ess {1.0 / np.sum(rc.w ** 2):.1f}")
    assert rc.margin >= MARGIN
    assert abs(rc.margin - SEEN[case][0]) <= 0.05 * SEEN[case][0] and distinct == SEEN[case][1]
    assert P <= MAXP and Pn <= MAXP and M + 2 <= 64
    assert len(rc.u) == Pn and np.all((rc.u > 0.0) & (rc.u < 1.0))
    assert rc.src.min() >= 0 and rc.src.max() <= P - 1
    # not a collapsed cloud: where there is anything to choose from, the effective sample size is above a third of the cloud and most particles are distinct
    if P > 1:
        assert 1.0 / np.sum(rc.w ** 2) >= P / 3.0
    if P > 1 and Pn > 1:
        assert distinct >= min(P, Pn) // 2


def test_the_capacity_case_is_among_them_and_the_call_of_five_uses_proved_cases():
    assert any(r[1] == 62 for r in RESAMPLE)
    for slot, key, var, Pn, stream in FIVE + OTHERS:
        assert (*key, Pn, stream, var) in RESAMPLE, (slot, key)
    assert sorted(s for s, *_ in FIVE + OTHERS) == list(range(7))


def test_planted_underflow_sums_to_zero_in_the_plain_formula():
    cam, M, P, var = PLANTED_UNDERFLOW
    c = get_case(cam, M, P)
    q = -2.0 * loglik_at(c, var)
    with np.errstate(under="ignore"):
        assert np.exp(-0.5 * q).sum() == 0.0  # the reference's weights: 0 / 0
    w, lse, ess = log_weights(loglik_at(c, var))
    assert np.all(np.isfinite(w)) and abs(w.sum() - 1.0) <= 1e-12 and np.isfinite(lse) and ess >= 1.0


def test_sizes_cover_the_kernels_edges():
    cases = likelihood_cases()
    assert {c[0] for c in cases} == {0, 1, 2}
    assert {c[1] for c in cases} == set(SIZES_M) and {c[2] for c in cases} == set(SIZES_P)
    for cam in range(3):
        assert {c[1] for c in cases if c[0] == cam} == set(SIZES_M)  # every M with every camera
    assert all(c[1] in SMALL_M for c in cases if c[2] == 513) and all(c[1] + 2 <= 64 for c in cases)
    assert len(set(cases)) == len(cases) and len(set(COV_CASES)) == len(COV_CASES)


def test_statfixture_output_check_has_the_margin_with_seeded_uniforms():
    c = stat_case()
    u = cached_uniforms(SEED, STAT_STREAM, c.P)
    m = margin(c.weights[0], u)
    print(f"[batch ensemble output case] StatFixture N=2 P=1000 stream {STAT_STREAM} margin {m:.2e}")
    assert m >= MARGIN
