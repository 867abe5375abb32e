"""The planted cases of tests/ensemble_output_cases.py, proved on the CPU with the restatement alone (oracle/indep's measure, the log-sum-exp weights, the
sequential weightedResample loop): the conditions tests/test_gpu_ensemble_output.py leans on hold for every case, and the reason for the feature is pinned -
at M = 70 the reference's plain exp(-q / 2) sums to exactly 0.0 while the log-domain weights are finite and sum to 1."""
import numpy as np
import pytest

from ensemble_output_cases import MARGIN_CPU, case_key, get_case, log_weights, running_sums, size_cases, stat_case, weighted_resample

CASES = size_cases()
IDS = [case_key(*c) for c in CASES]


def all_cases():
    return [get_case(*c) for c in CASES] + [stat_case()]


def test_the_grid_covers_every_size_and_camera():
    assert {c[1] for c in CASES} == {0, 1, 2, 11, 70}
    assert {c[2] for c in CASES} == {1, 2, 31, 32, 33, 257}
    for cam in range(3):
        assert sorted(c[1] for c in CASES if c[0] == cam) == [0, 1, 2, 11, 70]
    s = stat_case()
    assert (s.N, s.P, s.M) == (2, 1000, 2)


@pytest.mark.parametrize("cam,M,P", CASES, ids=IDS)
def test_case_conditions(cam, M, P):
    c = get_case(cam, M, P)
    assert c.p.shape == (P, M + 2, 3) and len(c.ids) == M + 2 and len(set(c.ids.tolist())) == M + 2
    assert np.all(c.p[:, :, 2] > 0), "a depth is not positive"
    assert not np.array_equal(c.mids, c.ids[:M]) or M < 2, "the measurement is in the ensemble's order"
    w, lse, ess = c.weights
    assert np.all(np.isfinite(w)) and abs(w.sum() - 1.0) <= 1e-13
    assert np.isfinite(lse) and 1.0 - 1e-12 <= ess <= P + 1e-9
    print(f"[output case] {case_key(cam, M, P)} exponents {(-0.5 * c.quad).min():.1f} .. {(-0.5 * c.quad).max():.1f} ess {ess:.3f} margin {c.margin:.2e}")
    assert c.margin >= MARGIN_CPU
    if M == 0:
        assert np.all(c.loglik == 0.0) and np.all(w == 1.0 / P)


def test_statfixture_case_conditions():
    c = stat_case()
    assert np.all(c.p[:, :, 2] > 0)
    w, _, ess = c.weights
    print(f"[output case] StatFixture N=2 P=1000 ess {ess:.2f} margin {c.margin:.2e}")
    assert c.margin >= MARGIN_CPU
    # the log-domain weights choose what the fixture's own plain-exp route chooses
    assert np.array_equal(c.src, c.fixture.resample_indices(c.sensor, c.p))


@pytest.mark.parametrize("cam,M,P", [c for c in CASES if c[1] == 70], ids=[case_key(*c) for c in CASES if c[1] == 70])
def test_plain_exp_underflows_at_M70_and_the_log_domain_does_not(cam, M, P):
    c = get_case(cam, M, P)
    plain = np.exp(-0.5 * c.quad)
    assert plain.sum() == 0.0, "the reference's plain sum is not exactly 0.0"
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.all(np.isnan(plain / plain.sum()))
    w, lse, _ = c.weights
    assert np.all(np.isfinite(w)) and abs(w.sum() - 1.0) <= 1e-13 and np.isfinite(lse)
    assert (-0.5 * c.quad).max() < -745.2  # log of the smallest denormal


def test_binary_search_rule_is_the_sequential_loop():
    """src_k = min{ j : cum_j >= thr_k }, capped at P - 1, on the loop's own running sums is what the loop returns"""
    for c in all_cases():
        w = c.weights[0]
        cum = running_sums(w)
        thr = (c.u + np.arange(len(c.u))) / len(c.u)
        first = np.minimum(np.searchsorted(cum, thr, side="left"), c.P - 1)
        assert np.array_equal(first.astype(np.int32), c.src)
    # P_new != P, a zero weight, and no running sum reaching the threshold
    w = np.array([0.25, 0.0, 0.5, 0.25])
    assert weighted_resample(w, np.array([0.5])).tolist() == [2]
    assert weighted_resample(w, np.full(8, 0.5)).tolist() == [0, 0, 2, 2, 2, 2, 3, 3]
    assert weighted_resample(np.array([0.5, 0.25]), np.array([0.9])).tolist() == [1]


def test_non_finite_counts_as_minus_infinity():
    w, lse, ess = log_weights(np.array([-3.0, np.nan, -3.0, -np.inf]))
    assert w.tolist() == [0.5, 0.0, 0.5, 0.0] and ess == 2.0 and abs(lse - (-3.0 + np.log(2.0))) < 1e-15
