"""The planted cases of tests/ensemble_cases.py are what they claim - proved by the restatement (oracle/indep/eqvio_ref.py, numpy) and the CPU oracle alone,
no device involved. These are the conditions the flat bounds of tests/test_gpu_ensemble.py rest on."""
import json

import numpy as np
import pytest

from ensemble_cases import (BASELINE_PATH, CHART_NAMES, R, STAT_BANDS, STAT_SEEDS, case_key, get_case, load_baseline, restated_statistics, size_cases)
from oracle_binding import OracleFilter
from util import settings_for

CASES = size_cases()
IDS = [case_key(*c) for c in CASES]


def test_sizes_cover_every_edge():
    assert {c[1] for c in CASES} == {0, 1, 2, 4, 11, 70}
    for chart in range(3):
        assert {c[2] for c in CASES if c[0] == chart} == {1, 2, 31, 32, 33, 257}
        assert {c[1] for c in CASES if c[0] == chart} == {0, 1, 2, 4, 11, 70}


@pytest.mark.parametrize("chart,N,P", CASES, ids=IDS)
def test_case_conditions(chart, N, P):
    c = get_case(chart, N, P)
    assert np.array_equal(c.Sigma, c.Sigma.T)
    assert np.linalg.cond(c.Sigma) <= 1e8
    sens, pts = c.sampled
    assert np.all(np.isfinite(sens)) and np.all(np.isfinite(pts))
    assert np.all(pts[:, :, 2] > 0), "a sampled depth is not positive"
    assert np.all(c.nees_restated > 0)
    # the truth the device gets differs from the filter's landmark list: two more ids, another order
    ids, _, p = c.truth_x
    assert len(ids) == N + 2 and p.shape == (P, N + 2, 3) and len(set(ids.tolist())) == N + 2
    if N > 1:
        assert list(ids[:N]) != list(c.ids)


@pytest.mark.parametrize("chart,N,P", [c for c in CASES if c[2] <= 33 and c[1] <= 11], ids=[case_key(*c) for c in CASES if c[2] <= 33 and c[1] <= 11])
def test_restated_nees_is_the_oracles(chart, N, P):
    """the one-solve formula of the cases against compute_nees of the restatement and of the CPU oracle, per particle (1e-9 relative, test_compute_nees' bound)"""
    c = get_case(chart, N, P)
    ids, sens, p = c.truth_x
    orc = OracleFilter(settings_for(chart))
    orc.set_eqf(c.xi0f, c.Xsf, c.ids, c.q0, c.Q, c.Sigma)
    for k in range(P):
        a = float(R.compute_nees(c.kind, c.X, c.xi0, c.Sigma, R.sensor_from_flat(sens[k]), ids, p[k]))
        b = orc.compute_nees(sens[k], ids, p[k])
        assert abs(a - c.nees_restated[k]) <= 1e-9 * abs(a)
        assert abs(b - c.nees_restated[k]) <= 1e-9 * abs(b)


def test_identity_baseline_file_is_current():
    """tests/golden/ensemble_identity_baseline.json: per case what the restatement loses on NEES(sampled particle) = |xi|^2 / n. The device test allows ten times
    that (floor 1e-12); here the file must hold every case, every entry must be a rounding-level figure (the conditions above put it below 1e-11), and the
    restatement on THIS machine - another BLAS may sum in another order - must itself pass the bound the device is held to."""
    base = load_baseline()
    assert sorted(base) == sorted(IDS)
    for c in CASES:
        have, now = base[case_key(*c)], get_case(*c).identity_baseline
        assert np.isfinite(have) and 0 <= have < 1e-11, (case_key(*c), have)
        assert now <= max(10.0 * have, 1e-12), (case_key(*c), have, now)
    assert json.load(open(BASELINE_PATH)) == base


@pytest.mark.parametrize("N,P,check", [(2, 1000, "initial"), (2, 1000, "true_input"), (2, 1000, "random_input"), (2, 1000, "output"), (40, 256, "initial"), (40, 256, "true_input")])
def test_restated_statistics_stay_inside_half_the_band(N, P, check):
    """the reference's four checks with the restatement and the CPU oracle: the planted seeds leave half of each band (0.1 / 1.0 / 0.1 / 0.5) to the device"""
    vals = restated_statistics(N, P, check, STAT_SEEDS[(N, check)])
    assert len(vals) == (5 if check.endswith("input") else 1)
    for v in vals:
        assert abs(v - 1.0) <= 0.5 * STAT_BANDS[check], (check, vals)


def test_chart_names_follow_the_enum():
    from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL

    assert (CHART_NAMES[COORD_EUCLIDEAN], CHART_NAMES[COORD_INVDEPTH], CHART_NAMES[COORD_NORMAL]) == ("euclid", "invdepth", "normal")
