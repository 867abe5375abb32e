"""Every planted case of tests/nonfinite_cases.py is what its label says - shown with the CPU oracle alone, so tests/test_gpu_nonfinite.py compares the device's
EQF_OPT_CHECK_FINITE with the reference's hasNaN() behind the same call and not with itself - and the set of cases is the one the option needs."""
import numpy as np
import pytest

import nonfinite_cases as nc


@pytest.mark.parametrize("case", nc.CASES, ids=lambda c: c.id)
def test_label_is_the_oracles_verdict(case):
    """not np.all(np.isfinite(Sigma)) of the oracle's Sigma behind the call, on the planted Sigma. (A measured landmark's variance: the reference's LU inverse
    never refuses, its Sigma is not finite afterwards - the device may refuse earlier, with either code.)"""
    verdict = nc.oracle_verdict(case)
    assert verdict == ("clean" if nc.label(case) == "clean" else "reported"), (case.id, verdict)


def test_planted_entries_are_where_the_names_say():
    for case in nc.REPORTED:
        S, P = nc.inputs(case).S, nc.planted_sigma(case)
        assert np.all(np.isfinite(S)) and np.array_equal(S, S.T)
        bad = sorted((int(r), int(c)) for r, c in zip(*np.nonzero(~np.isfinite(P))))
        assert bad == nc.entries(case) and bad, case.id
        assert all(P[r, c] == nc.VALUES[case.value] or (case.value == "nan" and np.isnan(P[r, c])) for r, c in bad)
        assert {(c, r) for r, c in bad} == set(bad)  # symmetric
        n = case.n
        where = {"sensor_diag": [(3, 3)], "sensor_offdiag": [(2, 17), (17, 2)], "first_lm": [(21, 21)], "last_diag": [(n - 1, n - 1)], "last_row_first_col": [(0, n - 1), (n - 1, 0)],
                 "row_255": [(255, 255)], "row_256": [(256, 256)], "row_257": [(257, 257)]}
        if case.position in where:
            assert bad == where[case.position], case.id
    assert all(np.array_equal(nc.planted_sigma(c), nc.inputs(c).S) and nc.entries(c) == [] for c in nc.TWINS)


def test_an_update_case_plants_where_the_factorisation_does_not_read():
    """the update reads the columns of the measured landmarks only: no planted entry of a "reported" update case lies in one of them (rows or columns, Sigma is
    symmetric), its two unmeasured landmarks are the last two, and the look-ahead / chain cases are what lookahead_fits says."""
    seen = set()
    for case in nc.REPORTED:
        if case.call not in nc.UPDATES:
            continue
        meas = nc.measured(case)
        cols = {21 + 3 * i + k for i in meas for k in range(3)}
        hit = [e for e in nc.entries(case) if e[0] in cols or e[1] in cols]
        if case.position == "measured_diag":
            assert hit and nc.label(case) == "nonzero"
        else:
            assert not hit and nc.label(case) == "reported", case.id
        assert len(nc.inputs(case).mid) == len(meas)
        if case.N >= 78:
            assert not set(nc.unmeasured(case.N)) & set(meas)
            assert nc.update_form(case) == {"update_la": "lookahead", "update_chain": "chain"}[case.call]
            assert len(meas) >= 33 if case.call == "update_la" else len(meas) <= 16
            seen.add(nc.update_form(case))
        else:
            assert nc.update_form(case) == "chain"
    assert seen == {"lookahead", "chain"}


def test_required_cases_are_present():
    have = {(c.chart, c.N, c.call, c.value, c.position, c.fp32) for c in nc.REPORTED}
    charts = lambda N, call, value, pos, fp32=0: {ch for ch in nc.CHART_NAMES if (ch, N, call, value, pos, fp32) in have}
    assert {c.N for c in nc.CASES} == set(nc.SIZES) and [21 + 3 * N for N in nc.SIZES] == [24, 255, 258, 279]
    # every call x NaN x three positions at N = 79
    for call in nc.CALLS:
        for pos in ("sensor_diag", "last_diag", "last_row_first_col"):
            assert {"invdepth", "euclid"} <= charts(79, call, "nan", pos), (call, pos)
            if call in nc.PROPAGATIONS:
                assert "normal" in charts(79, call, "nan", pos)
    # every position x every value for fast and accurate at N = 79
    for call in ("fast", "accurate"):
        for pos in nc.POSITIONS:
            for value in nc.VALUES:
                assert charts(79, call, value, pos), (call, pos, value)
    # the row edges at the three sizes, where n allows
    for N, rows in ((78, ()), (79, nc.ROW_EDGES), (86, nc.ROW_EDGES)):
        assert {c.position for c in nc.REPORTED if c.N == N and c.call == "fast" and c.position in nc.ROW_EDGES} == set(rows)
    assert charts(78, "fast", "nan", "last_diag") and charts(78, "fast", "nan", "last_row_first_col")
    assert not nc.allowed(78, "row_255") and nc.allowed(79, "row_257") and 257 == 21 + 3 * 79 - 1 and 257 < 21 + 3 * 86 - 1
    # N = 1 for every call
    assert {c.call for c in nc.REPORTED if c.N == 1} == set(nc.CALLS)
    # the float stores
    for mode in nc.FP32_MODES:
        for call in ("fast",) + nc.UPDATES:
            assert charts(79, call, "nan", "last_diag", mode), (mode, call)
    # the measured landmark: both forms of the update
    assert {c.call for c in nc.REPORTED if c.position == "measured_diag"} == set(nc.UPDATES)


def test_every_reported_case_has_its_clean_twin():
    ids = [c.id for c in nc.CASES]
    assert len(ids) == len(set(ids))
    for case in nc.REPORTED:
        t = case.twin()
        assert t in nc.TWINS and t.seed == case.seed and nc.label(t) == "clean"
        a, b = nc.inputs(case), nc.inputs(t)
        assert a is b  # the same state, Sigma, IMU sample and measurement
    assert all(c.value == "none" for c in nc.TWINS) and all(c.value != "none" for c in nc.REPORTED)
    print(f"{len(nc.REPORTED)} planted cases, {len(nc.TWINS)} clean twins")
