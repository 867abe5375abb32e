"""Every planted case of tests/riccati_cases.py is the edge it claims to be - shown with the CPU oracle alone, so tests/test_gpu_batch_riccati.py compares
the device against cases that are known to exercise what they are named after."""
import numpy as np
import pytest

import batch_scenarios as bs
import riccati_cases as rc
from oracle_binding import OracleFilter
from util import imu_selection, rel_fro

CHARTS = ["euclid", "invdepth"]


@pytest.mark.parametrize("chart", CHARTS)
def test_sizes_and_sample_counts_are_covered(chart):
    _, _, cases = rc.cases(chart)
    assert {sc.N for sc in cases} >= {0, 1, 40, 64}
    assert {len(sc.imus) for sc in cases if not rc.is_long(sc) and "zero_dt" not in sc.name} >= {1, 2, 10}
    for sc in cases:
        dts = imu_selection(sc.imus, sc.t0, sc.stamp)[0]
        if "zero_dt" in sc.name:
            assert len(dts) == 3 and dts[0] > 0 and dts[1] == 0.0 and dts[2] > 0, dts
        elif rc.is_long(sc):
            assert len(dts) == 2 and np.allclose(dts, rc.DT_LONG)
            assert np.all(np.linalg.norm(sc.imus[:, 1:4], axis=1) > 1.0)  # a few rad/s
        else:
            assert np.allclose(dts, rc.DT), (sc.name, dts)


@pytest.mark.parametrize("chart", CHARTS)
def test_norm_edge(chart):
    """|dt [A B]|_inf at every sample's X, from the oracle's matrices: at most 0.25 (no squaring) for the dt = 0.005 cases, at least 1 for the long steps"""
    _, so, cases = rc.cases(chart)
    for sc in cases:
        _, norms = rc.walk(so, sc)
        assert len(norms) == rc.expected_samples(sc)
        print(f"{sc.name}: |dt [A B]|_inf {np.round(norms, 4)}")
        if rc.is_long(sc):
            assert min(norms) >= 1.0, (sc.name, norms)
        else:
            assert max(norms) <= rc.NORM_EDGE, (sc.name, norms)


@pytest.mark.parametrize("chart", CHARTS)
def test_accurate_is_not_fast(chart):
    """the oracle with fastRiccati = 0 and with fastRiccati = 1 differ by more than 1e-6 relative in Sigma wherever there is a landmark: a fast step cannot
    pass for an accurate one. Shown on the propagation alone and on the whole frame."""
    s, so, cases = rc.cases(chart)
    for sc in cases:
        acc, _ = rc.walk(so, sc)
        fast, _ = rc.walk(s, sc, accurate=False)
        d = rel_fro(fast.get_sigma(), acc.get_sigma())
        print(f"{sc.name}: propagation alone, fast against accurate {d:.2e}")
        if sc.N > 0:
            assert d > 1e-6, (sc.name, d)
        full = []
        for st in (so, s):
            orc = OracleFilter(st)
            orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
            for u in sc.imus:
                orc.process_imu(u)
            orc.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
            full.append(orc)
        assert np.array_equal(full[0].get_eqf()[2], full[1].get_eqf()[2])
        d = rel_fro(full[1].get_sigma(), full[0].get_sigma())
        print(f"{sc.name}: whole frame, fast against accurate {d:.2e}")
        if sc.N > 0:
            assert d > 1e-6, (sc.name, d)
        # the walk is the filter's own propagation: the whole frame of the empty measurement is the walk
        po = rc.propagation_only(sc)
        keep = rc.oracle_settings(bs.shipped_euroc(coordinateChoice=s.coordinateChoice, removeLostLandmarks=0))
        orc = OracleFilter(keep)
        orc.set_eqf(*po.state, po.Sigma, time=po.t0)
        for u in po.imus:
            orc.process_imu(u)
        orc.process_vision(po.stamp, po.cam, po.mid, po.y)
        assert np.array_equal(orc.get_sigma(), acc.get_sigma()), sc.name


@pytest.mark.parametrize("chart", CHARTS)
def test_turnover_and_outlier_cases(chart):
    _, so, cases = rc.cases(chart)
    by = {sc.name.split("_", 1)[1]: sc for sc in cases}
    d = bs.describe(so, by["turnover"])
    assert len(d["lost"]) == 5 and len(d["new"]) == 5 and not d["discarded"], d
    assert d["flags"] == bs.REMOVED_OLD | bs.ADDED | bs.UPDATED
    assert len(d["ids_after"]) == 40
    d = bs.describe(so, by["outliers"])
    assert len(d["discarded"]) == 2 and d["distinct"], d
    assert d["flags"] == bs.REMOVED_OUTLIERS | bs.UPDATED
