"""The planted cases of tests/riccati_cases.py serve the discrete-state-matrix mode of the filter batch - shown with the CPU oracle and oracle/indep alone, so
tests/test_gpu_batch_discrete.py compares the device against cases on which the third propagation is told apart from the other two, against an oracle whose
filter takes that propagation, within bounds that leave room for the reference's own differencing noise."""
import os
import sys

import numpy as np
import pytest

import batch_scenarios as bs
import discrete_cases as dc
import riccati_cases as rc
from oracle_binding import OracleFilter
from util import imu_selection, rel_fro

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "indep"))
from eqvio_ref import Camera as RCam  # noqa: E402
from eqvio_ref import F64, EqVIORef  # noqa: E402

CHARTS = ["euclid", "invdepth"]


@pytest.mark.parametrize("chart", CHARTS)
def test_discrete_is_neither_accurate_nor_fast(chart):
    """(a) wherever there is a landmark the oracle's discrete walk differs from its accurate and from its fast walk by more than 1e-6 relative in Sigma, on the
    propagation alone and on the whole frame: neither existing call can pass for the new one."""
    s, so, cases = rc.cases(chart)
    sd = dc.oracle_settings(s)
    for sc in cases:
        walks = {m: dc.walk(sd if m == "discrete" else so if m == "accurate" else s, sc, m).get_sigma() for m in ("discrete", "accurate", "fast")}
        full = {m: dc.whole_frame(st, sc) for m, st in (("discrete", sd), ("accurate", so), ("fast", s))}
        for other in ("accurate", "fast"):
            d = rel_fro(walks[other], walks["discrete"])
            assert np.array_equal(full[other].get_eqf()[2], full["discrete"].get_eqf()[2]), sc.name
            df = rel_fro(full[other].get_sigma(), full["discrete"].get_sigma())
            print(f"{sc.name}: discrete against {other}: propagation alone {d:.2e}, whole frame {df:.2e}")
            if sc.N > 0:
                assert d > 1e-6 and df > 1e-6, (sc.name, other, d, df)


@pytest.mark.parametrize("chart", CHARTS)
def test_filter_with_discrete_state_matrix_is_the_walk(chart):
    """(b) the oracle's filter with fastRiccati = 0, useDiscreteStateMatrix = 1 on the propagation-only form of a case equals the walk by
    integrate_riccati_discrete / integrate_observer calls, bit for bit"""
    s, _, cases = rc.cases(chart)
    keep = dc.oracle_settings(bs.shipped_euroc(coordinateChoice=s.coordinateChoice, removeLostLandmarks=0))
    for sc in cases:
        po = rc.propagation_only(sc)
        orc = dc.whole_frame(keep, po)
        walked = dc.walk(keep, sc)
        assert np.array_equal(orc.get_sigma(), walked.get_sigma()), sc.name
        for a, b in zip(orc.get_eqf(), walked.get_eqf()):
            assert np.array_equal(a, b), sc.name


def _state_dist(a, b):
    """largest absolute difference of two flat 23-vectors (quaternion signs aligned) or Q arrays"""
    a = np.array(a, float).copy()
    if a.ndim == 1:
        for sl in (slice(6, 10), slice(16, 20)):
            if np.dot(a[sl], b[sl]) < 0:
                a[sl] = -a[sl]
    else:
        a[:, :4] *= np.sign(np.sum(a[:, :4] * b[:, :4], axis=1))[:, None]
    return float(np.abs(a - b).max()) if a.size else 0.0


@pytest.mark.parametrize("chart", CHARTS)
def test_two_cpu_restatements_agree_within_the_bounds(chart):
    """(c) oracle/*.hpp and oracle/indep/eqvio_ref.py, X teacher forced (every sample starts from the oracle's X), Sigma free over the walk, then the vision
    update of the landmarks the frame measures: within 5e-9 in Sigma on every case. The bounds of tests/test_gpu_batch_discrete.py (5e-9 for at most two
    samples, 1e-8 beyond) leave room for the reference's own noise."""
    s, _, cases = rc.cases(chart)
    sd = dc.oracle_settings(s)
    r = EqVIORef(F64())
    kind = chart
    worst_walk = worst_upd = worst_state = 0.0
    for sc in cases:
        xi0, Xs, ids, q0, Q = sc.state
        N = len(ids)
        orc = OracleFilter(sd)
        orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
        st = r.state_from_flat(xi0, ids, q0)
        Qin, P = r.diag(sd.input_gain_diag12()), r.state_gain(sd.state_gain_diag8(), N)
        S = np.array(sc.Sigma, float)
        dts = imu_selection(sc.imus, sc.t0, sc.stamp)[0]
        for u, dt in zip(sc.imus, dts):
            _, Xo, _, _, Qo = orc.get_eqf()
            X = r.group_from_flat(Xo, ids, Qo)
            if dt > 0:
                S = r.riccati_discrete(kind, X, st, S, r.imu_from_flat(u), dt, Qin, P)
                orc.integrate_riccati_discrete(u, dt)
            orc.integrate_observer(u, dt, bool(sd.useDiscreteVelocityLift))
        d = rel_fro(S, orc.get_sigma())
        worst_walk = max(worst_walk, d)
        assert d <= dc.TOL_SHORT, (sc.name, d)
        # the update of the landmarks the frame measures, each side from its own Sigma
        have = [j for j, i in enumerate(sc.mid) if int(i) in set(ids.tolist())]
        if not have:
            continue
        mid, y = sc.mid[have], sc.y.reshape(-1, 2)[have].reshape(-1)
        _, Xo, _, _, Qo = orc.get_eqf()
        X = r.group_from_flat(Xo, ids, Qo)
        cam = RCam(sc.cam.model, sc.cam.fx, sc.cam.fy, sc.cam.cx, sc.cam.cy, list(sc.cam.dist))
        X2, S2, _ = r.vision_update(kind, X, st, S, cam, r.meas_from_flat(mid, y), sd.measurementNoise**2, bool(sd.useEquivariantOutput), bool(sd.useDiscreteInnovationLift))
        orc.vision_update(sc.cam, mid, y)
        _, Xs2, _, _, Q2 = orc.get_eqf()
        Xf, Qf = r.group_to_flat(X2)
        du, dx = rel_fro(S2, orc.get_sigma()), max(_state_dist(Xf, Xs2), _state_dist(Qf, Q2))
        print(f"{sc.name}: walk {d:.2e}, after the update Sigma {du:.2e}, state {dx:.2e}")
        worst_upd, worst_state = max(worst_upd, du), max(worst_state, dx)
        assert du <= dc.TOL_SHORT and dx <= dc.TOL_SHORT, (sc.name, du, dx)
    print(f"{chart}: oracle against oracle/indep: walk {worst_walk:.2e}, update Sigma {worst_upd:.2e}, state {worst_state:.2e}")
