"""The single-filter context path (EqfCore) against the CPU oracle on BOTH sides of every size at which it switches kernels, and above 512 landmarks
(context_scenarios.py; the CPU half is test_context_scenarios.py). Every scenario and route is held to the project's existing bounds - flat 1e-9 on the state
(check_state) and on Sigma (relative Frobenius), identical ids, identical outlier decisions, the outlier statistics to test_outlier_stats' bound - and the device's
own counters must name the form on the scenario's label with no stalled look-ahead launch. The Riccati modes and NEES, so far compared at toy sizes only, are
compared at size with the tolerance of their small-size tests. Serial, short-lived contexts, nothing here stalls or faults a kernel on purpose."""
import numpy as np
import pytest

import context_scenarios as cs
from eqvio_amd.capi import OPT_RICCATI_DENSE, EqfCore
from oracle_binding import OracleFilter, se3_log_dist
from test_gpu_parity import TOL, check_sigma, check_state, make_pair
from util import CHARTS, random_imu, random_spd, reasonable_state, rel_fro, settings_for

pytestmark = pytest.mark.gpu


class _Snapshot:
    """What check_state reads of a context or an oracle, from stored arrays"""

    def __init__(self, state, estimate):
        self._state, self._estimate = state, estimate

    def get_state(self):
        return self._state

    get_eqf = get_state

    def state_estimate(self):
        return self._estimate


def state_error(dev, orc):
    """The largest of check_state's quantities, each over its own scale (reported next to the assertion)"""
    (_, Xg, _, _, Qg), (sg, _, pg) = dev
    (_, Xo, _, _, Qo), (so, _, po) = orc
    e = [np.max(np.abs(Xg[0:6] - Xo[0:6])), se3_log_dist(Xg[6:13], Xo[6:13]) / max(1.0, np.linalg.norm(Xo[10:13])), se3_log_dist(Xg[16:23], Xo[16:23]),
         se3_log_dist(sg[6:13], so[6:13]) / max(1.0, np.linalg.norm(so[10:13]))]
    if len(po):
        sign = np.sign(np.sum(Qg[:, :4] * Qo[:, :4], axis=1))[:, None]
        e += [np.max(np.abs(Qg[:, :4] * sign - Qo[:, :4])), np.max(np.abs(Qg[:, 4] / Qo[:, 4] - 1)), np.max(np.linalg.norm(pg - po, axis=1) / np.maximum(1.0, np.linalg.norm(po, axis=1)))]
    return float(max(e))


def compare(sc, dev, orun):
    """Assertions of one scenario; returns (worst state error, worst Sigma error)"""
    worst_s = worst_S = 0.0
    assert len(dev.after) == sc.frames
    for f in range(sc.frames):
        (st_g, est_g, S_g), (st_o, est_o, S_o) = dev.after[f], orun.after[f]
        assert np.array_equal(st_g[2], st_o[2]), (sc.name, f)
        es, eS = state_error((st_g, est_g), (st_o, est_o)), rel_fro(S_g, S_o)
        print(f"{sc.name} frame {f}: state {es:.2e} Sigma {eS:.2e}")
        worst_s, worst_S = max(worst_s, es), max(worst_S, eS)
        assert S_g.shape == S_o.shape and np.all(np.isfinite(S_g))
        assert eS <= TOL, (sc.name, f, eS)
        check_state(_Snapshot(st_g, est_g), _Snapshot(st_o, est_o))
    return worst_s, worst_S


@pytest.mark.parametrize("name", [sc.name for sc in cs.SCENARIOS])
def test_scenario_against_the_oracle(name):
    sc = cs.BY_NAME[name]
    orun = cs.oracle_run(sc)
    dev = cs.run_device(sc, orun)
    c, want = dev.counters, sc.expected()
    print(f"{name}: N {sc.N} M {sc.M} NJ {sc.NJ} form {sc.form()} counters {c} oracle {orun.seconds:.1f} s")
    if sc.route != "update":
        assert dev.updated == [1] * sc.frames
    assert c["la_fallbacks"] == 0 and c["cancelled"] == 0
    for k, v in want.items():
        assert c[k] == v, (name, k, c, want)
    if sc.route == "select":
        ab, pr, disc = orun.candidates
        assert list(dev.removed) == disc and c["discarded"] == len(disc) == sc.cap
        a_o, p_o = orun.stats
        a_g, p_g, _ = dev.stats
        np.testing.assert_allclose(a_g, a_o, rtol=1e-11, atol=1e-11)  # test_outlier_stats' bounds
        np.testing.assert_allclose(p_g, p_o, rtol=1e-9, atol=1e-11)
    compare(sc, dev, orun)


@pytest.mark.parametrize("name", cs.LARGEST)
def test_largest_scenarios_repeat_bit_identically(name):
    sc = cs.BY_NAME[name]
    orun = cs.oracle_run(sc)
    a, b = cs.run_device(sc, orun), cs.run_device(sc, orun)
    assert a.counters == b.counters and a.counters["la_fallbacks"] == 0
    for (sa, ea, Sa), (sb, eb, Sb) in zip(a.after, b.after):
        assert np.array_equal(Sa, Sb)
        for u, v in zip(tuple(sa) + tuple(ea), tuple(sb) + tuple(eb)):
            assert np.array_equal(u, v)


# ------------------------------------------------------------------------------------------------ modes compared at toy sizes so far
@pytest.mark.parametrize("chart", list(CHARTS))
@pytest.mark.parametrize("N,dt", [(200, 0.005), (200, 0.7), (205, 0.02)])
def test_riccati_accurate_at_size(chart, N, dt):
    """test_riccati_accurate's comparison and tolerance (1e-11) with n = 621 (20 GEMM tiles a side, an edge tile of 13) and n = 636 (20 tiles, an edge of 28 - not a
    multiple of the 32-wide tile either); dt = 0.7 takes the scaling-and-squaring branch of the device exponential at size."""
    rng, settings, orc, core, _ = make_pair(CHARTS[chart], N, seed=3000 + N)
    Qd, Pd = settings.input_gain_diag12(), settings.state_gain_diag8()
    try:
        for rep in range(2):
            imu = random_imu(rng, bias_vel=True)
            orc.integrate_riccati_accurate(imu, dt)
            core.integrate_riccati_accurate(imu, dt, Qd, Pd)
            e = rel_fro(core.get_sigma(), orc.get_sigma())
            print(f"accurate {chart} N {N} dt {dt} rep {rep}: {e:.2e}")
            check_sigma(core, orc, 1e-11)
    finally:
        core.close()


@pytest.mark.parametrize("chart", list(CHARTS))
def test_riccati_discrete_at_size(chart):
    """test_riccati_discrete's comparison and tolerance (5e-9: the differencing's rounding noise) at N = 130"""
    N = 130
    rng, settings, orc, core, _ = make_pair(CHARTS[chart], N, seed=3300)
    try:
        for rep in range(2):
            imu = random_imu(rng, bias_vel=True)
            dt = float(rng.uniform(0.004, 0.02))
            core.integrate_riccati_discrete(imu, dt, settings.input_gain_diag12(), settings.state_gain_diag8())
            orc.integrate_riccati_discrete(imu, dt)
            e = rel_fro(core.get_sigma(), orc.get_sigma())
            print(f"discrete {chart} N {N} rep {rep}: {e:.2e}")
            assert e <= 5e-9, e
            core.integrate_observer(imu[None, :], np.array([dt]), True)
            orc.integrate_observer(imu, dt, True)
    finally:
        core.close()


@pytest.mark.parametrize("chart", list(CHARTS))
def test_riccati_dense_mode_at_size(chart):
    """test_riccati_dense_mode_matches_structured's comparison and tolerance (1e-12) at N = 300: the dense mode (k_build_F, two k_gemm_nt of 29 x 29 tiles with an
    edge of 25) against the oracle, and against the structured mode in its mirrored lower-triangle form"""
    N = 300
    rng, settings, orc, core, (xi0, Xs, ids, q0, Q, S) = make_pair(CHARTS[chart], N, seed=3400)
    twin = EqfCore(N, CHARTS[chart])
    try:
        twin.set_state(xi0, Xs, ids, q0, Q)
        twin.set_sigma(S)
        imu = random_imu(rng)
        orc.integrate_riccati_fast(imu, 0.04)
        core.set_option(OPT_RICCATI_DENSE, 1)
        core.integrate_riccati_fast(imu, 0.04, settings.input_gain_diag12(), settings.state_gain_diag8())
        twin.integrate_riccati_fast(imu, 0.04, settings.input_gain_diag12(), settings.state_gain_diag8())
        print(f"dense {chart} N {N}: {rel_fro(core.get_sigma(), orc.get_sigma()):.2e} structured {rel_fro(twin.get_sigma(), orc.get_sigma()):.2e}")
        check_sigma(core, orc, 1e-12)
        check_sigma(twin, orc, 1e-12)
        assert rel_fro(core.get_sigma(), twin.get_sigma()) <= 1e-12
    finally:
        core.close()
        twin.close()


def _true_state(rng, orc, N, extra=4):
    """test_compute_nees' true state: more landmarks than the filter holds, in another order"""
    s_e, ids_e, p_e = orc.state_estimate()
    ts = s_e.copy()
    ts[0:6] += rng.normal(size=6) * 0.01
    ts[10:13] += rng.normal(size=3) * 0.05
    ts[13:16] += rng.normal(size=3) * 0.05
    tids = np.concatenate([ids_e, 100000 + np.arange(extra)]).astype(np.int32)
    tp = np.concatenate([p_e * (1.0 + 0.02 * rng.normal(size=(N, 1))) + rng.normal(size=(N, 3)) * 0.05, rng.normal(size=(extra, 3)) + [0, 0, 5]])
    perm = rng.permutation(N + extra)
    return ts, tids[perm], tp[perm]


@pytest.mark.parametrize("chart,N", [("invdepth", 200), ("euclid", 200), ("invdepth", 334), ("invdepth", 335), ("euclid", 335), ("invdepth", 420)])
def test_compute_nees_at_size(chart, N):
    """test_compute_nees' comparison and tolerance (1e-9 relative) where the chain over 21 + 3 N + 1 columns has 20 panels, 32 | 33 panels (N = 334 | 335) and 41"""
    rng, settings, orc, core, _ = make_pair(CHARTS[chart], N, seed=3900 + N)
    try:
        assert (21 + 3 * N + 1 + 31) // 32 == {200: 20, 334: 32, 335: 33, 420: 41}[N]
        ts, tids, tp = _true_state(rng, orc, N)
        nees_o, nees_g = orc.compute_nees(ts, tids, tp), core.compute_nees(ts, tids, tp)
        print(f"nees {chart} N {N}: oracle {nees_o:.6g} relative error {abs(nees_g - nees_o) / nees_o:.2e}")
        assert nees_o > 0 and core.nees_lu_fallbacks() == 0
        assert abs(nees_g - nees_o) <= 1e-9 * nees_o
        check_sigma(core, orc, 0.0)
    finally:
        core.close()


def test_nees_elimination_fallback_at_size():
    """test_nees_returns_a_number_when_sigma_is_not_numerically_spd's construction and tolerance (1e-6) at N = 110 (n = 351): k_ge_step / k_ge_back over 351 pivots"""
    from eqvio_amd.capi import COORD_INVDEPTH

    rng = np.random.default_rng(78)
    N = 110
    n = 21 + 3 * N
    settings = settings_for(COORD_INVDEPTH)
    xi0, Xs, ids, q0, Q = reasonable_state(rng, N)
    V, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), n))
    lam[3] = -1e-9  # slightly indefinite: what rounding leaves of a zero eigenvalue
    S = (V * lam) @ V.T
    S = 0.5 * (S + S.T)
    core = EqfCore(N, COORD_INVDEPTH)
    try:
        core.set_state(xi0, Xs, ids, q0, Q)
        core.set_sigma(S)
        orc = OracleFilter(settings)
        orc.set_eqf(xi0, Xs, ids, q0, Q, S)
        es, eids, ep = orc.state_estimate()
        ts = es.copy()
        ts[0:6] += rng.normal(size=6) * 1e-3
        ts[13:16] += rng.normal(size=3) * 1e-2
        tp = ep + rng.normal(size=ep.shape) * 1e-2
        assert core.nees_lu_fallbacks() == 0
        nees, ref = core.compute_nees(ts, eids, tp), orc.compute_nees(ts, eids, tp)
        print(f"nees fallback N {N}: oracle {ref:.6g} relative error {abs(nees - ref) / abs(ref):.2e}")
        assert core.nees_lu_fallbacks() == 1
        assert np.isfinite(nees) and abs(nees - ref) <= 1e-6 * abs(ref), (nees, ref)
        # the same context with an SPD matrix: the factorisation again, the counter stays
        S2 = random_spd(rng, n)
        core.set_sigma(S2)
        orc.set_eqf(xi0, Xs, ids, q0, Q, S2)
        n2 = core.compute_nees(ts, eids, tp)
        assert core.nees_lu_fallbacks() == 1 and abs(n2 - orc.compute_nees(ts, eids, tp)) <= 1e-9 * abs(n2)
    finally:
        core.close()
