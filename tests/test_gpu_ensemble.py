"""Particle ensembles on the device (include/eqf_ensemble.h, eqvio_amd/ensemble.py) against the restated truth of tests/ensemble_cases.py
(oracle/indep/eqvio_ref.py + numpy), the CPU oracle's compute_nees and the single-truth route eqf_compute_nees.

Bounds. 1e-9 relative to max(1, |value|) for everything that is restated geometry (errors, sampled particles, integration; test_compute_nees' bound for NEES).
NEES(sampled particle) = |xi|^2 / n within ten times what the restatement itself loses (tests/golden/ensemble_identity_baseline.json), floor 1e-12.
Covariance within 1e-11 |C|_F of numpy on the device's own E: P u sqrt(n) < 3e-12 for P <= 1024 terms summed in another order. Across positions in the
ensemble and across P a particle's NEES agrees to 1e-12 relative (the test prints whether it is bit-identical).
Seen values are printed (run with -s); profiles/r26_ensemble_parity.txt is such a run."""
import ctypes as C

import numpy as np
import pytest

from ensemble_cases import (PINHOLE, STAT_BANDS, STAT_SEEDS, Case, StatFixture, align_quats, case_key, get_case, load_baseline, size_cases)
from eqvio_amd.capi import COORD_INVDEPTH, OPT_INNOVATION_STATS, OPT_SIGMA_FP32, Camera, EqfCore, EqfError
from eqvio_amd.ensemble import ParticleEnsemble
from oracle_binding import OracleFilter
from util import settings_for, synth_measurement

pytestmark = pytest.mark.gpu
CASES = size_cases()
P_AT_N11 = {c[0]: c[2] for c in CASES if c[1] == 11}  # the P each chart has at N = 11
IDS = [case_key(*c) for c in CASES]
EPS = np.finfo(np.float64).eps


def make_core(c):
    core = EqfCore(max(c.N, 1), c.chart)
    core.set_state(c.xi0f, c.Xsf, c.ids, c.q0, c.Q)
    core.set_sigma(c.Sigma)
    return core


def rel1(a, b):
    """max |a - b| relative to max(1, |b|)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def index_order_mean(vals):
    """the host's sum in index order, divided by P - the same doubles in the same order as the library's loop"""
    s = 0.0
    for v in vals:
        s += float(v)
    return s / len(vals)


def ens_bytes(ens):
    ids, s, p = ens.get()
    return ens.size, ids.tobytes(), s.tobytes(), p.tobytes()


def counters(core):
    lib, h = core.lib, core.h
    la, lf = C.c_long(), C.c_long()
    lib.eqf_lookahead_stats(h, C.byref(la), C.byref(lf), 0)
    a, b, c = C.c_long(), C.c_long(), C.c_long()
    lib.eqf_speculation_stats(h, C.byref(a), C.byref(b), C.byref(c), 0)
    calls, secs = (C.c_long * 2)(), (C.c_double * 2)()
    lib.eqf_host_wait_stats(h, calls, secs, 0)
    return (la.value, lf.value, a.value, b.value, c.value, core.fork_stats(), core.nees_lu_fallbacks(), calls[1], core.innovation_totals())


def ctx_bytes(core):
    xi0, Xs, ids, q0, Q = core.get_state()
    return xi0.tobytes(), Xs.tobytes(), ids.tobytes(), q0.tobytes(), Q.tobytes(), core.get_sigma().tobytes(), core.last_gamma().tobytes()


# ---- sampling and the identity NEES = |xi|^2 / n ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart,N,P", CASES, ids=IDS)
def test_sample_matches_restatement_and_identity(chart, N, P):
    c = get_case(chart, N, P)
    core = make_core(c)
    ens = ParticleEnsemble(core, P, N)
    ens.sample(c.xi)
    assert ens.size == (P, N)
    ids, sens, pts = ens.get()
    assert np.array_equal(ids, c.ids)
    ref_s, ref_p = c.sampled
    es, ep = rel1(align_quats(sens, ref_s), ref_s), rel1(pts, ref_p)
    vals, mean = ens.nees()
    ident = c.nees_identity
    dev = float(np.max(np.abs(vals - ident) / ident))
    bound = max(10.0 * load_baseline()[case_key(chart, N, P)], 1e-12)
    print(f"[ensemble sample] {case_key(chart, N, P)} sensor {es:.2e} points {ep:.2e} identity {dev:.2e} (bound {bound:.2e})")
    assert es <= 1e-9 and ep <= 1e-9
    assert dev <= bound
    assert mean == index_order_mean(vals)


# ---- errors and NEES of a planted truth with extra landmarks in another order ---------------------------------------------------------------
@pytest.mark.parametrize("chart,N,P", CASES, ids=IDS)
def test_errors_and_nees_of_a_truth(chart, N, P):
    c = get_case(chart, N, P)
    core = make_core(c)
    ids, sens, p = c.truth_x
    ens = ParticleEnsemble(core, P, N + 2)
    ens.set(ids, sens, p)
    E = ens.errors()
    ee = rel1(E, c.eps_truth)
    vals, mean = ens.nees()
    vals2, mean2 = ens.nees()
    assert np.array_equal(vals, vals2) and mean == mean2, "NEES differs run to run"
    orc = OracleFilter(settings_for(chart))
    orc.set_eqf(c.xi0f, c.Xsf, c.ids, c.q0, c.Q, c.Sigma)
    o = np.array([orc.compute_nees(sens[k], ids, p[k]) for k in range(P)])
    s = np.array([core.compute_nees(sens[k], ids, p[k]) for k in range(P)])
    eo, es = float(np.max(np.abs(vals - o) / np.abs(o))), float(np.max(np.abs(vals - s) / np.abs(s)))
    print(f"[ensemble nees] {case_key(chart, N, P)} errors {ee:.2e} vs oracle {eo:.2e} vs eqf_compute_nees {es:.2e}")
    assert ee <= 1e-9
    assert eo <= 1e-9 and es <= 1e-9
    assert mean == index_order_mean(vals)


def test_nees_does_not_depend_on_position_or_P():
    c = get_case(1, 11, 257) if (1, 11, 257) in CASES else Case(1, 11, 257)
    core = make_core(c)
    ids, sens, p = c.truth_x
    big = ParticleEnsemble(core, 257, 13)
    big.set(ids, sens, p)
    vals, _ = big.nees()
    worst, same = 0.0, True
    for pick in ([200, 5, 31], [256], [0, 1], list(range(64, 97))):
        small = ParticleEnsemble(core, len(pick), 13)
        small.set(ids, sens[pick], p[pick])
        v, _ = small.nees()
        worst = max(worst, float(np.max(np.abs(v - vals[pick]) / vals[pick])))
        same = same and np.array_equal(v, vals[pick])
    print(f"[ensemble nees] across positions and P: worst relative difference {worst:.2e}, bit-identical: {same}")
    assert worst <= 1e-12


def test_one_factorisation_and_launches_independent_of_P():
    c1, c257 = get_case(1, 4, 1), get_case(1, 4, 257)
    seen = {}
    for c in (c1, c257):
        core = make_core(c)
        ens = ParticleEnsemble(core, c.P, c.N + 2)
        ens.set(*c.truth_x)
        ens.stats(reset=True)
        ens.nees()
        nees_stats = ens.stats(reset=True)
        ens.errors()
        err_stats = ens.stats(reset=True)
        ens.covariance()
        cov_stats = ens.stats(reset=True)
        ens2 = ParticleEnsemble(core, c.P, c.N)
        ens2.sample(c.xi)
        smp_stats = ens2.stats(reset=True)
        ens2.integrate(c.imu, c.dt)
        int_stats = ens2.stats(reset=True)
        seen[c.P] = (nees_stats, err_stats, cov_stats, smp_stats, int_stats)
    print(f"[ensemble stats] (launches, factorisations) of nees, errors, covariance, sample, integrate: P=1 {seen[1]}  P=257 {seen[257]}")
    assert seen[1] == seen[257]
    assert seen[1][0][1] == 1 and seen[1][3][1] == 1  # one factorisation per nees call and per sample call
    assert seen[1][1][1] == 0 and seen[1][2][1] == 0 and seen[1][4][1] == 0
    # n = 33: two panels. errors 1; nees = errors + build + first tile + 2 panels + row sums
    assert seen[1][1][0] == 1 and seen[1][0][0] == 6


# ---- covariance ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart,N,P", CASES, ids=IDS)
def test_covariance(chart, N, P):
    c = get_case(chart, N, P)
    core = make_core(c)
    ens = ParticleEnsemble(core, P, N + 2)
    ens.set(*c.truth_x)
    E = ens.errors()
    Cd = ens.covariance()
    assert np.array_equal(Cd, Cd.T), "not exactly symmetric"
    assert np.array_equal(Cd, ens.covariance()), "differs run to run"
    ref = E @ E.T / P
    err = float(np.linalg.norm(Cd - ref) / np.linalg.norm(ref))
    print(f"[ensemble covariance] {case_key(chart, N, P)} {err:.2e}")
    assert err <= 1e-11


# ---- integration -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart,N,P", [c for c in CASES if c[0] == 1], ids=[case_key(*c) for c in CASES if c[0] == 1])
def test_integrate(chart, N, P):
    c = get_case(chart, N, P)
    core = make_core(c)
    sens, pts = c.sampled
    ens = ParticleEnsemble(core, P, N)
    worst = 0.0
    for off in (None, c.offsets):
        ens.set(c.ids, sens, pts)
        ens.integrate(c.imu, c.dt, off)
        _, s1, p1 = ens.get()
        rs, rp = c.integrated(sens, pts, off)
        worst = max(worst, rel1(align_quats(s1, rs), rs), rel1(p1, rp))
    # dt = 0: cameraPoseChangeInv = T^-1 I T, the identity up to one rounding of its quaternion and translation (a few ulp of the point and the camera offset)
    ens.set(c.ids, sens, pts)
    ens.integrate(c.imu, 0.0)
    _, s0, p0 = ens.get()
    d0 = float(np.max(np.abs(p0 - pts))) if pts.size else 0.0
    print(f"[ensemble integrate] {case_key(chart, N, P)} worst {worst:.2e} dt=0 point change {d0:.2e}")
    assert worst <= 1e-9
    assert d0 <= 16 * EPS * max(1.0, float(np.max(np.abs(pts))) if pts.size else 1.0)
    assert rel1(align_quats(s0, sens), sens) <= 1e-14


# ---- set / get / resample: pure data movement --------------------------------------------------------------------------------------------------
def test_set_get_and_resample_are_bit_exact():
    c = get_case(2, 4, 257)
    core = make_core(c)
    ids, sens, p = c.truth_x
    ens = ParticleEnsemble(core, 300, 8)
    ens.set(ids, sens, p)
    g_ids, g_s, g_p = ens.get()
    assert g_ids.tobytes() == ids.tobytes() and g_s.tobytes() == sens.tobytes() and g_p.tobytes() == p.tobytes()
    rng = np.random.default_rng(5)
    for idx in (rng.integers(0, 257, 257), rng.permutation(257), rng.integers(0, 257, 300), np.array([256, 0, 0, 17]), np.array([3])):
        ens.set(ids, sens, p)
        ens.resample(idx)
        r_ids, r_s, r_p = ens.get()
        assert ens.size == (len(idx), 6)
        assert r_ids.tobytes() == ids.tobytes() and r_s.tobytes() == sens[idx].tobytes() and r_p.tobytes() == np.ascontiguousarray(p[idx]).tobytes()
    # twice in a row: the second gather reads what the first one wrote
    ens.set(ids, sens, p)
    a, b = rng.integers(0, 257, 100), rng.integers(0, 100, 50)
    ens.resample(a)
    ens.resample(b)
    assert ens.get()[2].tobytes() == np.ascontiguousarray(p[a][b]).tobytes()
    # no landmarks at all
    e0 = ParticleEnsemble(core, 4, 0)
    e0.set(np.zeros(0, np.int32), sens[:3], np.zeros((3, 0, 3)))
    e0.resample([2, 2, 0, 1])
    assert e0.get()[1].tobytes() == sens[[2, 2, 0, 1]].tobytes()


# ---- the context is read only --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", [0, 1, 2])
def test_context_is_untouched(chart):
    c = get_case(chart, 11, P_AT_N11[chart])
    core = make_core(c)
    ids, sens, p = c.truth_x
    core.compute_nees(sens[0], ids, p[0])  # the context's own NEES scratch and counters in use before the ensemble comes
    ens = ParticleEnsemble(core, c.P, c.N + 2)
    ens.set(*c.truth_x)
    fresh = ParticleEnsemble(core, c.P, c.N)
    cnt0, ctx0 = counters(core), ctx_bytes(core)
    for name, call in (("errors", ens.errors), ("nees", ens.nees), ("covariance", ens.covariance), ("sample", lambda: fresh.sample(c.xi))):
        call()
        cnt1 = counters(core)
        assert cnt1 == cnt0, (name, cnt0, cnt1)
        assert ctx_bytes(core) == ctx0, name
        cnt0 = counters(core)  # (the snapshot's own get_state / get_sigma are launches of the context)


def test_context_is_untouched_after_an_unsettled_update():
    """an update whose lift has not been waited for (early doorbell) followed by an ensemble call: the context ends as a twin that ran no ensemble call"""
    c = get_case(1, 70, 32)
    cam = Camera.pinhole(*PINHOLE, 752, 480)
    rng = np.random.default_rng(3)
    mid, y = synth_measurement(rng, cam, c.ids, c.q0, c.Q)
    s = settings_for(1)
    out = []
    for with_ensemble in (False, True):
        core = make_core(c)
        core.set_option(OPT_INNOVATION_STATS, 1)
        core.propagate_fast(c.imu, c.dt, s.input_gain_diag12(), s.state_gain_diag8(), c.imu[None, :], np.array([c.dt]), True)
        upd = core.stats_then_update(cam, mid, y, 1e8, 1e8, s.measurementNoise**2, True, False)[0]
        assert upd == 1
        unsettled = core.lib.eqf_update_unsettled(core.h)
        if with_ensemble:
            ens = ParticleEnsemble(core, c.P, c.N + 2)
            ens.set(*c.truth_x)
            vals, _ = ens.nees()
            assert np.all(np.isfinite(vals))
            ens.errors()
            ens.covariance()
            ParticleEnsemble(core, c.P, c.N).sample(c.xi)
        out.append((ctx_bytes(core), core.innovation_totals(), core.last_innovation()))
        print(f"[ensemble context] update unsettled before the ensemble call: {unsettled}")
    assert out[0] == out[1]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(EqfError) as e:
        call()
    return e.value.code


def test_refusals_leave_everything_untouched():
    c = get_case(1, 4, 33)
    core = make_core(c)
    ids, sens, p = c.truth_x
    ens = ParticleEnsemble(core, 40, 6)
    ens.set(ids, sens, p)
    before, ctx0 = ens_bytes(ens), ctx_bytes(core)
    # capacity
    assert code_of(lambda: ens.set(ids, np.tile(sens, (2, 1)), np.tile(p, (2, 1, 1)))) == -4
    assert code_of(lambda: ens.set(np.arange(7, dtype=np.int32), sens, np.zeros((33, 7, 3)))) == -4
    assert code_of(lambda: ens.sample(np.zeros((c.n, 41)))) == -4
    assert code_of(lambda: ens.resample(np.zeros(41, np.int32))) == -4
    assert code_of(lambda: ParticleEnsemble(core, 40, 3).sample(c.xi)) == -4  # the filter holds more landmarks than the ensemble has room for
    # bad arguments
    assert code_of(lambda: ens.resample([0, 33])) == -3
    assert code_of(lambda: ens.resample([-1])) == -3
    assert code_of(lambda: ens.set(np.array([1, 1], np.int32), sens, np.zeros((33, 2, 3)))) == -3  # a repeated id
    lacking = ParticleEnsemble(core, 40, 6)
    keep = [k for k in range(6) if ids[k] != c.ids[2]]
    lacking.set(ids[keep], sens, p[:, keep, :])
    lb = ens_bytes(lacking)
    for call in (lacking.errors, lacking.nees, lacking.covariance):
        assert code_of(call) == -3  # a filter id the ensemble lacks
    assert ens_bytes(lacking) == lb
    empty = ParticleEnsemble(core, 40, 6)
    assert code_of(empty.nees) == -3 and code_of(lambda: empty.resample([0])) == -3
    assert ens_bytes(ens) == before and ctx_bytes(core) == ctx0
    # the float Sigma store
    core32 = make_core(c)
    core32.set_option(OPT_SIGMA_FP32, 2)
    e32 = ParticleEnsemble(core32, 40, 6)
    e32.set(ids, sens, p)
    b32, s32 = ens_bytes(e32), core32.get_sigma().tobytes()
    for call in (e32.errors, e32.nees, e32.covariance, lambda: e32.sample(c.xi)):
        assert code_of(call) == -6
    assert ens_bytes(e32) == b32 and core32.get_sigma().tobytes() == s32
    # another device
    import torch

    if torch.cuda.device_count() > 1:
        other = ParticleEnsemble(core, 40, 6, device=1)
        other.set(ids, sens, p)
        assert code_of(other.nees) == -3 and code_of(lambda: other.sample(c.xi)) == -3


def test_not_spd_is_reported_and_nothing_changes():
    c = get_case(0, 4, 33)
    core = make_core(c)
    S = c.Sigma.copy()
    S[32, 32] = -S[32, 32]  # n = 33: a pivot <= 0 in the second panel
    core.set_sigma(S)
    ens = ParticleEnsemble(core, 33, 6)
    ens.set(*c.truth_x)
    before, ctx0 = ens_bytes(ens), ctx_bytes(core)
    assert code_of(ens.nees) == -2
    assert code_of(lambda: ens.sample(c.xi)) == -2
    assert ens_bytes(ens) == before and ctx_bytes(core) == ctx0
    assert core.nees_lu_fallbacks() == 0  # no partial-pivot fallback on this path
    S[32, 32] = c.Sigma[32, 32]
    S[2, 2] = 0.0  # ... and in the first tile
    core.set_sigma(S)
    assert code_of(ens.nees) == -2
    core.set_sigma(c.Sigma)
    assert np.all(ens.nees()[0] > 0)  # the context and the ensemble are good again


# ---- the workload's size ---------------------------------------------------------------------------------------------------------------------------
def test_N200_P8_against_the_oracle():
    c = Case(1, 200, 8)
    core = make_core(c)
    ids, sens, p = c.truth_x
    ens = ParticleEnsemble(core, 8, 202)
    ens.set(ids, sens, p)
    vals, _ = ens.nees()
    orc = OracleFilter(settings_for(1))
    orc.set_eqf(c.xi0f, c.Xsf, c.ids, c.q0, c.Q, c.Sigma)
    o = np.array([orc.compute_nees(sens[k], ids, p[k]) for k in range(8)])
    err = float(np.max(np.abs(vals - o) / o))
    print(f"[ensemble nees] N=200 P=8 vs oracle {err:.2e}; launches, factorisations {ens.stats()}")
    assert err <= 1e-9


def test_N200_P64_against_numpy():
    c = Case(1, 200, 64)
    core = make_core(c)
    ens = ParticleEnsemble(core, 64, 200)
    ens.sample(c.xi)
    _, sens, pts = ens.get()
    ref_s, ref_p = c.sampled
    es, ep = rel1(align_quats(sens, ref_s), ref_s), rel1(pts, ref_p)
    E = ens.errors()
    vals, _ = ens.nees()
    S = core.get_sigma()
    ref = np.einsum("ik,ik->k", E, np.linalg.solve(S, E)) / c.n  # one solve of the read-back Sigma for all right-hand sides
    err = float(np.max(np.abs(vals - ref) / ref))
    ident = float(np.max(np.abs(vals - c.nees_identity) / c.nees_identity))
    Cd = ens.covariance()
    ec = float(np.linalg.norm(Cd - E @ E.T / 64) / np.linalg.norm(Cd))
    print(f"[ensemble N=200 P=64] sample sensor {es:.2e} points {ep:.2e}; nees vs numpy {err:.2e}; identity {ident:.2e}; covariance {ec:.2e}")
    assert es <= 1e-9 and ep <= 1e-9
    assert err <= 1e-9
    assert np.array_equal(Cd, Cd.T) and ec <= 1e-11


# ---- the reference's statistical suite through the ensemble -------------------------------------------------------------------------------------------
def run_statistics(N, P, check, per_particle):
    f = StatFixture(N, P, STAT_SEEDS[(N, check)])
    core = EqfCore(N, COORD_INVDEPTH)
    core.set_state(f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
    core.set_sigma(f.sigma0)
    ens = ParticleEnsemble(core, P, N)
    ens.sample(f.xi)
    band = STAT_BANDS[check]

    def judge(tag):
        vals, mean = ens.nees()
        line = f"[ensemble statistics] N={N} P={P} {check} {tag}: mean NEES {mean:.6f} (band {band})"
        if per_particle:
            ids, sens, p = ens.get()
            single = float(np.mean([core.compute_nees(sens[k], ids, p[k]) for k in range(P)]))
            line += f", per-particle route {single:.6f}, difference {abs(mean - single):.2e}"
            assert abs(mean - single) <= 1e-9 * abs(single), line
        print(line)
        assert abs(mean - 1.0) <= band, line

    if check == "initial":
        judge("")
    elif check in ("true_input", "random_input"):
        vel, dt = (f.true_vel, 0.2) if check == "true_input" else (f.random_vel, 0.05)
        for rep in range(5):
            ens.integrate(vel, dt)
            core.integrate_riccati_discrete(vel, dt, np.zeros(12), np.zeros(8))
            core.integrate_observer(vel[None, :], np.array([dt]), True)
            judge(f"step {rep}")
    else:
        _, sens, p = ens.get()
        ens.resample(f.resample_indices(sens, p))
        mids, y = f.meas_flat()
        core.vision_update(Camera.pinhole(*PINHOLE, 752, 480), mids, y, f.var, True, False)
        judge("")


@pytest.mark.parametrize("check", ["initial", "true_input", "random_input", "output"])
def test_reference_statistics_N2_P1000(check):
    run_statistics(2, 1000, check, per_particle=True)


@pytest.mark.parametrize("check", ["initial", "true_input"])
def test_reference_statistics_N40_P256(check):
    run_statistics(40, 256, check, per_particle=False)
