"""The ensemble's measurement side on the device (include/eqf_ensemble_output.h, ParticleEnsemble.measure / likelihood / resample_weighted) against the
restated cases of tests/ensemble_output_cases.py.

Bounds. measure: 1e-7 px of the restatement (the bound of DESIGN.md 11.8); pinhole also 1e-9 relative of the CPU oracle's projectPoint, which is all its
measureSystemState applies to each point. loglik: 1e-9 relative to max(1, |value|) of the restatement, M = 0 exactly 0. weights, logsumexp, ess: 1e-12
relative of exp(ll - max) / sum formed in numpy from the DEVICE'S OWN loglik (that separates the exponent's error from the normalisation's); below the normal
range a double has fewer than 53 digits to be relative in, so a weight's bound is 1e-12 of itself plus 1e-300. The weights sum to 1 within 1e-13.
resample_weighted: under the condition that the running sums of the device's own weights keep 1e-9 from every threshold (asserted, never skipped; the CPU test
proves 1e-8 on the restated weights) the indices are the reference loop's exactly, and the particles afterwards are the old ones gathered, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from ensemble_cases import PINHOLE, STAT_BANDS, STAT_SEEDS, StatFixture
from ensemble_output_cases import (MARGIN_GPU, case_key, device_camera, get_case, log_weights, margin, size_cases, stat_case, weighted_resample)
from eqvio_amd.capi import COORD_INVDEPTH, Camera, EqfCore, EqfError
from eqvio_amd.ensemble import ParticleEnsemble
from oracle_binding import oracle_cam_project

pytestmark = pytest.mark.gpu
CASES = size_cases()
IDS = [case_key(*c) for c in CASES]
BIG = (1, 11, 257)  # the 257-particle case whose subsets are judged elsewhere in smaller ensembles
assert BIG in CASES


def make_ens(c, capP=None, capN=None):
    ens = ParticleEnsemble(None, capP or c.P, capN or c.N)
    ens.set(c.ids, c.sensor, c.p)
    return ens


def rel1(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def ens_bytes(ens):
    ids, s, p = ens.get()
    return ens.size, ids.tobytes(), s.tobytes(), p.tobytes()


def code_of(call):
    with pytest.raises(EqfError) as e:
        call()
    return e.value.code


def weights_close(w, ref):
    return bool(np.all(np.abs(w - ref) <= 1e-12 * ref + 1e-300))


# ---- measure -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,M,P", CASES, ids=IDS)
def test_measure(cam, M, P):
    c = get_case(cam, M, P)
    ens, dcam = make_ens(c), device_camera(cam)
    before = ens_bytes(ens)
    y = ens.measure(dcam, c.mids)
    assert y.shape == (P, M, 2)
    err = float(np.max(np.abs(y - c.measured))) if M else 0.0
    line = f"[ensemble measure] {case_key(cam, M, P)} vs restatement {err:.2e} px"
    if cam == 0 and M:
        o = np.array([[oracle_cam_project(dcam, c.p[k, t]) for t in c.mpos] for k in range(P)])
        eo = float(np.max(np.abs(y - o) / np.abs(o)))
        line += f", vs oracle {eo:.2e} relative"
        assert eo <= 1e-9, line
    print(line)
    assert err <= 1e-7, line
    assert ens_bytes(ens) == before  # read only


# ---- likelihood ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,M,P", CASES, ids=IDS)
def test_likelihood(cam, M, P):
    c = get_case(cam, M, P)
    ens, dcam = make_ens(c), device_camera(cam)
    before = ens_bytes(ens)
    ll, w, lse, ess = ens.likelihood(dcam, c.mids, c.y, c.var)
    ll2, w2, lse2, ess2 = ens.likelihood(dcam, c.mids, c.y, c.var)
    assert ll.tobytes() == ll2.tobytes() and w.tobytes() == w2.tobytes() and lse == lse2 and ess == ess2, "differs run to run"
    el = rel1(ll, c.loglik)
    rw, rlse, ress = log_weights(ll)  # from the device's own loglik
    ew = float(np.max(np.abs(w - rw) / np.maximum(rw, 1e-288)))
    print(f"[ensemble likelihood] {case_key(cam, M, P)} loglik {el:.2e}; weights {ew:.2e} logsumexp {abs(lse - rlse) / max(1.0, abs(rlse)):.2e} ess {abs(ess - ress) / ress:.2e}"
          f" sum-1 {abs(w.sum() - 1.0):.2e}")
    assert el <= 1e-9
    if M == 0:
        assert np.all(ll == 0.0) and np.all(w == 1.0 / P)
    assert weights_close(w, rw)
    assert abs(lse - rlse) <= 1e-12 * max(1.0, abs(rlse)) and abs(ess - ress) <= 1e-12 * ress
    assert abs(w.sum() - 1.0) <= 1e-13
    assert ens_bytes(ens) == before  # the particles are read only


def test_loglik_does_not_depend_on_position_or_P():
    c = get_case(*BIG)
    dcam = device_camera(c.cam)
    ll = make_ens(c).likelihood(dcam, c.mids, c.y, c.var)[0]
    for pick in ([256], [0, 1], [200, 5, 31], list(range(64, 97))):
        small = ParticleEnsemble(None, len(pick), c.N)
        small.set(c.ids, c.sensor[pick], c.p[pick])
        v = small.likelihood(dcam, c.mids, c.y, c.var)[0]
        assert v.tobytes() == ll[pick].tobytes(), pick


# ---- resample_weighted -----------------------------------------------------------------------------------------------------------------------------
def check_resample(ens, c_sensor, c_p, w_dev, u, src):
    """the condition, the indices, and the particles afterwards"""
    m = margin(w_dev, u)
    assert m >= MARGIN_GPU, f"margin {m:.2e}: the case does not decide the indices"
    ref = weighted_resample(w_dev, u)
    assert np.array_equal(src, ref), (src, ref)
    _, s, p = ens.get()
    assert ens.size[0] == len(u)
    assert s.tobytes() == c_sensor[ref].tobytes() and p.tobytes() == np.ascontiguousarray(c_p[ref]).tobytes()
    return m


@pytest.mark.parametrize("cam,M,P", CASES, ids=IDS)
def test_resample_weighted_by_the_kept_weights(cam, M, P):
    c = get_case(cam, M, P)
    ens = make_ens(c)
    _, w, _, _ = ens.likelihood(device_camera(cam), c.mids, c.y, c.var)
    src = ens.resample_weighted(c.u)
    m = check_resample(ens, c.sensor, c.p, w, c.u, src)
    print(f"[ensemble resample_weighted] {case_key(cam, M, P)} margin {m:.2e}, distinct {len(set(src.tolist()))}")
    assert np.array_equal(src, c.src)  # ... which are the restatement's too (the CPU test proved ten times the margin there)
    assert ens.get()[0].tobytes() == c.ids.tobytes()


def test_resample_weighted_to_another_size():
    rng = np.random.default_rng(11)
    for key, Pn in (((1, 70, 1), 33), (BIG, 1), ((2, 1, 257), 300), ((2, 1, 257), 40)):
        c = get_case(*key)
        ens = make_ens(c, capP=max(c.P, Pn))
        _, w, _, _ = ens.likelihood(device_camera(c.cam), c.mids, c.y, c.var)
        u = rng.uniform(size=Pn)
        src = ens.resample_weighted(u)
        check_resample(ens, c.sensor, c.p, w, u, src)
        assert ens.size == (Pn, c.N)


def test_resample_weighted_by_the_callers_weights():
    c = get_case(2, 1, 257)
    rng = np.random.default_rng(12)
    wc = rng.uniform(0.5, 1.5, c.P) * 7.0  # not normalised
    wc[17] = 0.0
    ens = make_ens(c)
    src = ens.resample_weighted(c.u, wc)
    check_resample(ens, c.sensor, c.p, wc / wc.sum(), c.u, src)
    assert 17 not in src.tolist()
    # uniform weights and u = 0.5: the identity
    for key in ((0, 2, 31), (2, 1, 257), (1, 70, 1)):
        c = get_case(*key)
        ens = make_ens(c)
        src = ens.resample_weighted(np.full(c.P, 0.5), np.ones(c.P))
        assert np.array_equal(src, np.arange(c.P))
        assert ens_bytes(ens)[2:] == (c.sensor.tobytes(), c.p.tobytes())
    # an ensemble without landmarks: the sensor states alone are gathered
    e0 = ParticleEnsemble(None, 4, 0)
    e0.set(np.zeros(0, np.int32), c.sensor[:1].repeat(3, 0) * np.array([[1.0], [2.0], [3.0]]), np.zeros((3, 0, 3)))
    s0 = e0.get()[1]
    src = e0.resample_weighted(np.array([0.5, 0.5, 0.5, 0.5]), np.array([0.0, 1.0, 1.0]))
    assert src.tolist() == [1, 1, 2, 2] and e0.get()[1].tobytes() == s0[[1, 1, 2, 2]].tobytes()


# ---- non-finite values: planted values in read-only kernels ---------------------------------------------------------------------------------------------
def test_a_non_finite_particle_gets_weight_zero():
    c = get_case(1, 2, 33)
    dcam = device_camera(c.cam)
    ll0, w0, lse0, ess0 = make_ens(c).likelihood(dcam, c.mids, c.y, c.var)
    for bad_point in (np.zeros(3), np.array([np.nan, 0.1, 5.0])):
        p = c.p.copy()
        p[7, c.mpos[0]] = bad_point
        ens = ParticleEnsemble(None, c.P, c.N)
        ens.set(c.ids, c.sensor, p)
        ll, w, lse, ess = ens.likelihood(dcam, c.mids, c.y, c.var)
        keep = np.arange(c.P) != 7
        assert ll[7] == -np.inf and w[7] == 0.0
        assert ll[keep].tobytes() == ll0[keep].tobytes()
        rw, rlse, ress = log_weights(ll)
        assert weights_close(w, rw) and abs(lse - rlse) <= 1e-12 * max(1.0, abs(rlse)) and abs(ess - ress) <= 1e-12 * ress
        src = ens.resample_weighted(c.u)
        assert 7 not in src.tolist()


def test_all_non_finite_is_reported_and_nothing_is_kept():
    c = get_case(1, 2, 33)
    dcam = device_camera(c.cam)
    ens = make_ens(c)
    ens.likelihood(dcam, c.mids, c.y, c.var)  # weights kept ...
    p = c.p.copy()
    p[:, c.mpos[1]] = 0.0
    ens.set(c.ids, c.sensor, p)
    before = ens_bytes(ens)
    assert code_of(lambda: ens.likelihood(dcam, c.mids, c.y, c.var)) == -1
    assert code_of(lambda: ens.resample_weighted(c.u)) == -3  # ... and nothing is kept now
    assert ens_bytes(ens) == before
    # a measurement that avoids the bad landmark is fine again
    ll, w, _, _ = ens.likelihood(dcam, c.mids[:1], c.y[:1], c.var)
    assert np.all(np.isfinite(ll)) and abs(w.sum() - 1.0) <= 1e-13


# ---- the kept weights, refusals, launches ------------------------------------------------------------------------------------------------------------------
def test_kept_weights_are_invalidated_by_each_of_the_five_calls():
    c = get_case(0, 2, 31)
    dcam = device_camera(c.cam)
    ens = make_ens(c)
    assert code_of(lambda: ens.resample_weighted(c.u)) == -3  # never formed
    imu = np.zeros(13)
    for name, call in (("set", lambda: ens.set(c.ids, c.sensor, c.p)), ("integrate", lambda: ens.integrate(imu, 0.01)), ("resample", lambda: ens.resample(np.arange(c.P))),
                       ("resample_weighted", lambda: ens.resample_weighted(c.u))):
        ens.set(c.ids, c.sensor, c.p)
        ens.likelihood(dcam, c.mids, c.y, c.var)
        call()
        before = ens_bytes(ens)
        assert code_of(lambda: ens.resample_weighted(c.u)) == -3, name
        assert ens_bytes(ens) == before, name
    # measure keeps them: it is read only
    ens.set(c.ids, c.sensor, c.p)
    _, w, _, _ = ens.likelihood(dcam, c.mids, c.y, c.var)
    ens.measure(dcam, c.mids)
    assert np.array_equal(ens.resample_weighted(c.u), weighted_resample(w, c.u))
    # sample: a context's particles replace the ensemble's
    f = StatFixture(2, 31, STAT_SEEDS[(2, "output")])
    core = EqfCore(2, COORD_INVDEPTH)
    core.set_state(f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
    core.set_sigma(f.sigma0)
    es = ParticleEnsemble(core, 31, 2)
    es.sample(f.xi)
    mids, y = f.meas_flat()
    es.likelihood(Camera.pinhole(*PINHOLE, 752, 480), mids, y, f.var)
    es.sample(f.xi)
    assert code_of(lambda: es.resample_weighted(f.uniforms)) == -3, "sample"


def test_refusals_leave_everything_untouched():
    c = get_case(0, 2, 31)
    dcam = device_camera(c.cam)
    ens = make_ens(c, capP=40)
    _, w, _, _ = ens.likelihood(dcam, c.mids, c.y, c.var)
    before = ens_bytes(ens)
    bad_cam = device_camera(0)
    bad_cam.model = 3
    u = c.u
    refusals = [
        (lambda: ens.measure(None, c.mids), -3), (lambda: ens.measure(bad_cam, c.mids), -3), (lambda: ens.measure(dcam, [c.mids[0], 424242]), -3),
        (lambda: ens.measure(dcam, [c.mids[0], c.mids[0]]), -3),
        (lambda: ens.likelihood(None, c.mids, c.y, c.var), -3), (lambda: ens.likelihood(dcam, c.mids, c.y, 0.0), -3), (lambda: ens.likelihood(dcam, c.mids, c.y, -1.0), -3),
        (lambda: ens.likelihood(dcam, c.mids, c.y, np.nan), -3), (lambda: ens.likelihood(dcam, c.mids, c.y, np.inf), -3),
        (lambda: ens.likelihood(dcam, [c.mids[1], c.mids[1]], c.y, c.var), -3), (lambda: ens.likelihood(dcam, [c.mids[0], 424242], c.y, c.var), -3),
        (lambda: ens.resample_weighted(np.zeros(0)), -3), (lambda: ens.resample_weighted(np.zeros(41)), -4), (lambda: ens.resample_weighted(np.r_[u[:-1], 1.0]), -3),
        (lambda: ens.resample_weighted(np.r_[u[:-1], -1e-300]), -3), (lambda: ens.resample_weighted(np.r_[u[:-1], np.nan]), -3),
        (lambda: ens.resample_weighted(u, np.zeros(c.P)), -3), (lambda: ens.resample_weighted(u, np.r_[w[:-1], -1.0]), -3), (lambda: ens.resample_weighted(u, np.r_[w[:-1], np.inf]), -3),
        (lambda: ens.resample_weighted(u, np.r_[w[:-1], np.nan]), -3),
    ]
    for call, code in refusals:
        assert code_of(call) == code
        assert ens_bytes(ens) == before
    # the kept weights survived every refusal
    assert np.array_equal(ens.resample_weighted(u), weighted_resample(w, u))
    empty = ParticleEnsemble(None, 4, 2)
    assert code_of(lambda: empty.measure(dcam, [])) == -3 and code_of(lambda: empty.likelihood(dcam, [], np.zeros(0), 1.0)) == -3
    assert code_of(lambda: empty.resample_weighted([0.5])) == -3


def test_launches_do_not_depend_on_P_or_M():
    seen = {}
    for key in ((0, 1, 2), (2, 1, 257), (0, 70, 33), (2, 70, 31)):
        c = get_case(*key)
        dcam = device_camera(c.cam)
        ens = make_ens(c)
        ens.stats(reset=True)
        ens.measure(dcam, c.mids)
        a = ens.stats(reset=True)
        ens.likelihood(dcam, c.mids, c.y, c.var)
        b = ens.stats(reset=True)
        ens.resample_weighted(c.u)
        d = ens.stats(reset=True)
        ens.resample_weighted(c.u, np.ones(c.P))
        e = ens.stats(reset=True)
        seen[key] = (a, b, d, e)
    print(f"[ensemble output stats] (launches, factorisations) of measure, likelihood, resample_weighted kept / given: {seen}")
    assert len(set(seen.values())) == 1
    assert seen[(0, 1, 2)] == ((1, 0), (2, 0), (2, 0), (3, 0))


# ---- the reference's output check through the device route ---------------------------------------------------------------------------------------------------
def test_reference_output_check_N2_P1000_through_the_device_route():
    f = StatFixture(2, 1000, STAT_SEEDS[(2, "output")])
    cam = Camera.pinhole(*PINHOLE, 752, 480)
    mids, y = f.meas_flat()
    means = {}
    for route in ("host", "device"):
        core = EqfCore(2, COORD_INVDEPTH)
        core.set_state(f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
        core.set_sigma(f.sigma0)
        ens = ParticleEnsemble(core, 1000, 2)
        ens.sample(f.xi)
        _, sens, p = ens.get()
        ref = f.resample_indices(sens, p)
        if route == "host":
            ens.resample(ref)
        else:
            _, w, _, ess = ens.likelihood(cam, mids, y, f.var)
            m = margin(w, f.uniforms)
            assert m >= MARGIN_GPU, f"margin {m:.2e}"
            src = ens.resample_weighted(f.uniforms)
            assert np.array_equal(src, ref)
            print(f"[ensemble output check] N=2 P=1000 ess {ess:.2f} distinct {len(set(src.tolist()))} margin {m:.2e}")
        core.vision_update(cam, mids, y, f.var, True, False)
        means[route] = ens.nees()[1]
    print(f"[ensemble output check] mean NEES host route {means['host']:.9f} device route {means['device']:.9f} (band {STAT_BANDS['output']})")
    assert abs(means["device"] - means["host"]) <= 1e-12
    assert abs(means["device"] - 1.0) <= STAT_BANDS["output"]


def test_statfixture_case_matches_its_restatement():
    c = stat_case()
    ens = make_ens(c)
    ll, w, _, _ = ens.likelihood(device_camera(0), c.mids, c.y, c.var)
    assert rel1(ll, c.loglik) <= 1e-9
    src = ens.resample_weighted(c.u)
    check_resample(ens, c.sensor, c.p, w, c.u, src)
    assert np.array_equal(src, c.src)
