"""The measurement side of the particle ensembles against batch slots on the device (include/eqf_batch_ensemble_output.h, eqvio_amd/batch_ensemble.py) against
the restated truth of tests/batch_ensemble_output_cases.py (oracle/indep/eqvio_ref.py + numpy; proved on the CPU by tests/test_batch_ensemble_output_cases.py).

Clouds are put with ens.set. Bounds: 1e-9 relative to max(1, |value|) against the restatement for the log-likelihoods and the covariance; the weights,
logsumexp and ess against numpy's log-domain formula on the device's own log-likelihoods within the same bound, |sum w - 1| <= 1e-12; the chosen indices equal
weightedResample's sequential loop on the device's weights with the restated uniforms exactly (every case has a margin >= 1e-9). Everything else is byte for
byte. Seen values are printed (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from batch_ensemble_output_cases import (COV_CASES, COV_FIVE, COV_OTHERS, FIVE, MARGIN, MAXP, OTHERS, PLANTED_UNDERFLOW, RESAMPLE, SEED, STAT_STREAM, cov_key, cov_reference,
                                         lik_key, likelihood_cases, res_key, resample_case, seeded_case)
from ensemble_cases import PINHOLE, STAT_BANDS, STAT_SEEDS, StatFixture
from ensemble_output_cases import device_camera, get_case, log_weights, margin, stat_case, weighted_resample
from ensemble_random_cases import cached_uniforms
from eqvio_amd.batch import BatchCore
from eqvio_amd.batch_ensemble import BatchEnsemble, BensLikelihoodEntry
from eqvio_amd.capi import Camera, Settings
from eqvio_amd.ensemble import ParticleEnsemble

pytestmark = pytest.mark.gpu
NONFINITE, BAD_ARG, CAPACITY = -1, -3, -4
LIK_CASES = likelihood_cases()


def settings():
    s = Settings.defaults()
    s.fastRiccati = 1
    s.removeLostLandmarks = 0
    return s


def plant(core, slot, c):
    core.set_slot_chart(slot, c.chart)
    core.set_state(slot, c.xi0f, c.Xsf, c.ids, c.q0, c.Q)
    core.set_sigma(slot, c.Sigma)


def rel1(a, b):
    """max |a - b| relative to max(1, |b|)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def cloud_bytes(ens, slot):
    ids, s, p = ens.get(slot)
    return ens.size(slot), ids.tobytes(), s.tobytes(), p.tobytes()


def slot_bytes(core, k):
    """everything of a slot its API shows: state, Sigma, chart, last result, last innovation, totals"""
    lib = core.elib
    xi0, Xs, ids, q0, Q = core.get_state(k)
    dof, nis, ld = C.c_int(), C.c_double(), C.c_double()
    lib.eqf_batch_last_innovation(core.h, k, C.byref(dof), C.byref(nis), C.byref(ld))
    n, td, tn, tl = C.c_long(), C.c_long(), C.c_double(), C.c_double()
    lib.eqf_batch_innovation_totals(core.h, k, C.byref(n), C.byref(td), C.byref(tn), C.byref(tl))
    return (xi0.tobytes(), Xs.tobytes(), ids.tobytes(), q0.tobytes(), Q.tobytes(), core.get_sigma(k).tobytes(), core.slot_chart(k), core.last_result(k),
            (dof.value, nis.value, ld.value), (n.value, td.value, tn.value, tl.value))


def put(ens, slot, c, p=None):
    ens.set(slot, c.ids, c.sensor, c.p if p is None else p)


def lik_entry(slot, c, var=None, mids=None, y=None, cam=None):
    return (slot, device_camera(c.cam) if cam is None else cam, c.mids if mids is None else mids, c.y if y is None else y, c.var if var is None else var)


def one_slot(c, room=0):
    core = BatchCore(settings(), 1)
    ens = BatchEnsemble(core, c.P + room)
    put(ens, 0, c)
    return core, ens


def seven():
    """a 7-slot batch, its ensemble of MAXP particles per slot, and the cloud of every slot: {slot: (OutputCase, meas_var, P_new, stream)}"""
    core = BatchCore(settings(), 7)
    ens = BatchEnsemble(core, MAXP)
    cases = {slot: (get_case(*key), var, Pn, stream) for slot, key, var, Pn, stream in FIVE + OTHERS}
    for slot, (c, *_) in cases.items():
        put(ens, slot, c)
    return core, ens, cases


def lik_row(out, e, P):
    ll, w, lse, ess, _ = out
    return ll[e, :P].tobytes(), w[e, :P].tobytes(), float(lse[e]), float(ess[e])


def check_weights(ll, w, lse, ess):
    rw, rlse, ress = log_weights(ll)
    ew, el, ee, es = rel1(w, rw), abs(lse - rlse) / max(1.0, abs(rlse)), abs(ess - ress) / max(1.0, abs(ress)), abs(float(np.sum(w)) - 1.0)
    assert ew <= 1e-9 and el <= 1e-9 and ee <= 1e-9 and es <= 1e-12, (ew, el, ee, es)
    return ew, el, ee, es


# ---- likelihood parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,M,P", LIK_CASES, ids=[lik_key(*c) for c in LIK_CASES])
def test_likelihood_matches_the_restatement(cam, M, P):
    c = get_case(cam, M, P)
    core, ens = one_slot(c, room=3)
    before = cloud_bytes(ens, 0)
    ll, w, lse, ess, status = ens.likelihood([lik_entry(0, c)])
    assert status == [0]
    again = ens.likelihood([lik_entry(0, c)])
    assert lik_row((ll, w, lse, ess, status), 0, P) == lik_row(again, 0, P), "differs run to run"
    el = rel1(ll[0, :P], c.loglik)
    ew, els, ee, es = check_weights(ll[0, :P], w[0, :P], lse[0], ess[0])
    print(f"[batch ensemble likelihood] {lik_key(cam, M, P)} loglik {el:.2e}; weights {ew:.2e} logsumexp {els:.2e} ess {ee:.2e} sum-1 {es:.2e}")
    assert el <= 1e-9
    if M == 0:
        assert np.all(ll[0, :P] == 0.0) and not np.any(np.signbit(ll[0, :P])) and np.all(w[0, :P] == 1.0 / P)
    assert np.all(np.isnan(ll[0, P:])) and np.all(np.isnan(w[0, P:]))  # the rest of a row is not written
    assert cloud_bytes(ens, 0) == before  # the particles are read only


def test_planted_underflow_has_finite_weights_where_the_plain_sum_is_zero():
    cam, M, P, var = PLANTED_UNDERFLOW
    c = get_case(cam, M, P)
    _, ens = one_slot(c)
    ll, w, lse, ess, status = ens.likelihood([lik_entry(0, c, var=var)])
    assert status == [0]
    with np.errstate(under="ignore"):
        plain = float(np.exp(ll[0, :P]).sum())
    print(f"[batch ensemble likelihood] planted M={M} P={P}: max loglik {ll[0, :P].max():.1f}, plain exp sum {plain}, ess {ess[0]:.3f}")
    assert plain == 0.0
    assert np.all(np.isfinite(w[0, :P])) and abs(float(w[0, :P].sum()) - 1.0) <= 1e-12 and np.isfinite(lse[0]) and ess[0] >= 1.0


# ---- byte invariances ---------------------------------------------------------------------------------------------------------------------------
def test_five_entries_equal_every_slot_alone_byte_for_byte():
    core, ens, cases = seven()
    order = [slot for slot, *_ in FIVE]
    entries = [lik_entry(slot, cases[slot][0], var=cases[slot][1]) for slot in order]
    out = ens.likelihood(entries)
    assert out[4] == [0] * 5
    rows = [lik_row(out, e, cases[slot][0].P) for e, slot in enumerate(order)]
    assert [lik_row(ens.likelihood(entries), e, cases[slot][0].P) for e, slot in enumerate(order)] == rows  # run to run
    for e, slot in enumerate(order):  # every entry alone, in a fresh ensemble of another size
        c = cases[slot][0]
        solo = BatchEnsemble(core, c.P)
        put(solo, slot, c)
        assert lik_row(solo.likelihood([entries[e]]), 0, c.P) == rows[e]
    every = [lik_entry(slot, cases[slot][0], var=cases[slot][1]) for slot, *_ in (FIVE + OTHERS)[::-1]]  # seven entries, in reverse order
    out7 = ens.likelihood(every)
    assert out7[4] == [0] * 7
    rorder = [en[0] for en in every]
    for e, slot in enumerate(order):
        assert lik_row(out7, rorder.index(slot), cases[slot][0].P) == rows[e]


def test_loglik_does_not_depend_on_position_or_P():
    c = get_case(1, 11, 257)
    core, ens = one_slot(c)
    ll = ens.likelihood([lik_entry(0, c)])[0][0].copy()
    for pick in ([200], list(range(33)), [256, 5, 31]):
        small = BatchEnsemble(core, 40)
        small.set(0, c.ids, c.sensor[pick], c.p[pick])
        l2 = small.likelihood([lik_entry(0, c)])[0]
        assert l2[0, :len(pick)].tobytes() == ll[pick].tobytes()


def test_measured_ids_in_another_order():
    c = get_case(0, 11, 33)
    _, ens = one_slot(c)
    perm = np.random.default_rng(3).permutation(c.M)
    ll, w, lse, ess, status = ens.likelihood([lik_entry(0, c, mids=c.mids[perm], y=c.y[perm])])
    assert status == [0]
    assert rel1(ll[0, :c.P], c.loglik) <= 1e-9
    check_weights(ll[0, :c.P], w[0, :c.P], lse[0], ess[0])
    sub = perm[:4]  # a subset, in another order
    ll4 = ens.likelihood([lik_entry(0, c, mids=c.mids[sub], y=c.y[sub])])[0]
    e = (c.y[sub][None] - c.measured[:, sub]).reshape(c.P, -1)
    assert rel1(ll4[0, :c.P], -0.5 * np.einsum("ki,ki->k", e, e) / c.var) <= 1e-9


# ---- non-finite values: planted values in read-only kernels ----------------------------------------------------------------------------------------
def test_a_non_finite_particle_gets_weight_zero():
    c = get_case(1, 2, 33)
    _, ens = one_slot(c)
    ll0 = ens.likelihood([lik_entry(0, c)])[0][0].copy()
    for bad_point in (np.zeros(3), np.array([np.nan, 0.1, 5.0])):
        p = c.p.copy()
        p[7, c.mpos[0]] = bad_point
        put(ens, 0, c, p)
        ll, w, lse, ess, status = ens.likelihood([lik_entry(0, c)])
        assert status == [0]
        keep = np.arange(c.P) != 7
        assert ll[0, 7] == -np.inf and w[0, 7] == 0.0
        assert ll[0, :c.P][keep].tobytes() == ll0[:c.P][keep].tobytes()
        check_weights(ll[0, :c.P], w[0, :c.P], lse[0], ess[0])
        src, st = ens.resample_weighted_seeded([(0, c.P, SEED, 1)])
        assert st == [0] and 7 not in src[0, :c.P].tolist()


def test_an_all_non_finite_entry_is_reported_alone_and_keeps_nothing():
    core, ens, cases = seven()
    order = [slot for slot, *_ in FIVE]
    entries = [lik_entry(slot, cases[slot][0], var=cases[slot][1]) for slot in order]
    clean = ens.likelihood(entries)  # weights kept for all five ...
    bad_slot, e_bad = 3, order.index(3)
    cb = cases[bad_slot][0]
    p = cb.p.copy()
    p[:, cb.mpos[1]] = 0.0
    put(ens, bad_slot, cb, p)
    sentinel = (np.full((5, MAXP), -7.0), np.full((5, MAXP), -7.0), np.full(5, -7.0), np.full(5, -7.0))
    before = [cloud_bytes(ens, k) for k in range(7)]
    out = ens.likelihood(entries, out=sentinel)
    assert out[4] == [0 if slot != bad_slot else NONFINITE for slot in order]
    for e, slot in enumerate(order):
        P = cases[slot][0].P
        if slot == bad_slot:
            assert np.all(out[0][e] == -7.0) and np.all(out[1][e] == -7.0) and out[2][e] == -7.0 and out[3][e] == -7.0
        else:
            assert lik_row(out, e, P) == lik_row(clean, e, P) and np.all(out[0][e, P:] == -7.0)
    assert [cloud_bytes(ens, k) for k in range(7)] == before
    src, st = ens.resample_weighted_seeded([(slot, cases[slot][2], SEED, cases[slot][3]) for slot in order])
    assert st == [0 if slot != bad_slot else BAD_ARG for slot in order]  # ... and nothing is kept for the bad one
    assert cloud_bytes(ens, bad_slot) == before[bad_slot]
    # a measurement that avoids the bad landmark is fine again
    ll, w, _, _, st = ens.likelihood([lik_entry(bad_slot, cb, mids=cb.mids[:1], y=cb.y[:1])])
    assert st == [0] and np.all(np.isfinite(ll[0, :cb.P])) and abs(float(w[0, :cb.P].sum()) - 1.0) <= 1e-12


# ---- resampling --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RESAMPLE, ids=[res_key(*r) for r in RESAMPLE])
def test_resample_weighted_seeded(case):
    cam, M, P, Pn, stream, var = case
    rc = resample_case(*case)
    c = rc.c
    core = BatchCore(settings(), 1)
    ens = BatchEnsemble(core, MAXP)
    put(ens, 0, c)
    _, w, _, _, status = ens.likelihood([lik_entry(0, c, var=var)])
    assert status == [0]
    wd = w[0, :P].copy()
    m = margin(wd, rc.u)
    src, st = ens.resample_weighted_seeded([(0, Pn, SEED, stream)])
    assert st == [0]
    got = src[0, :Pn]
    print(f"[batch ensemble resample] {res_key(*case)} margin on the device's weights {m:.2e}, distinct sources {len(set(got.tolist()))}")
    assert m >= MARGIN
    assert np.array_equal(got, weighted_resample(wd, rc.u)) and np.array_equal(got, rc.src)
    assert got.max() <= P - 1 and np.all(src[0, Pn:] == -1)
    ids, s, p = ens.get(0)
    assert ens.size(0) == (Pn, c.N) and ids.tobytes() == c.ids.tobytes()
    assert s.tobytes() == np.ascontiguousarray(c.sensor[got]).tobytes() and p.tobytes() == np.ascontiguousarray(c.p[got]).tobytes()
    # a second resample without a new likelihood is refused, the cloud untouched
    after = cloud_bytes(ens, 0)
    assert ens.resample_weighted_seeded([(0, Pn, SEED, stream)])[1] == [BAD_ARG] and cloud_bytes(ens, 0) == after
    # the single-filter ensemble fed the same cloud chooses the same indices
    single = ParticleEnsemble(None, MAXP, c.N)
    single.set(c.ids, c.sensor, c.p)
    single.likelihood(device_camera(cam), c.mids, c.y, var)
    assert np.array_equal(single.resample_weighted_seeded(Pn, SEED, stream), got)


def test_kept_weights_are_invalidated_by_set_sample_seeded_and_integrate():
    c = get_case(0, 2, 33)
    f = seeded_case(0, 1, 2)
    core = BatchCore(settings(), 1)
    plant(core, 0, f)
    ens = BatchEnsemble(core, 40)
    assert ens.resample_weighted_seeded([(0, 33, SEED, 1)])[1] == [BAD_ARG]  # never formed
    imu = np.zeros(13)
    for name, call in (("set", lambda: put(ens, 0, c)), ("sample_seeded", lambda: ens.sample_seeded([(0, 33, SEED, 0)])), ("integrate", lambda: ens.integrate([(0, imu, 0.01)]))):
        put(ens, 0, c)
        assert ens.likelihood([lik_entry(0, c, var=400.0)])[4] == [0]
        assert not any(call() or [])
        before = cloud_bytes(ens, 0)
        assert ens.resample_weighted_seeded([(0, 33, SEED, 1)])[1] == [BAD_ARG], name
        assert cloud_bytes(ens, 0) == before, name
    # what changes no cloud keeps them: a refused integrate entry, get
    put(ens, 0, c)
    _, w, _, _, _ = ens.likelihood([lik_entry(0, c, var=400.0)])
    assert ens.integrate([(0, None, 0.01)]) == [BAD_ARG]
    ens.get(0)
    src, st = ens.resample_weighted_seeded([(0, 33, SEED, 1)])
    assert st == [0] and np.array_equal(src[0, :33], weighted_resample(w[0, :33], cached_uniforms(SEED, 1, 33)))


def test_refused_resample_entries_leave_their_clouds_untouched_while_the_others_run():
    core, ens, cases = seven()
    good = [6, 1, 3]
    assert ens.likelihood([lik_entry(s, cases[s][0], var=cases[s][1]) for s in good + [5]])[4] == [0] * 4
    before = [cloud_bytes(ens, k) for k in range(7)]
    rs = lambda s: (s, cases[s][2], SEED, cases[s][3])  # noqa: E731
    sentinel = np.full((8, MAXP), -9, np.int32)
    src, st = ens.resample_weighted_seeded([rs(6), (0, 4, SEED, 1), (9, 4, SEED, 1), (6, 4, SEED, 1), (3, 0, SEED, 1), (5, MAXP + 1, SEED, 1), rs(1), (-1, 4, SEED, 1)], out=sentinel)
    assert st == [0, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, CAPACITY, 0, BAD_ARG]  # slot 0 has no kept weights; 9, -1 no such slot; 6 listed twice; P_new 0; beyond the room
    for e in (1, 2, 3, 4, 5, 7):
        assert np.all(src[e] == -9)
    for k in (0, 2, 3, 4, 5):
        assert cloud_bytes(ens, k) == before[k]
    alone = BatchEnsemble(core, MAXP)
    for e, s in ((0, 6), (6, 1)):
        put(alone, s, cases[s][0])
        alone.likelihood([lik_entry(s, cases[s][0], var=cases[s][1])])
        a, sta = alone.resample_weighted_seeded([rs(s)])
        assert sta == [0] and a[0].tobytes() == np.where(src[e] == -9, -1, src[e]).astype(np.int32).tobytes()
        assert cloud_bytes(alone, s) == cloud_bytes(ens, s)
    # the refused entries' kept weights stand: slots 3 and 5 resample now, as they do alone
    src2, st2 = ens.resample_weighted_seeded([rs(3), rs(5)])
    assert st2 == [0, 0]
    for e, s in enumerate((3, 5)):
        key = {slot: k for slot, k, *_ in FIVE}[s]
        assert np.array_equal(src2[e, :cases[s][2]], resample_case(*key, cases[s][2], cases[s][3], cases[s][1]).src)


def test_refused_likelihood_entries_leave_everything_untouched():
    core, ens, cases = seven()
    c3, c6 = cases[3][0], cases[6][0]
    good = lik_entry(6, c6, var=cases[6][1])
    ref = ens.likelihood([lik_entry(3, c3, var=cases[3][1]), good])
    row6 = lik_row(ref, 1, c6.P)
    before = [cloud_bytes(ens, k) for k in range(7)]
    bad_cam = device_camera(0)
    bad_cam.model = 3
    cam3, i32, f64 = device_camera(c3.cam), np.ascontiguousarray(c3.mids, np.int32), np.ascontiguousarray(c3.y, float).reshape(-1)
    ip, dp = i32.ctypes.data_as(C.POINTER(C.c_int)), f64.ctypes.data_as(C.POINTER(C.c_double))
    twice, unknown = np.array([c3.mids[0], c3.mids[0]], np.int32), np.array([c3.mids[0], 424242], np.int32)
    camp = C.cast(C.pointer(cam3), C.c_void_p)
    empty = BatchEnsemble(core, 4)
    # (slot, cam, ids, y, M, meas_var) of the refused entry, through the C struct: nulls and M < 0 cannot be said through the binding's tuples
    refused = [(9, camp, ip, dp, 2, 400.0), (-1, camp, ip, dp, 2, 400.0), (6, camp, ip, dp, 2, 400.0), (3, None, ip, dp, 2, 400.0), (3, camp, None, dp, 2, 400.0),
               (3, camp, ip, None, 2, 400.0), (3, C.cast(C.pointer(bad_cam), C.c_void_p), ip, dp, 2, 400.0), (3, camp, ip, dp, -1, 400.0), (3, camp, ip, dp, 2, 0.0),
               (3, camp, ip, dp, 2, -1.0), (3, camp, ip, dp, 2, np.nan), (3, camp, ip, dp, 2, np.inf), (3, camp, twice.ctypes.data_as(C.POINTER(C.c_int)), dp, 2, 400.0),
               (3, camp, unknown.ctypes.data_as(C.POINTER(C.c_int)), dp, 2, 400.0)]
    for k, (slot, cam, ids, y, M, var) in enumerate(refused):
        arr = (BensLikelihoodEntry * 2)()
        g = arr[0 if slot == 6 else 1]  # the good entry of slot 6 runs beside it (in front of its own repetition)
        b = arr[1 if slot == 6 else 0]
        g.slot, g.cam, g.M, g.meas_var = 6, C.cast(C.pointer(good[1]), C.c_void_p), c6.M, good[4]
        gi, gy = np.ascontiguousarray(c6.mids, np.int32), np.ascontiguousarray(c6.y, float).reshape(-1)
        g.ids, g.y = gi.ctypes.data_as(C.POINTER(C.c_int)), gy.ctypes.data_as(C.POINTER(C.c_double))
        b.slot, b.cam, b.ids, b.y, b.M, b.meas_var = slot, cam, ids, y, M, var
        out = (np.full((2, MAXP), -7.0), np.full((2, MAXP), -7.0), np.full(2, -7.0), np.full(2, -7.0))
        status = np.zeros(2, np.int32)
        dpp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        assert ens.lib.eqf_bens_likelihood(ens.h, 2, arr, dpp(out[0]), dpp(out[1]), dpp(out[2]), dpp(out[3]), status.ctypes.data_as(C.POINTER(C.c_int))) == 0
        eb, eg = (1, 0) if slot == 6 else (0, 1)
        assert status[eb] == BAD_ARG and status[eg] == 0, k
        assert np.all(out[0][eb] == -7.0) and np.all(out[1][eb] == -7.0) and out[2][eb] == -7.0 and out[3][eb] == -7.0, k
        assert lik_row((*out, None), eg, c6.P) == row6, k
        assert [cloud_bytes(ens, q) for q in range(7)] == before, k
    assert empty.likelihood([(0, cam3, np.zeros(0, np.int32), np.zeros(0), 1.0)])[4] == [BAD_ARG]  # an empty cloud
    # the kept weights of slot 3 survived every refusal
    src, st = ens.resample_weighted_seeded([(3, cases[3][2], SEED, cases[3][3])])
    assert st == [0] and np.array_equal(src[0, :cases[3][2]], weighted_resample(ref[1][0, :c3.P], cached_uniforms(SEED, cases[3][3], cases[3][2])))


# ---- covariance ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart,N,P", COV_CASES, ids=[cov_key(*c) for c in COV_CASES])
def test_covariance_matches_the_restatement(chart, N, P):
    c = seeded_case(chart, N, P)
    truth, eps, ref = cov_reference(chart, N, P)
    core = BatchCore(settings(), 1)
    plant(core, 0, c)
    ens = BatchEnsemble(core, P)
    ens.set(0, *truth)
    before, sbefore = cloud_bytes(ens, 0), slot_bytes(core, 0)
    mats, status = ens.covariance([0])
    assert status == [0]
    Cd = mats[0]
    err = rel1(Cd, ref)
    print(f"[batch ensemble covariance] {cov_key(chart, N, P)} n = {c.n}: {err:.2e}")
    assert Cd.shape == (c.n, c.n) and err <= 1e-9
    assert np.array_equal(Cd, Cd.T)  # exactly symmetric
    assert ens.covariance([0])[0][0].tobytes() == Cd.tobytes()  # run to run
    # the filter's own landmarks alone, in the filter's order: the same particles' errors, the same C
    own = BatchEnsemble(core, P)
    own.set(0, c.ids, *c.sampled)
    assert own.covariance([0])[0][0].tobytes() == Cd.tobytes()
    assert cloud_bytes(ens, 0) == before and slot_bytes(core, 0) == sbefore


def test_covariance_of_five_entries_equals_every_slot_alone_and_a_missing_id_is_refused_alone():
    core = BatchCore(settings(), 7)
    ens = BatchEnsemble(core, 257)
    for slot, key in COV_FIVE + COV_OTHERS:
        plant(core, slot, seeded_case(*key))
        ens.set(slot, *cov_reference(*key)[0])
    order = [slot for slot, _ in COV_FIVE]
    mats, status = ens.covariance(order)
    assert status == [0] * 5
    for e, (slot, key) in enumerate(COV_FIVE):
        assert rel1(mats[e], cov_reference(*key)[2]) <= 1e-9
        solo = BatchEnsemble(core, key[2])
        solo.set(slot, *cov_reference(*key)[0])
        m1, s1 = solo.covariance([slot])
        assert s1 == [0] and m1[0].tobytes() == mats[e].tobytes()
    rev, st = ens.covariance([2, 4] + order[::-1])
    assert st == [0] * 7
    for e, slot in enumerate(order):
        assert rev[2 + 4 - e].tobytes() == mats[e].tobytes()
    # a cloud that lacks one of the filter's ids, a repeated slot, a bad slot, an empty cloud: refused alone
    ids3, s3, p3 = ens.get(3)
    lacking = BatchEnsemble(core, 257)
    for slot, key in COV_FIVE:
        lacking.set(slot, *cov_reference(*key)[0])
    filter_ids = seeded_case(*dict(COV_FIVE)[3]).ids
    drop = int(np.where(ids3 == filter_ids[0])[0][0])
    keep = [i for i in range(len(ids3)) if i != drop]
    lacking.set(3, ids3[keep], s3, np.ascontiguousarray(p3[:, keep]))
    m, st = lacking.covariance([6, 9, 0, 6, 3, 2, 5])
    assert st == [0, BAD_ARG, 0, BAD_ARG, BAD_ARG, BAD_ARG, 0]
    assert m[0].tobytes() == mats[0].tobytes() and m[2].tobytes() == mats[1].tobytes() and m[6].tobytes() == mats[3].tobytes()
    assert all(m[e] is None for e in (1, 3, 4, 5))


# ---- counting -------------------------------------------------------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_entries_P_or_M():
    seen = []
    for slots, key in (([0], (0, 1, 2)), ([6, 0, 3, 5, 1], (1, 11, 257))):
        c = get_case(*key)
        core = BatchCore(settings(), 7)  # slots without landmarks: the covariance is the sensor block's, n = 21
        ens = BatchEnsemble(core, 257)
        for s in slots:
            put(ens, s, c)
        ens.stats(reset=True)
        assert ens.likelihood([lik_entry(s, c, var=4000.0) for s in slots])[4] == [0] * len(slots)
        a = ens.stats(reset=True)
        assert ens.covariance(slots)[1] == [0] * len(slots)
        b = ens.stats(reset=True)
        assert ens.resample_weighted_seeded([(s, c.P, SEED, 2) for s in slots])[1] == [0] * len(slots)
        d = ens.stats(reset=True)
        seen.append((a, b, d))
    print(f"[batch ensemble output stats] (launches, factorisations) of likelihood, covariance, resample_weighted_seeded: 1 entry P=2 {seen[0]}  5 entries P=257 {seen[1]}")
    assert seen[0] == seen[1] == ((2, 0), (2, 0), (3, 0))


# ---- the slot is read only ----------------------------------------------------------------------------------------------------------------------------
def test_slot_is_read_only_and_its_next_step_is_its_twins():
    key = (1, 9, 257)
    c = seeded_case(*key)
    truth = cov_reference(*key)[0]
    cam = Camera.pinhole(*PINHOLE, 752, 480)
    imus = np.stack([c.imu, c.imu])
    frame = (0, cam, imus, np.array([0.02, 0.03]), np.zeros(0, np.int32), np.zeros(0), c.imu, 0.05)
    mids = np.ascontiguousarray(truth[0][:3])
    y = np.array([[300.0, 200.0], [350.0, 260.0], [400.0, 240.0]])
    cores = []
    for with_ensemble in (True, False):
        core = BatchCore(settings(), 1)
        plant(core, 0, c)
        assert list(core.step([frame])) == [0]  # a propagation-only frame: the slot then has a last result and a Sigma of the device's own making
        if with_ensemble:
            ens = BatchEnsemble(core, 257)
            ens.set(0, *truth)
            before = slot_bytes(core, 0)
            assert ens.likelihood([(0, cam, mids, y, 1e6)])[4] == [0]
            assert slot_bytes(core, 0) == before
            assert ens.covariance([0])[1] == [0]
            assert slot_bytes(core, 0) == before
            assert ens.resample_weighted_seeded([(0, 200, SEED, 1)])[1] == [0]
            assert slot_bytes(core, 0) == before
            assert ens.covariance([0])[1] == [0]
            assert slot_bytes(core, 0) == before
        assert list(core.step_accurate([frame])) == [0]
        cores.append(core)
    assert slot_bytes(cores[0], 0) == slot_bytes(cores[1], 0)


# ---- the reference's output check, three charts in one call each ----------------------------------------------------------------------------------------
def test_reference_output_check_three_charts():
    f = StatFixture(2, 1000, STAT_SEEDS[(2, "output")])
    sc = stat_case()
    s = f.settings
    s.fastRiccati, s.removeLostLandmarks = 1, 0
    core = BatchCore(s, 3)
    for chart in range(3):
        core.set_slot_chart(chart, chart)
        core.set_state(chart, f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
        core.set_sigma(chart, f.sigma0)
    ens = BatchEnsemble(core, 1000)
    assert ens.sample_seeded([(0, 1000, SEED, 0), (2, 1000, SEED, 2)]) == [0, 0]
    ens.set(1, sc.ids, sc.sensor, sc.p)  # the InvDepth slot holds StatFixture's own particles
    cam = Camera.pinhole(*PINHOLE, 752, 480)
    mids, y = f.meas_flat()
    _, w, _, ess, status = ens.likelihood([(k, cam, mids, y, f.var) for k in range(3)])
    assert status == [0, 0, 0]
    u = cached_uniforms(SEED, STAT_STREAM, 1000)
    m = margin(w[1], u)
    src, status = ens.resample_weighted_seeded([(k, 1000, SEED, STAT_STREAM) for k in range(3)])
    assert status == [0, 0, 0]
    # the single-filter device route of the same case, the same uniforms through the seed
    single = ParticleEnsemble(None, 1000, 2)
    single.set(sc.ids, sc.sensor, sc.p)
    single.likelihood(cam, mids, y, f.var)
    ref = single.resample_weighted_seeded(1000, SEED, STAT_STREAM)
    print(f"[batch ensemble output check] N=2 P=1000 ess {[round(float(v), 2) for v in ess]} distinct {[len(set(src[k].tolist())) for k in range(3)]} margin (invdepth) {m:.2e}")
    assert m >= MARGIN
    assert np.array_equal(src[1], ref) and np.array_equal(src[1], weighted_resample(w[1], u))
    none13, none = np.zeros((0, 13)), np.zeros(0)
    assert list(core.step_accurate([(k, cam, none13, none, mids, y) for k in range(3)])) == [0, 0, 0]  # the vision update alone: no IMU sample
    assert all(core.last_result(k)[0] & 16 for k in range(3))  # EQF_BATCH_UPDATED
    _, mean, status = ens.nees([0, 1, 2])
    assert status == [0, 0, 0]
    print(f"[batch ensemble output check] mean NEES after the update: euclid {mean[0]:.6f} invdepth {mean[1]:.6f} normal {mean[2]:.6f} (band {STAT_BANDS['output']})")
    assert np.all(np.abs(mean - 1.0) <= STAT_BANDS["output"])
