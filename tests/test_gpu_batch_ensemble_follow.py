"""eqf_bens_follow on the device (eqvio_amd/csrc/eqf_batch_ensemble_follow.h, BatchEnsemble.follow) against the restated truth of tests/batch_ensemble_follow_cases.py
(numpy's cholesky, a triangular solve, oracle/indep/eqvio_ref.py's charts; proved and admitted on the CPU by tests/test_batch_ensemble_follow_cases.py).

Bounds. The project's flat 1e-9 relative to max(1, |value|) (rel1) for the added points and for the NEES afterwards; the mean NEES of the statistical case within
the reference's own bands (ensemble_cases.STAT_BANDS). Everything else - ids, sensor planes, kept points, invariance to position, company, P and run, what a
refusal leaves - is byte for byte. The refusals are refusals by screening or by the pivot flag of a planted indefinite Sigma: code paths on valid memory.
Seen values are printed (run with -s); profiles/r31_batch_ensemble_follow_parity.txt is such a run."""
import ctypes as C

import numpy as np
import pytest

from batch_ensemble_follow_cases import FIVE, MAXP, OTHERS, REGEN, SEED, STREAM_0, TABLE, StatCase, get_case, key
from ensemble_cases import PINHOLE, STAT_BANDS, StatFixture
from eqvio_amd.batch import BatchCore
from eqvio_amd.batch_ensemble import BatchEnsemble
from eqvio_amd.capi import Camera, Settings

pytestmark = pytest.mark.gpu
NOT_SPD, BAD_ARG, UNSUPPORTED = -2, -3, -6
REMOVED_OLD, ADDED, UPDATED = 1, 4, 16


def settings():
    s = Settings.defaults()
    s.fastRiccati = 1
    s.removeLostLandmarks = 0
    return s


def plant(core, slot, c, Sigma=None):
    core.set_slot_chart(slot, c.chart)
    core.set_state(slot, c.xi0f, c.Xsf, c.ids, c.q0, c.Q)
    core.set_sigma(slot, c.Sigma if Sigma is None else Sigma)


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


def camera():
    return Camera.pinhole(*PINHOLE, 752, 480)


def keep_weights(ens, slot):
    """a likelihood call with an empty measurement (uniform weights): afterwards the slot has kept weights"""
    assert ens.likelihood([(slot, camera(), np.zeros(0, np.int32), np.zeros(0), 1.0)])[4] == [0]


def check_followed(ens, slot, fc):
    """ids, sensor planes and kept points byte for byte, the added points against the restatement: the seen error"""
    ids, s, p = ens.get(slot)
    assert ens.size(slot) == (fc.P, fc.N) and np.array_equal(ids, fc.c.ids)
    assert s.tobytes() == fc.sensor.tobytes()
    assert np.ascontiguousarray(p[:, :fc.nK]).tobytes() == fc.kept_p.tobytes()
    return rel1(p[:, fc.nK:], fc.added_p) if fc.N > fc.nK else 0.0


def seven(room=MAXP):
    """the 7-slot batch of the multi-entry tests, planted, and an ensemble whose seven clouds are set"""
    core = BatchCore(settings(), 7)
    cases = {slot: get_case(*k) for slot, k in FIVE + OTHERS}
    for slot, fc in cases.items():
        plant(core, slot, fc.c)
    ens = BatchEnsemble(core, room)
    for slot, fc in cases.items():
        ens.set(slot, *fc.cloud)
    return core, ens, cases


# ---- parity with the restatement, every case of the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE, ids=[key(*t) for t in TABLE])
def test_follow_matches_the_restatement(case):
    fc = get_case(*case)
    core = BatchCore(settings(), 1)
    plant(core, 0, fc.c)
    ens = BatchEnsemble(core, fc.P + 3)
    ens.set(0, *fc.cloud)
    before = slot_bytes(core, 0)
    dropped, added, status = ens.follow([(0, SEED, fc.stream)])
    assert status == [0] and (int(dropped[0]), int(added[0])) == fc.counts
    ep = check_followed(ens, 0, fc)
    vals, _, st = ens.nees([0])
    assert st == [0]
    en = rel1(vals[0, :fc.P], fc.nees)
    print(f"[batch ensemble follow] {key(*case)} n_K = {fc.nk} n = {fc.n}: added points {ep:.2e} nees {en:.2e}")
    assert ep <= 1e-9 and en <= 1e-9
    assert slot_bytes(core, 0) == before
    d2, a2, st2 = ens.follow([(0, SEED, fc.stream)])  # now in step: a no-op
    assert st2 == [0] and (int(d2[0]), int(a2[0])) == (0, 0)


# ---- regeneration: the cloud's own draw comes back ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REGEN, ids=[key(*t) for t in REGEN])
def test_cut_cloud_followed_with_its_own_seed_gets_its_points_back(case):
    fc = get_case(*case)
    core = BatchCore(settings(), 1)
    plant(core, 0, fc.c)
    ens = BatchEnsemble(core, fc.P)
    assert ens.sample_seeded([(0, fc.P, SEED, STREAM_0)]) == [0]
    ids0, s0, p0 = ens.get(0)
    cut_ids, _, cut_p = fc.cloud  # the planted cut: the kept ids and the foreign ones in the case's order, with the device's own points for the kept ones
    cut_p = cut_p.copy()
    for j, gid in enumerate(cut_ids):
        if gid in ids0:
            cut_p[:, j] = p0[:, list(ids0).index(gid)]
    ens.set(0, cut_ids, s0, cut_p)
    assert ens.follow([(0, SEED, STREAM_0)])[2] == [0]
    ids1, s1, p1 = ens.get(0)
    err = rel1(p1[:, fc.nK:], p0[:, fc.nK:])
    print(f"[batch ensemble follow regeneration] {key(*case)}: {err:.2e}")
    assert np.array_equal(ids1, ids0) and s1.tobytes() == s0.tobytes() and np.ascontiguousarray(p1[:, :fc.nK]).tobytes() == np.ascontiguousarray(p0[:, :fc.nK]).tobytes()
    assert err <= 1e-9


# ---- byte for byte: position, company, P and run do not matter ---------------------------------------------------------------------------------------
def test_five_entries_equal_every_entry_alone_byte_for_byte():
    core, ens, cases = seven()
    before = [slot_bytes(core, k) for k in range(7)]
    order = [slot for slot, _ in FIVE]
    entries = [(slot, SEED, cases[slot].stream + slot) for slot in order]
    dropped, added, status = ens.follow(entries)
    assert status == [0] * 5
    clouds = {}
    for e, slot in enumerate(order):
        assert (int(dropped[e]), int(added[e])) == cases[slot].counts
        clouds[slot] = cloud_bytes(ens, slot)
    for slot, _ in OTHERS:  # not listed: untouched
        assert cloud_bytes(ens, slot)[1] == cases[slot].cloud[0].tobytes()
    for e, slot in enumerate(order):  # every entry alone, in a fresh ensemble of another size; twice: run to run
        for _ in range(2):
            solo = BatchEnsemble(core, cases[slot].P)
            solo.set(slot, *cases[slot].cloud)
            assert solo.follow([entries[e]])[2] == [0]
            assert cloud_bytes(solo, slot) == clouds[slot]
    _, rev, rcases = seven()  # seven entries, in reverse order
    every = [(slot, SEED, rcases[slot].stream + slot) for slot, _ in (FIVE + OTHERS)[::-1]]
    assert rev.follow(every)[2] == [0] * 7
    for slot in order:
        assert cloud_bytes(rev, slot) == clouds[slot]
    assert [slot_bytes(core, k) for k in range(7)] == before


def test_a_particles_added_points_do_not_depend_on_P():
    fc = get_case(2, 9, 12, 257, "order", 0)
    core = BatchCore(settings(), 1)
    plant(core, 0, fc.c)
    ids, sens, p = fc.cloud
    got = {}
    for P in (1, 33, 257):
        ens = BatchEnsemble(core, P)
        ens.set(0, ids, sens[:P], p[:P])
        assert ens.follow([(0, SEED, fc.stream)])[2] == [0]
        got[P] = ens.get(0)[2]
    assert got[1].tobytes() == np.ascontiguousarray(got[257][:1]).tobytes() and got[33].tobytes() == np.ascontiguousarray(got[257][:33]).tobytes()
    other = BatchEnsemble(core, 33)  # another stream changes every added point and no kept one
    other.set(0, ids, sens[:33], p[:33])
    assert other.follow([(0, SEED, fc.stream + 1)])[2] == [0]
    q = other.get(0)[2]
    assert np.array_equal(q[:, :fc.nK], got[33][:, :fc.nK]) and not np.any(q[:, fc.nK:] == got[33][:, fc.nK:])


# ---- no-ops, drops, counting --------------------------------------------------------------------------------------------------------------------------
def test_no_op_keeps_everything_and_drops_count_no_factorisation():
    fc = get_case(1, 5, 6, 16, "foreign", 3)
    core = BatchCore(settings(), 1)
    plant(core, 0, fc.c)
    ens = BatchEnsemble(core, 40)
    assert ens.sample_seeded([(0, 16, SEED, STREAM_0)]) == [0]
    keep_weights(ens, 0)
    before = cloud_bytes(ens, 0)
    ens.stats(reset=True)
    dropped, added, status = ens.follow([(0, SEED, 1)])
    assert status == [0] and (int(dropped[0]), int(added[0])) == (0, 0)
    assert ens.stats(reset=True) == (0, 0) and cloud_bytes(ens, 0) == before
    assert ens.resample_weighted_seeded([(0, 16, SEED, 1)])[1] == [0]  # the kept weights stood
    for case, launches in (((1, 2, 2, 33, "order", 2), 0), ((2, 2, 2, 1, "foreign", 2), 2), ((0, 3, 3, 257, "shuffled", 0), 2)):  # drops at the tail; drops and a move; a reorder
        dc = get_case(*case)
        core = BatchCore(settings(), 1)
        plant(core, 0, dc.c)
        big = BatchEnsemble(core, dc.P)
        big.set(0, *dc.cloud)
        keep_weights(big, 0)
        big.stats(reset=True)
        dropped, added, status = big.follow([(0, SEED, 1)])
        assert status == [0] and (int(dropped[0]), int(added[0])) == dc.counts
        assert big.stats(reset=True) == (launches, 0), case
        assert check_followed(big, 0, dc) == 0.0
        assert big.resample_weighted_seeded([(0, dc.P, SEED, 1)])[1] == [BAD_ARG]  # ... and invalidated the kept weights, as every change of the cloud does
        vals, _, st = big.nees([0])
        assert st == [0] and rel1(vals[0, :dc.P], dc.nees) <= 1e-9


def test_launches_do_not_depend_on_entries_P_or_N():
    seen = []
    for slots, case in (([0], (0, 9, 10, 2, "foreign", 2)), ([6, 0, 3, 5, 1], (0, 5, 6, 257, "shuffled", 0))):
        fc = get_case(*case)
        assert fc.moves and fc.counts[1] > 0
        core = BatchCore(settings(), 7)
        ens = BatchEnsemble(core, 257)
        for s in slots:
            plant(core, s, fc.c)
            ens.set(s, *fc.cloud)
        ens.stats(reset=True)
        assert ens.follow([(s, SEED, 3) for s in slots])[2] == [0] * len(slots)
        seen.append(ens.stats(reset=True))
        inorder = get_case(0, 0, 1, 1, "order", 0)  # an entry that adds and moves nothing
        plant(core, slots[0], inorder.c)
        ens.set(slots[0], *inorder.cloud)
        assert ens.follow([(slots[0], SEED, 3)])[2] == [0]
        assert ens.stats(reset=True) == (4, 1)
    print(f"[batch ensemble follow stats] (launches, factorisations): 1 entry P=2 N=10 {seen[0]}  5 entries P=257 N=6 {seen[1]}")
    assert seen[0][0] == seen[1][0] == 5  # errors, factor, eps, the move out, the move back with the added points
    assert seen[0][1] == 1 and seen[1][1] == 5  # one factorisation per adding entry


# ---- refusals beside a good entry ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_their_clouds_untouched_while_the_good_entry_runs():
    core, ens, cases = seven()
    good = (6, SEED, 77)
    alone = BatchEnsemble(core, MAXP)
    alone.set(6, *cases[6].cloud)
    assert alone.follow([good])[2] == [0]
    want6 = cloud_bytes(alone, 6)
    # slot 3: a cloud made with set that holds the slot's landmarks 0 and 2 but not 1: the suffix rule is broken
    c3 = cases[3]
    ids3, s3, p3 = c3.cloud
    pick = [list(ids3).index(c3.c.ids[0]), list(ids3).index(c3.c.ids[2])]
    ens.set(3, ids3[pick], s3, np.ascontiguousarray(p3[:, pick]))
    # slot 1: an indefinite Sigma under an entry that adds and moves (n = 99): a pivot in the second panel, a code path on valid memory
    S = cases[1].c.Sigma.copy()
    S[30, 30] = -S[30, 30]
    core.set_sigma(1, S)
    assert cases[1].moves and cases[1].counts[1] > 0
    # slot 4: an empty cloud
    ens.set(4, np.zeros(0, np.int32), np.zeros((0, 23)), np.zeros((0, 0, 3)))
    for k in (1, 3, 5):
        keep_weights(ens, k)
    before = [cloud_bytes(ens, k) for k in range(7)]
    ens.stats(reset=True)
    sentinel = (np.full(8, -9, np.int32), np.full(8, -9, np.int32))
    entries = [(9, SEED, 1), good, (-1, SEED, 1), (3, SEED, 1), (6, SEED, 2), (4, SEED, 1), (1, SEED, 1), (7, SEED, 1)]
    dropped, added, status = ens.follow(entries, out=sentinel)
    assert status == [BAD_ARG, 0, BAD_ARG, UNSUPPORTED, BAD_ARG, BAD_ARG, NOT_SPD, BAD_ARG]
    assert (int(dropped[1]), int(added[1])) == cases[6].counts
    assert all(int(dropped[e]) == -9 and int(added[e]) == -9 for e in (0, 2, 3, 4, 5, 6, 7))
    assert cloud_bytes(ens, 6) == want6  # the good entry is what it is alone
    for k in (0, 1, 2, 3, 4, 5):  # every refused cloud, and every cloud not listed: ids and planes as they were
        assert cloud_bytes(ens, k) == before[k], k
    assert ens.stats()[1] == 2  # the good entry's factorisation and the refused one: a refused factorisation counts as one
    # the kept weights of the refused entries stand (slot 5 was not listed)
    assert ens.resample_weighted_seeded([(1, 5, SEED, 1), (3, 5, SEED, 1), (5, 5, SEED, 1)])[1] == [0, 0, 0]
    # with Sigma repaired the same entry is accepted
    core.set_sigma(1, cases[1].c.Sigma)
    ens.set(1, *cases[1].cloud)
    assert ens.follow([(1, SEED, cases[1].stream)])[2] == [0]
    assert check_followed(ens, 1, cases[1]) <= 1e-9


# ---- the slot is read only ------------------------------------------------------------------------------------------------------------------------------
def test_slot_is_read_only_and_its_next_step_is_its_twins():
    fc = get_case(2, 9, 12, 257, "order", 0)
    c = fc.c
    imus = np.stack([c.imu, c.imu])
    frame = (0, camera(), imus, np.array([0.02, 0.03]), np.zeros(0, np.int32), np.zeros(0), c.imu, 0.05)
    cores = []
    for with_ensemble in (True, False):
        core = BatchCore(settings(), 1)
        plant(core, 0, c)
        assert list(core.step([frame])) == [0]  # a propagation-only frame: the slot then has a last result and a Sigma of the device's own making
        if with_ensemble:
            ens = BatchEnsemble(core, 257)
            ens.set(0, *fc.cloud)
            before = slot_bytes(core, 0)
            assert ens.follow([(0, SEED, 5)])[2] == [0] and ens.size(0) == (257, 12)
            assert slot_bytes(core, 0) == before
            assert ens.nees([0])[2] == [0]
            assert slot_bytes(core, 0) == before
        assert list(core.step_accurate([frame])) == [0]
        cores.append(core)
    assert slot_bytes(cores[0], 0) == slot_bytes(cores[1], 0)


# ---- what was refused before is accepted now ---------------------------------------------------------------------------------------------------------------
def test_after_a_step_with_turnover_nees_is_refused_before_follow_and_accepted_after():
    f = StatFixture(2, 64, 4)
    s = f.settings
    s.fastRiccati, s.removeLostLandmarks = 1, 1
    core = BatchCore(s, 1)
    core.set_state(0, f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
    core.set_sigma(0, f.sigma0)
    ens = BatchEnsemble(core, 64)
    assert ens.sample_seeded([(0, 64, SEED, STREAM_0)]) == [0]
    cam = camera()
    # the frame tracks id 1, has lost id 0 and brings id 5
    mids = np.array([1, 5], np.int32)
    y = np.concatenate([f.meas[1], [420.0, 180.0]])
    assert list(core.step_accurate([(0, cam, np.zeros((0, 13)), np.zeros(0), mids, y)])) == [0]
    flags = core.last_result(0)[0]
    assert flags & REMOVED_OLD and flags & ADDED and flags & UPDATED
    assert core.get_state(0)[2].tolist() == [1, 5]
    assert ens.nees([0])[2] == [BAD_ARG]  # the behaviour before this call existed, pinned: a filter id the cloud does not hold
    assert ens.covariance([0])[1] == [BAD_ARG]
    _, s0, p0 = ens.get(0)
    dropped, added, status = ens.follow([(0, SEED, 9)])
    assert status == [0] and (int(dropped[0]), int(added[0])) == (1, 1)
    ids, s1, p1 = ens.get(0)
    assert ids.tolist() == [1, 5] and s1.tobytes() == s0.tobytes() and np.ascontiguousarray(p1[:, 0]).tobytes() == np.ascontiguousarray(p0[:, 1]).tobytes()
    vals, mean, st = ens.nees([0])
    assert st == [0] and np.all(np.isfinite(vals[0, :64])) and np.all(vals[0, :64] > 0)
    mats, st = ens.covariance([0])
    assert st == [0] and mats[0].shape == (27, 27)
    ll, w, _, _, st = ens.likelihood([(0, cam, np.array([5], np.int32), np.array([[420.0, 180.0]]), f.var)])
    assert st == [0] and np.all(np.isfinite(ll[0, :64])) and abs(float(w[0, :64].sum()) - 1.0) <= 1e-12
    print(f"[batch ensemble follow after a step] flags {flags}, mean NEES of 64 particles after follow {mean[0]:.4f}")


# ---- statistics: the turnover of the restated case, three charts in one call, then one output round ---------------------------------------------------------
def test_statistics_after_turnover_three_charts_in_one_call():
    sc = StatCase()
    f = sc.f
    s = f.settings
    s.fastRiccati, s.removeLostLandmarks = 1, 0
    core = BatchCore(s, 3)
    for chart in range(3):
        core.set_slot_chart(chart, chart)
        core.set_state(chart, f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
        core.set_sigma(chart, f.sigma0)
    ens = BatchEnsemble(core, 1000)
    assert ens.sample_seeded([(k, 1000, SEED, STREAM_0) for k in range(3)]) == [0, 0, 0]
    rng = np.random.default_rng(8)
    new_p = rng.uniform(-1, 1, (2, 3)) * 10.0 + np.array([0, 0, 20.0])
    assert list(core.augment([(k, [1, 7, 8], [7, 8], new_p) for k in range(3)])) == [0, 0, 0]  # id 0 leaves, 7 and 8 arrive
    assert ens.nees([0, 1, 2])[2] == [BAD_ARG] * 3
    dropped, added, status = ens.follow([(k, SEED, sc.stream) for k in range(3)])
    assert status == [0, 0, 0] and dropped.tolist() == [1, 1, 1] and added.tolist() == [2, 2, 2]
    _, mean, status = ens.nees([0, 1, 2])
    assert status == [0, 0, 0]
    print(f"[batch ensemble follow statistics] N=2->3 P=1000, one call, mean NEES euclid {mean[0]:.6f} invdepth {mean[1]:.6f} normal {mean[2]:.6f} "
          f"(restated {sc.mean_nees:.6f}, band {STAT_BANDS['initial']})")
    assert np.all(np.abs(mean - 1.0) <= STAT_BANDS["initial"])
    # one output round on the changed landmark set: likelihood, resample, a vision step, follow, nees
    cam = camera()
    mids = np.array([1, 7, 8], np.int32)
    y = np.concatenate([f.meas[1]] + [np.array([PINHOLE[0] * p[0] / p[2] + PINHOLE[2], PINHOLE[1] * p[1] / p[2] + PINHOLE[3]]) + np.sqrt(f.var) * rng.normal(size=2)
                                      for p in new_p])
    _, _, _, ess, status = ens.likelihood([(k, cam, mids, y, f.var) for k in range(3)])
    assert status == [0, 0, 0]
    assert ens.resample_weighted_seeded([(k, 1000, SEED, 6) for k in range(3)])[1] == [0, 0, 0]
    none13, none = np.zeros((0, 13)), np.zeros(0)
    assert list(core.step_accurate([(k, cam, none13, none, mids, y) for k in range(3)])) == [0, 0, 0]
    assert all(core.last_result(k)[0] & UPDATED for k in range(3))
    dropped, added, status = ens.follow([(k, SEED, 12) for k in range(3)])
    assert status == [0, 0, 0] and dropped.tolist() == [0, 0, 0] and added.tolist() == [0, 0, 0]  # the step kept the landmark set: in step already
    _, mean, status = ens.nees([0, 1, 2])
    assert status == [0, 0, 0]
    print(f"[batch ensemble follow statistics] output round: ess {[round(float(v), 1) for v in ess]}, mean NEES euclid {mean[0]:.6f} invdepth {mean[1]:.6f} "
          f"normal {mean[2]:.6f} (band {STAT_BANDS['output']})")
    assert np.all(np.abs(mean - 1.0) <= STAT_BANDS["output"])
