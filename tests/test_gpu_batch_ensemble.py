"""Particle ensembles against batch slots on the device (include/eqf_batch_ensemble.h, eqvio_amd/batch_ensemble.py) against the restated truth of
tests/ensemble_cases.py (oracle/indep/eqvio_ref.py + numpy) with the normals of tests/ensemble_random_cases.py.

Truth. seeded_case(chart, N, P) is ensemble_cases.Case(chart, N, P) - the planted filter - with its columns of normals replaced by
normals(SEED, STREAM, n, P), the draw eqf_bens_sample_seeded is defined by; .sampled, .truth_x, .eps_truth, .nees_restated, .nees_identity, .identity_baseline
and .integrated follow from it. A reference is computed once per case and shared.

Shapes. N in {0, 1, 2, 4, 5, 11, 64}: n = 21 (padded to 22), 24, 27 (padded), 33 (padded to 34), 36, 54, 213 (padded to 214, the last partial panel), and
P in {1, 2, 15, 16, 17, 31, 32, 33, 257} dealt round over N and chart. The edges of the kernels as built (eqvio_amd/csrc/eqf_batch_ensemble.hpp):
  - k_bens_factor: 16-column panels, 16 x 16 trailing tiles - np = 48 exactly three panels (N = 9), np = 46 (N = 8) and 52 (N = 10) on either side; one
    panel plus six columns at np = 22, thirteen plus six at np = 214;
  - k_bens_solve / k_bens_sample_eps: 16 particles per wave (P = 15, 16, 17 and 31, 32, 33), 16-row tiles (the same N = 8, 9, 10), four rows of normals per
    counter (n mod 4 = 1, 0, 3, 1, 0, 2 at N = 0, 1, 2, 4, 5, 11);
  - k_bens_errors / k_bens_sample_apply / k_bens_integrate_*: 256 particles per workgroup (P = 255, 256, 257).
One call lists 5 entries of a 7-slot batch in the order 6, 0, 3, 5, 1 with another N, chart and P per entry.

Bounds. 1e-9 relative to max(1, |value|) against the restatement for errors, nees, the sampled sensor states (quaternion signs aligned) and points and
integrate with and without sigma6. NEES(sampled k) = |xi_k|^2 / n within ten times what the restatement itself loses on that filter (identity_baseline),
floor 1e-12; L^-1 eps recovers the normals within the same bound, per particle relative to |xi_k|. Everything else is byte for byte.
Seen values are printed (run with -s); profiles/r29_batch_ensemble_parity.txt is such a run."""
import ctypes as C
import functools

import numpy as np
import pytest

from ensemble_cases import STAT_BANDS, STAT_SEEDS, Case, StatFixture, align_quats, case_key
from ensemble_random_cases import cached_normals
from eqvio_amd.batch import BatchCore, load_batch_protos
from eqvio_amd.batch_ensemble import BatchEnsemble
from eqvio_amd.capi import COORD_INVDEPTH, Camera, EqfCore, Settings
from eqvio_amd.ensemble import ParticleEnsemble

pytestmark = pytest.mark.gpu
SEED, STREAM = 2026, 0
BAD_ARG, CAPACITY, NOT_SPD = -3, -4, -2
SIZES_N = (0, 1, 2, 4, 5, 11, 64)
SIZES_P = (1, 2, 15, 16, 17, 31, 32, 33, 257)
EDGES = [(1, 64, 33), (2, 5, 257), (0, 9, 16), (1, 8, 255), (2, 10, 256)]  # the issue's two planted cases; the panel / tile and the workgroup edges
CASES = [(c, N, SIZES_P[(k + 3 * c) % len(SIZES_P)]) for c in range(3) for k, N in enumerate(SIZES_N)] + EDGES
IDS = [case_key(*c) for c in CASES]
FIVE = [(6, (1, 11, 257)), (0, (0, 0, 1)), (3, (1, 4, 32)), (5, (0, 64, 32)), (1, (2, 1, 33))]  # (slot, case) in the call's order
OTHERS = [(2, (2, 5, 2)), (4, (1, 5, 33))]  # the batch's two slots the call does not list
assert all(c in CASES for _, c in FIVE + OTHERS)


@functools.lru_cache(maxsize=None)
def seeded_case(chart, N, P):
    c = Case(chart, N, P)
    c.xi = np.array(cached_normals(SEED, STREAM, c.n, P))
    return c


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


def index_order_mean(vals):
    s = 0.0
    for v in vals:
        s += float(v)
    return s / len(vals)


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


def one_slot(c, max_particles=None, extra=0):
    core = BatchCore(settings(), 1)
    plant(core, 0, c)
    return core, BatchEnsemble(core, max_particles or c.P + extra)


def seven():
    """the 7-slot batch of the multi-entry tests, planted; and its ensemble of 257 particles per slot"""
    core = BatchCore(settings(), 7)
    for slot, key in FIVE + OTHERS:
        plant(core, slot, seeded_case(*key))
    return core, BatchEnsemble(core, 257)


# ---- set / get --------------------------------------------------------------------------------------------------------------------------------
def test_set_get_round_trip_is_byte_exact():
    c = seeded_case(1, 11, 257)
    core, ens = one_slot(c)
    assert ens.size(0) == (0, 0)
    ids, sens, p = c.truth_x
    ens.set(0, ids, sens, p)
    assert ens.size(0) == (257, 13)
    gi, gs, gp = ens.get(0)
    assert gi.tobytes() == ids.tobytes() and gs.tobytes() == np.ascontiguousarray(sens).tobytes() and gp.tobytes() == p.tobytes()
    ens.set(0, ids[:0], sens[:1], p[:1, :0])  # one particle, no landmark
    assert ens.size(0) == (1, 0) and ens.get(0)[1].tobytes() == np.ascontiguousarray(sens[:1]).tobytes()
    rng = np.random.default_rng(5)
    big_ids, big_s, big_p = np.arange(64, dtype=np.int32)[::-1].copy(), rng.normal(size=(3, 23)), rng.normal(size=(3, 64, 3))
    ens.set(0, big_ids, big_s, big_p)  # the 64-landmark capacity itself
    assert cloud_bytes(ens, 0) == ((3, 64), big_ids.tobytes(), big_s.tobytes(), big_p.tobytes())


# ---- parity with the restatement, every size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart,N,P", CASES, ids=IDS)
def test_sample_errors_nees_integrate_match_the_restatement(chart, N, P):
    c = seeded_case(chart, N, P)
    core, ens = one_slot(c)
    before = slot_bytes(core, 0)
    key = case_key(chart, N, P)
    bound = max(10.0 * c.identity_baseline, 1e-12)
    # sampling, the normals it used, the identity
    assert ens.sample_seeded([(0, P, SEED, STREAM)]) == [0]
    assert ens.size(0) == (P, N)
    ids, sens, pts = ens.get(0)
    assert np.array_equal(ids, c.ids)
    ref_s, ref_p = c.sampled
    es, ep = rel1(align_quats(sens, ref_s), ref_s), rel1(pts, ref_p)
    E = ens.errors(0)
    back = np.linalg.solve(c.L, E)
    en = float(np.max(np.linalg.norm(back - c.xi, axis=0) / np.linalg.norm(c.xi, axis=0)))
    vals, mean, status = ens.nees([0])
    assert status == [0]
    ident = c.nees_identity
    dev = float(np.max(np.abs(vals[0, :P] - ident) / ident))
    print(f"[batch ensemble sample] {key} sensor {es:.2e} points {ep:.2e} normals {en:.2e} identity {dev:.2e} (bound {bound:.2e}, cond {np.linalg.cond(c.Sigma):.0f})")
    assert es <= 1e-9 and ep <= 1e-9
    assert en <= bound and dev <= bound
    assert mean[0] == index_order_mean(vals[0, :P]) and np.all(np.isnan(vals[0, P:]))
    # errors and NEES of a truth with two more landmarks in another order
    tids, tsens, tp = c.truth_x
    if N + 2 > 64:  # no room for the two extra landmarks: the filter's own, in another order
        keep = c.perm[c.perm < N]
        tids, tp = c.ids[keep], np.ascontiguousarray(ref_p[:, keep])
    wide = BatchEnsemble(core, P)
    wide.set(0, tids, tsens, tp)
    ee = rel1(wide.errors(0), c.eps_truth)
    v2, m2, status = wide.nees([0])
    assert status == [0]
    ev = float(np.max(np.abs(v2[0, :P] - c.nees_restated) / np.abs(c.nees_restated)))
    print(f"[batch ensemble nees] {key} errors {ee:.2e} nees {ev:.2e}")
    assert ee <= 1e-9 and ev <= 1e-9
    assert m2[0] == index_order_mean(v2[0, :P])
    # integration, plain and with seeded input noise
    sigma6 = np.array([0.01, 0.02, 0.03, 0.1, 0.2, 0.3])
    offsets = (sigma6[:, None] * cached_normals(SEED, 9, 6, P)).T
    worst = 0.0
    for off, entry in ((None, (0, c.imu, c.dt)), (offsets, (0, c.imu, c.dt, sigma6, SEED, 9))):
        ens.set(0, c.ids, ref_s, ref_p)
        assert ens.integrate([entry]) == [0]
        _, s1, p1 = ens.get(0)
        rs, rp = c.integrated(ref_s, ref_p, off)
        worst = max(worst, rel1(align_quats(s1, rs), rs), rel1(p1, rp))
    print(f"[batch ensemble integrate] {key} worst {worst:.2e}")
    assert worst <= 1e-9
    assert slot_bytes(core, 0) == before


# ---- one call over five slots of seven: position, company, P and run do not matter ------------------------------------------------------------------
def test_five_entries_equal_every_slot_alone_byte_for_byte():
    core, ens = seven()
    before = [slot_bytes(core, k) for k in range(7)]
    order = [slot for slot, _ in FIVE]
    cases = {slot: seeded_case(*key) for slot, key in FIVE}
    entries = [(slot, cases[slot].P, SEED, STREAM) for slot in order]
    assert ens.sample_seeded(entries) == [0] * 5
    clouds = {slot: cloud_bytes(ens, slot) for slot in order}
    vals, mean, status = ens.nees(order)
    assert status == [0] * 5
    for e, slot in enumerate(order):
        c = cases[slot]
        assert ens.size(slot) == (c.P, c.N)
        ident = c.nees_identity
        assert float(np.max(np.abs(vals[e, :c.P] - ident) / ident)) <= max(10.0 * c.identity_baseline, 1e-12)
        assert mean[e] == index_order_mean(vals[e, :c.P])
    assert ens.size(2) == (0, 0) and ens.size(4) == (0, 0)
    # run to run
    v2, m2, _ = ens.nees(order)
    assert v2.tobytes() == vals.tobytes() and m2.tobytes() == mean.tobytes()
    # every slot alone, in a fresh ensemble
    solo = BatchEnsemble(core, 257)
    for e, slot in enumerate(order):
        assert solo.sample_seeded([entries[e]]) == [0]
        assert cloud_bytes(solo, slot) == clouds[slot]
        v, m, _ = solo.nees([slot])
        assert v[0].tobytes() == vals[e].tobytes() and m[0] == mean[e]
    # another entry position and other company (the two other slots join, the order is reversed)
    rev = BatchEnsemble(core, 257)
    rentries = [(2, 1, SEED, STREAM), (4, 32, SEED, STREAM)] + entries[::-1]
    assert rev.sample_seeded(rentries) == [0] * 7
    rorder = [e[0] for e in rentries]
    v, m, st = rev.nees(rorder)
    assert st == [0] * 7
    for e, slot in enumerate(order):
        assert cloud_bytes(rev, slot) == clouds[slot]
        assert v[rorder.index(slot)].tobytes() == vals[e].tobytes() and m[rorder.index(slot)] == mean[e]
    # a smaller P is the head of a larger one: the normals depend on (row, particle) alone
    head = BatchEnsemble(core, 257)
    assert head.sample_seeded([(6, 33, SEED, STREAM)]) == [0]
    full = ens.get(6)
    part = head.get(6)
    assert part[1].tobytes() == np.ascontiguousarray(full[1][:33]).tobytes() and part[2].tobytes() == np.ascontiguousarray(full[2][:33]).tobytes()
    assert head.nees([6])[0][0, :33].tobytes() == vals[0, :33].tobytes()
    # another stream changes every particle
    assert head.sample_seeded([(6, 33, SEED, STREAM + 1)]) == [0]
    other = head.get(6)
    assert not np.any(np.all(other[1] == part[1], axis=1)) and not np.any(other[2] == part[2])
    assert [slot_bytes(core, k) for k in range(7)] == before


def test_subsets_put_back_with_set_equal_the_full_cloud():
    c = seeded_case(1, 11, 257)
    core, ens = one_slot(c)
    ids, sens, p = c.truth_x
    ens.set(0, ids, sens, p)
    vals = ens.nees([0])[0][0].copy()
    for pick in ([256], [0, 1], [200, 5, 31], list(range(64, 97))):
        small = BatchEnsemble(core, 64)
        small.set(0, ids, sens[pick], p[pick])
        v, m, _ = small.nees([0])
        assert v[0, :len(pick)].tobytes() == vals[pick].tobytes()
        assert m[0] == index_order_mean(vals[pick])


def test_integrate_zero_sigma_is_integrate_without_sigma():
    c = seeded_case(1, 11, 257)
    core, ens = one_slot(c)
    sens, pts = c.sampled
    out = {}
    for route, entry in (("plain", (0, c.imu, c.dt)), ("zero", (0, c.imu, c.dt, np.zeros(6), SEED, 9)), ("noisy", (0, c.imu, c.dt, np.full(6, 0.1), SEED, 9)),
                         ("noisy2", (0, c.imu, c.dt, np.full(6, 0.1), SEED, 9)), ("stream", (0, c.imu, c.dt, np.full(6, 0.1), SEED, 10))):
        ens.set(0, c.ids, sens, pts)
        assert ens.integrate([entry]) == [0]
        out[route] = cloud_bytes(ens, 0)
    assert out["zero"] == out["plain"]
    assert out["noisy"] == out["noisy2"] and out["noisy"] != out["plain"] and out["stream"] != out["noisy"]


# ---- counting ---------------------------------------------------------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_entries_or_P():
    core, ens = seven()
    order = [slot for slot, _ in FIVE]
    seen = []
    for entries in ([(0, 2, SEED, STREAM)], [(slot, 257, SEED, STREAM) for slot in order]):
        ens.stats(reset=True)
        assert ens.sample_seeded(entries) == [0] * len(entries)
        smp = ens.stats(reset=True)
        slots = [e[0] for e in entries]
        assert ens.nees(slots)[2] == [0] * len(entries)
        nee = ens.stats(reset=True)
        c0 = seeded_case(0, 0, 1)
        assert ens.integrate([(s, c0.imu, c0.dt) for s in slots]) == [0] * len(entries)
        integ = ens.stats(reset=True)
        ens.errors(slots[0])
        err = ens.stats(reset=True)
        seen.append((smp, nee, integ, err))
    print(f"[batch ensemble stats] (launches, factorisations) of sample_seeded, nees, integrate, errors: 1 entry P=2 {seen[0]}  5 entries P=257 {seen[1]}")
    assert [s[0] for s in seen[0]] == [s[0] for s in seen[1]] == [3, 3, 2, 1]
    assert [s[1] for s in seen[0]] == [1, 1, 0, 0] and [s[1] for s in seen[1]] == [5, 5, 0, 0]  # one factorisation per (entry, call)


# ---- the slot is read only ------------------------------------------------------------------------------------------------------------------------------
def test_slot_is_read_only_and_its_next_step_is_its_twins():
    c = seeded_case(1, 11, 257)
    cam = Camera.pinhole(458.654, 457.296, 367.215, 248.375, 752, 480)
    imus = np.stack([c.imu, c.imu])
    frame = (0, cam, imus, np.array([0.02, 0.03]), np.zeros(0, np.int32), np.zeros(0), c.imu, 0.05)
    cores = []
    for with_ensemble in (True, False):
        core = BatchCore(settings(), 1)
        plant(core, 0, c)
        assert list(core.step([frame])) == [0]  # a propagation-only frame: the slot then has a last result and a Sigma of the device's own making
        if with_ensemble:
            ens = BatchEnsemble(core, 257)
            before = slot_bytes(core, 0)
            ens.sample_seeded([(0, 257, SEED, STREAM)])
            assert slot_bytes(core, 0) == before
            ens.errors(0)
            assert slot_bytes(core, 0) == before
            assert ens.nees([0])[2] == [0]
            assert slot_bytes(core, 0) == before
            ens.integrate([(0, c.imu, c.dt, np.full(6, 0.1), SEED, 9)])
            assert slot_bytes(core, 0) == before
            ens.set(0, *c.truth_x)
            ens.get(0)
            assert slot_bytes(core, 0) == before
        assert list(core.step_accurate([frame])) == [0]
        cores.append(core)
    assert slot_bytes(cores[0], 0) == slot_bytes(cores[1], 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_clouds_and_other_entries_untouched():
    core, ens = seven()
    order = [slot for slot, _ in FIVE]
    cases = {slot: seeded_case(*key) for slot, key in FIVE}
    good = [(slot, cases[slot].P, SEED, STREAM) for slot in order]
    assert ens.sample_seeded(good) == [0] * 5
    clouds = [cloud_bytes(ens, k) for k in range(7)]
    ref_vals, ref_mean, _ = ens.nees(order)
    # sample_seeded: slots out of range, a slot listed twice, sizes below 1, P beyond the capacity - the five good entries among them still run
    twin = BatchEnsemble(core, 257)
    mixed = [(-1, 4, SEED, STREAM), good[0], (7, 4, SEED, STREAM), good[1], (6, 4, SEED, STREAM), good[2], (2, 0, SEED, STREAM), good[3], (4, 258, SEED, STREAM), good[4]]
    assert twin.sample_seeded(mixed) == [BAD_ARG, 0, BAD_ARG, 0, BAD_ARG, 0, BAD_ARG, 0, CAPACITY, 0]
    assert [cloud_bytes(twin, k) for k in range(7)] == clouds
    # set / get
    lib = ens.lib
    d, i70 = np.zeros(23 * 300), np.arange(70, dtype=np.int32)
    dp, ip = d.ctypes.data_as(C.POINTER(C.c_double)), i70.ctypes.data_as(C.POINTER(C.c_int))
    big = np.zeros(3 * 70 * 2)
    bp = big.ctypes.data_as(C.POINTER(C.c_double))
    for rc, code in ((lib.eqf_bens_set(ens.h, 7, 1, 0, ip, dp, bp), BAD_ARG), (lib.eqf_bens_set(ens.h, 0, 258, 0, ip, dp, bp), CAPACITY),
                     (lib.eqf_bens_set(ens.h, 0, 2, 65, ip, dp, bp), CAPACITY), (lib.eqf_bens_set(ens.h, 0, 1, 0, ip, None, bp), BAD_ARG),
                     (lib.eqf_bens_set(ens.h, 0, -1, 0, ip, dp, bp), BAD_ARG), (lib.eqf_bens_get(ens.h, 6, ip, dp, bp, 256, 64), CAPACITY),
                     (lib.eqf_bens_get(ens.h, -1, ip, dp, bp, 300, 64), BAD_ARG), (lib.eqf_bens_size(ens.h, 7, None, None), BAD_ARG),
                     (lib.eqf_bens_errors(ens.h, 0, None), BAD_ARG), (lib.eqf_bens_errors(ens.h, 2, dp), BAD_ARG),  # ... an empty cloud
                     (lib.eqf_bens_nees(ens.h, 1, None, dp, dp, ip), BAD_ARG), (lib.eqf_bens_nees(ens.h, -1, ip, dp, dp, ip), BAD_ARG),
                     (lib.eqf_bens_sample_seeded(ens.h, 1, None, ip), BAD_ARG), (lib.eqf_bens_integrate(ens.h, 1, None, ip), BAD_ARG)):
        assert rc == code
    dup = np.array([3, 3], np.int32)
    assert lib.eqf_bens_set(ens.h, 1, 1, 2, dup.ctypes.data_as(C.POINTER(C.c_int)), dp, bp) == BAD_ARG  # repeated ids
    assert [cloud_bytes(ens, k) for k in range(7)] == clouds
    # nees: bad and repeated slots, an empty cloud; a cloud that lacks one of the filter's ids; rows of refused entries are not written
    lacking = BatchEnsemble(core, 257)
    for slot in order:
        lacking.set(slot, *ens.get(slot))
    ids3, s3, p3 = ens.get(3)
    lacking.set(3, ids3[1:], s3, p3[:, 1:])
    sentinel = (np.full((7, 257), -7.0), np.full(7, -7.0))
    v, m, st = lacking.nees([6, 9, 0, 6, 3, 2, 5], out=sentinel)
    assert st == [0, BAD_ARG, 0, BAD_ARG, BAD_ARG, BAD_ARG, 0]
    for e, slot in ((0, 6), (2, 0), (6, 5)):
        P = cases[slot].P
        assert v[e, :P].tobytes() == ref_vals[order.index(slot), :P].tobytes() and m[e] == ref_mean[order.index(slot)] and np.all(v[e, P:] == -7.0)
    for e in (1, 3, 4, 5):
        assert np.all(v[e] == -7.0) and m[e] == -7.0
    assert ens.lib.eqf_bens_errors(lacking.h, 3, dp) == BAD_ARG
    # integrate: a null sample, an empty cloud, a repeated slot; the others move as they do alone
    c0 = cases[6]
    moved = BatchEnsemble(core, 257)
    alone = BatchEnsemble(core, 257)
    for slot in order:
        moved.set(slot, *ens.get(slot))
        alone.set(slot, *ens.get(slot))
    assert moved.integrate([(6, c0.imu, 0.05), (0, None, 0.05), (2, c0.imu, 0.05), (6, c0.imu, 0.05), (5, c0.imu, 0.01), (8, c0.imu, 0.05)]) == [0, BAD_ARG, BAD_ARG, BAD_ARG, 0, BAD_ARG]
    assert alone.integrate([(6, c0.imu, 0.05)]) == [0] and alone.integrate([(5, c0.imu, 0.01)]) == [0]
    assert [cloud_bytes(moved, k) for k in range(7)] == [cloud_bytes(alone, k) for k in range(7)]
    assert cloud_bytes(moved, 0) == clouds[0] and cloud_bytes(moved, 6) != clouds[6]


def test_indefinite_sigma_is_refused_for_its_entry_alone():
    core, ens = seven()
    order = [slot for slot, _ in FIVE]
    cases = {slot: seeded_case(*key) for slot, key in FIVE}
    entries = [(slot, cases[slot].P, SEED, STREAM) for slot in order]
    assert ens.sample_seeded(entries) == [0] * 5
    ref_vals, ref_mean, _ = ens.nees(order)
    clouds = [cloud_bytes(ens, k) for k in range(7)]
    bad_slot, e_bad = 3, order.index(3)
    S = cases[bad_slot].Sigma.copy()
    S[30, 30] = -S[30, 30]  # in the second panel of n = 33: a code path on valid memory
    core.set_sigma(bad_slot, S)
    sentinel = (np.full((5, 257), -7.0), np.full(5, -7.0))
    v, m, st = ens.nees(order, out=sentinel)
    assert st == [0 if slot != bad_slot else NOT_SPD for slot in order]
    for e, slot in enumerate(order):
        if slot == bad_slot:
            assert np.all(v[e] == -7.0) and m[e] == -7.0
        else:
            P = cases[slot].P
            assert v[e, :P].tobytes() == ref_vals[e, :P].tobytes() and m[e] == ref_mean[e]
    fresh = BatchEnsemble(core, 257)
    fresh.set(bad_slot, *ens.get(bad_slot))
    kept = cloud_bytes(fresh, bad_slot)
    assert fresh.sample_seeded(entries) == [0 if slot != bad_slot else NOT_SPD for slot in order]
    for k in range(7):
        assert cloud_bytes(fresh, k) == (clouds[k] if k != bad_slot else kept)
    without = BatchEnsemble(core, 257)
    assert without.sample_seeded([en for en in entries if en[0] != bad_slot]) == [0] * 4
    assert [cloud_bytes(without, k) for k in range(7) if k != bad_slot] == [clouds[k] for k in range(7) if k != bad_slot]
    assert ens.stats(reset=True)[1] == 15 and fresh.stats()[1] == 5  # a refused factorisation counts as one


# ---- against the single-filter ensemble -------------------------------------------------------------------------------------------------------------------
def test_nees_agrees_with_the_single_filter_ensemble():
    c = seeded_case(1, 11, 33) if (1, 11, 33) in CASES else Case(1, 11, 33)
    core, ens = one_slot(c)
    ctx = EqfCore(11, COORD_INVDEPTH)
    elib, _ = load_batch_protos()
    assert elib.eqf_batch_store_ctx(core.h, 0, ctx.h) == 0
    single = ParticleEnsemble(ctx, 33, 13)
    ids, sens, p = c.truth_x
    single.set(ids, sens, p)
    ens.set(0, ids, sens, p)
    a, _ = single.nees()
    b = ens.nees([0])[0][0, :33]
    err = float(np.max(np.abs(a - b) / np.abs(a)))
    print(f"[batch ensemble vs single-filter ensemble] invdepth N=11 P=33: {err:.2e}")
    assert err <= 1e-9


# ---- the reference's initial-distribution check, three charts in one call ---------------------------------------------------------------------------------
def test_reference_initial_distribution_three_charts_in_one_call():
    f = StatFixture(2, 1000, STAT_SEEDS[(2, "initial")])
    core = BatchCore(settings(), 3)
    for chart in range(3):
        core.set_slot_chart(chart, chart)
        core.set_state(chart, f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
        core.set_sigma(chart, f.sigma0)
    ens = BatchEnsemble(core, 1000)
    assert ens.sample_seeded([(chart, 1000, SEED, chart) for chart in range(3)]) == [0, 0, 0]
    _, mean, status = ens.nees([0, 1, 2])
    assert status == [0, 0, 0]
    print(f"[batch ensemble statistics] N=2 P=1000 initial, one call, mean NEES euclid {mean[0]:.6f} invdepth {mean[1]:.6f} normal {mean[2]:.6f} (band {STAT_BANDS['initial']})")
    assert np.all(np.abs(mean - 1.0) <= STAT_BANDS["initial"])
