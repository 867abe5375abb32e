"""The filter batch's frame kernel (k_batch_frame, eqvio_amd/csrc/eqf_batch.hpp) at its size and bookkeeping edges, on planted frames
(tests/batch_scenarios.py; tests/test_batch_scenarios.py shows on the CPU that every scenario is the edge it claims to be): every tile shape of the blocked
solve up to 64 landmarks, bit 63 of the 64-bit masks, the outlier ranking under a binding cap, unmeasured landmarks that stay, the empty measurement, the
median depth, both failure returns and what they promise about the slot, slots with different numbers of IMU samples, and NEES / augment at the same sizes.
Each scenario is ONE frame from a planted state (teacher forced by construction), many scenarios of different sizes share one batch and one device step,
and the bar is the project's flat 1e-9 on state and Sigma against the CPU oracle, with identical ids, flags and decisions."""
import numpy as np
import pytest

import batch_scenarios as bs
from batch_scenarios import ADDED, EMPTY, EQF_E_CAPACITY, EQF_E_NONFINITE, EQF_E_NOT_SPD, REMOVED_INVALID, REMOVED_OLD, REMOVED_OUTLIERS, UPDATED
from eqvio_amd.batch import VIOFilterBatch
from oracle_binding import OracleFilter, oracle_cam_undistort
from run_configs import parity
from util import rel_fro

pytestmark = pytest.mark.gpu
TOL = 1e-9


def run_group(name):
    s, scs = bs.build_group(name)
    batch = VIOFilterBatch(s, len(scs), 64)
    return s, scs, batch, bs.run(batch, s, scs)


def check(sc, r, flags, status=0):
    """one scenario against its oracle: status, identical ids (every removeOld / outlier / invalid decision), the flag word, state and Sigma at TOL"""
    assert r.status == status, (sc.name, r.status)
    assert np.array_equal(r.ids_dev, r.ids_orc), (sc.name, r.ids_dev, r.ids_orc)
    assert r.flags == flags, (sc.name, r.flags, flags)
    print(f"{sc.name}: N {sc.N} -> {len(r.ids_dev)}, M {len(sc.mid)}, k {len(sc.imus)}, flags {r.flags}, parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e}")
    assert r.parity[0] < TOL and r.parity[1] < TOL, (sc.name, r.parity)


def rerun_alone(s, sc, r):
    """the same scenario in a one-slot batch: bit-identical"""
    one = VIOFilterBatch(s, 1, 64)
    r1 = bs.run(one, s, [sc])[0]
    assert r1.status == r.status and r1.flags == r.flags and r1.depth == r.depth
    for a, b in zip(r1.eqf, r.eqf):
        assert np.array_equal(a, b, equal_nan=True), sc.name


def nees_matches(batch, slots, results, seed):
    rng = np.random.default_rng(seed)
    truths = [bs.true_of(results[k].orc, rng) for k in slots]
    vals, st = batch.compute_nees([(k, *t) for k, t in zip(slots, truths)])
    assert np.all(st == 0)
    for k, t, v in zip(slots, truths, vals):
        ref = results[k].orc.compute_nees(*t)
        assert abs(v - ref) <= TOL * abs(ref), (k, v, ref)


@pytest.mark.parametrize("group", [g for g in bs.GROUPS if g.startswith("sizes_")])
def test_size_grid(group):
    s, scs, batch, res = run_group(group)
    for sc, r in zip(scs, res):
        check(sc, r, UPDATED)
        assert np.array_equal(r.eqf[5], r.eqf[5].T)
    by = {sc.name: k for k, sc in enumerate(scs)}
    nees_matches(batch, [by["size63"], by["size64"], by["size1"]], res, 1)
    for name in ("size64", "size8", "size15"):
        rerun_alone(s, scs[by[name]], res[by[name]])


@pytest.mark.parametrize("chart", ["euclid", "invdepth"])
def test_partial_measurement_keeps_lost_landmarks(chart):
    s, scs, batch, res = run_group(f"partial_{chart}")
    for sc, r in zip(scs, res):
        check(sc, r, EMPTY if len(sc.mid) == 0 else UPDATED)
        assert len(r.ids_dev) == sc.N
    # the empty measurement: the slot is the oracle after its propagation and observer steps, and nothing else moved
    sc, r = scs[0], res[0]
    assert len(sc.mid) == 0 and r.flags == EMPTY
    for a, b in zip(r.eqf[2:4], r.before[2:4]):  # ids and origin points, bit for bit
        assert np.array_equal(a, b)
    assert np.array_equal(r.eqf[0], r.before[0])
    prop = bs.propagated(s, sc.state, sc.Sigma, sc.t0, sc.stamp, sc.imus, riccati=True)
    e = parity(batch.slot(0), prop)
    assert max(e) < TOL, e
    rerun_alone(s, scs[3], res[3])


@pytest.mark.parametrize("group", ["turnover_fixed_euclid", "turnover_fixed_invdepth", "turnover_median_euclid", "turnover_median_invdepth"])
def test_turnover_at_capacity(group):
    s, scs, batch, res = run_group(group)
    for k, (sc, r) in enumerate(zip(scs, res)):
        if sc.oracle == "none":  # 64 stay + 1 new: refused, the slot untouched bit for bit
            assert r.status == EQF_E_CAPACITY
            for a, b in zip(r.eqf, r.before):
                assert np.array_equal(a, b)
            assert batch.slot(k).get_time() == sc.t0
            continue
        check(sc, r, REMOVED_OLD | ADDED | UPDATED)
        assert len(r.ids_dev) == 64
        # the depth the new landmarks got against the oracle's: its new origin point is bearing * depth
        new = sc.plan["new"][0]
        i, j = list(r.ids_orc).index(new), list(sc.mid).index(new)
        depth = np.linalg.norm(r.orc.get_eqf()[3][i]) / np.linalg.norm(oracle_cam_undistort(sc.cam, sc.y[2 * j:2 * j + 2]))
        print(f"{sc.name}: depth device {r.depth!r} oracle {depth!r}")
        assert abs(r.depth - depth) <= 1e-12 * depth, (sc.name, r.depth, depth)
        if not s.useMedianDepth or sc.name == "turnover64":
            assert r.depth == s.initialSceneDepth
    rerun_alone(s, scs[3], res[3])  # every landmark replaced: Ns = 0, nnew = 64
    rerun_alone(s, scs[1], res[1])


@pytest.mark.parametrize("cap", bs.RANK_CAPS)
def test_outlier_ranking_under_the_cap(cap):
    s, scs, batch, res = run_group(f"rank_cap{cap}")
    for sc, r in zip(scs, res):
        d = bs.describe(s, sc)
        check(sc, r, d["flags"])
        discarded = sorted(set(sc.state[2].tolist()) - set(r.ids_dev.tolist()))
        assert discarded == sorted(d["discarded"]), (sc.name, discarded, d["discarded"])
        assert bool(r.flags & REMOVED_OUTLIERS) == bool(discarded)
    assert len(set(scs[0].state[2].tolist()) - set(res[0].ids_dev.tolist())) == min(cap, bs.C_ABS + bs.C_PROB)
    if cap in (1, bs.C_ABS + 1):
        rerun_alone(s, scs[0], res[0])


def test_max_outliers_truncation():
    s, scs, batch, res = run_group("rank_truncation")
    check(scs[0], res[0], UPDATED)  # (1 - 0.9) * 10 truncates to 0: the absolute outlier stays
    assert len(res[0].ids_dev) == 10


def test_invalid_landmarks_at_the_ends():
    s, scs, batch, res = run_group("invalid_ends")
    for k, (sc, r) in enumerate(zip(scs, res)):
        check(sc, r, UPDATED | (REMOVED_INVALID if sc.plan["invalid"] else 0))
        assert sorted(set(sc.state[2].tolist()) - set(r.ids_dev.tolist())) == [int(sc.state[2][i]) for i in sc.plan["invalid"]]
    nees_matches(batch, list(range(len(scs))), res, 2)  # slots 0, 2, 3 sit in their other buffer pair now
    rerun_alone(s, scs[3], res[3])
    rerun_alone(s, scs[1], res[1])


def sigma_close(a, b):
    """rel_fro where Sigma holds entries too large to square: the Frobenius norm of those entries after an exact scaling by 2^-600, and of the rest as it is"""
    big = np.abs(b) > 1e150
    e_big = rel_fro(np.ldexp(a[big], -600), np.ldexp(b[big], -600)) if big.any() else 0.0
    return max(e_big, rel_fro(np.where(big, 0.0, a), np.where(big, 0.0, b))), int(big.sum())


@pytest.mark.parametrize("group", ["failures", "failures_euclid"])
def test_failure_paths_keep_their_promise(group):
    s, scs, batch, res = run_group(group)
    by = {sc.name: k for k, sc in enumerate(scs)}
    for name in ("good_a", "good_b", "good_c"):  # the other slots of the step match their oracles
        sc = scs[by[name]]
        check(sc, res[by[name]], (REMOVED_OLD | ADDED if sc.plan["new"] else 0) | UPDATED)
    for name, status in (("not_spd", EQF_E_NOT_SPD), ("nonfinite", EQF_E_NONFINITE)):
        sc, r = scs[by[name]], res[by[name]]
        assert r.status == status, (name, r.status)
        # ids and flags show the frame's bookkeeping, without the update
        assert np.array_equal(r.ids_dev, r.ids_orc) and len(r.ids_dev) == 64 and set(sc.plan["new"]) <= set(r.ids_dev.tolist())
        assert r.flags == REMOVED_OLD | ADDED, (name, r.flags)
        assert r.depth == s.initialSceneDepth
        # ... and the slot holds the propagation and that bookkeeping: the oracle that ran them and no update
        e_sigma, n_big = sigma_close(r.eqf[5], r.orc.get_sigma())
        print(f"{name}: status {r.status}, parity state {r.parity[0]:.2e}, Sigma {e_sigma:.2e} ({n_big} entries beyond 1e150)")
        assert r.parity[0] < TOL and e_sigma < TOL, (name, r.parity[0], e_sigma)
        assert (n_big > 0) == (name == "nonfinite")
    rerun_alone(s, scs[by["nonfinite"]], res[by["nonfinite"]])


@pytest.mark.parametrize("chart", ["euclid", "invdepth"])
def test_unequal_imu_counts(chart):
    s, scs, batch, res = run_group(f"unequal_imu_{chart}")
    assert sorted({len(sc.imus) for sc in scs}) == [1, 2, 10, 45]
    for sc, r in zip(scs, res):
        check(sc, r, UPDATED)
    k45 = [k for k, sc in enumerate(scs) if len(sc.imus) == 45 and sc.N == 64][0]
    rerun_alone(s, scs[k45], res[k45])


def test_augment_at_capacity():
    s = bs.shipped_euroc()
    rng = np.random.default_rng(8)
    full = [bs.make(s, f"aug{k}", 8000 + k, 64) for k in range(2)]
    batch = VIOFilterBatch(s, 3, 64)
    orcs = []
    for k, sc in enumerate(full):
        batch.slot(k).force_eqf(*sc.state, sc.Sigma)
        orc = OracleFilter(s)
        orc.set_eqf(*sc.state, sc.Sigma)
        orcs.append(orc)
    orcs.append(OracleFilter(s))  # slot 2: no landmark
    fresh = (10 ** 5 + 2 * np.arange(64)).astype(np.int32)
    pts = rng.uniform(-1, 1, (64, 3)) * 3.0 + np.array([0, 0, 8.0])
    # 64 -> 64 with every id replaced, 64 -> 0, 0 -> 64, in one launch
    entries = [(0, fresh, fresh[::-1].copy(), pts[::-1].copy()), (1, np.zeros(0, np.int32), fresh, pts), (2, fresh, fresh, pts)]
    assert np.all(batch.augment_landmark_states(entries) == 0)
    for (k, new_ids, prov_ids, prov_p), n_after in zip(entries, (64, 0, 64)):
        orcs[k].augment_landmark_states(new_ids, np.zeros(23), prov_ids, prov_p)
        assert len(batch.slot(k).get_eqf()[2]) == n_after
        e = parity(batch.slot(k), orcs[k])
        assert max(e) < TOL, (k, e)
        assert rel_fro(batch.slot(k).get_sigma(), orcs[k].get_sigma()) == 0.0  # a copy and constants: exact
    assert np.array_equal(batch.slot(0).get_eqf()[2], fresh)
