"""The filter batch under the Normal chart on the GPU (eqf_batch_set_slot_chart; k_batch_normal, k_batch_riccati_normal and k_batch_discrete_normal in front of
k_batch_frame_tail, eqvio_amd/csrc/eqf_batch.hpp): the planted frames of tests/batch_normal_cases.py - the existing generators under Normal settings;
tests/test_batch_normal_cases.py shows on the CPU what each of them is - against the CPU oracle with coordinateChoice = Normal, in all three propagation modes;
charts and modes mixed in one step; a slot against a Normal context; the read-only calls; the chart rules; a simulated sequence and the tool.
The bar is the project's flat 1e-9 relative on state and Sigma with identical landmark ids, and tests/discrete_cases.py's bounds for the discrete mode."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_normal_cases as bn
import batch_scenarios as bs
import consistency_cases as cc
import discrete_cases as dc
import riccati_cases as rc
from batch_scenarios import ADDED, EMPTY, EQF_E_CAPACITY, EQF_E_NOT_SPD, REMOVED_INVALID, REMOVED_OLD, UPDATED
from eqvio_amd.batch import RICCATI_ACCURATE, RICCATI_FAST, STATE_MATRIX_CONTINUOUS, STATE_MATRIX_DISCRETE, BatchCore, BatchError, VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, EqfCore, Settings
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from run_configs import parity
from test_gpu_batch_edges import sigma_close
from test_gpu_batch_nees import plant as plant_state
from test_gpu_batch_nees import spd
from util import imu_selection, rel_fro, teacher_force

pytestmark = pytest.mark.gpu
TOL = 1e-9
EQF_E_BAD_ARG, EQF_E_UNSUPPORTED = -3, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.zeros(0, np.int32)
MODES = {"fast": (RICCATI_FAST, STATE_MATRIX_CONTINUOUS), "accurate": (RICCATI_ACCURATE, STATE_MATRIX_CONTINUOUS), "discrete": (RICCATI_ACCURATE, STATE_MATRIX_DISCRETE)}


def set_mode(batch, k, mode):
    batch.set_slot_riccati(k, MODES[mode][0])
    batch.set_slot_state_matrix(k, MODES[mode][1])


def arrays(slot):
    return tuple(slot.get_eqf()) + (slot.get_sigma(),)


def same_bytes(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def run_group(name):
    sn, scs = bn.build_group(name)
    batch = bn.make_batch(sn, len(scs))
    return sn, scs, batch, bs.run(batch, sn, scs)


def check(sc, r, flags, status=0, tol=TOL):
    assert r.status == status, (sc.name, r.status)
    assert np.array_equal(r.ids_dev, r.ids_orc), (sc.name, r.ids_dev, r.ids_orc)
    assert r.flags == flags, (sc.name, r.flags, flags)
    print(f"{sc.name}: N {sc.N} -> {len(r.ids_dev)}, M {len(sc.mid)}, k {len(sc.imus)}, flags {r.flags}, parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e}")
    assert r.parity[0] < tol and r.parity[1] < tol, (sc.name, r.parity)
    return max(r.parity)


def rerun_alone(sn, sc, r):
    r1 = bs.run(bn.make_batch(sn, 1), sn, [sc])[0]
    assert r1.status == r.status and r1.flags == r.flags and r1.depth == r.depth
    for a, b in zip(r1.eqf, r.eqf):
        assert np.array_equal(a, b, equal_nan=True), sc.name


# ------------------------------------------------------------------------------------------------ 1. the size grid
@pytest.mark.parametrize("group", bn.SIZE_GROUPS)
def test_size_grid(group):
    sn, scs, batch, res = run_group(group)
    assert all(batch.slot_chart(k) == COORD_NORMAL for k in range(len(scs)))
    worst = 0.0
    for sc, r in zip(scs, res):
        worst = max(worst, check(sc, r, UPDATED))
        assert np.array_equal(r.eqf[5], r.eqf[5].T)
    print(f"{group}: largest parity {worst:.2e}")
    by = {sc.name: k for k, sc in enumerate(scs)}
    for name in ("size64", "size1"):
        rerun_alone(sn, scs[by[name]], res[by[name]])


# ------------------------------------------------------------------------------------------------ 2. the bookkeeping edges
def test_partial_measurement_keeps_lost_landmarks():
    sn, scs, batch, res = run_group("partial")
    for sc, r in zip(scs, res):
        check(sc, r, EMPTY if len(sc.mid) == 0 else UPDATED)
        assert len(r.ids_dev) == sc.N
    sc, r = scs[0], res[0]  # the empty measurement: the propagation and the observer steps, nothing else
    prop = bs.propagated(sn, sc.state, sc.Sigma, sc.t0, sc.stamp, sc.imus, riccati=True)
    assert max(parity(batch.slot(0), prop)) < TOL


@pytest.mark.parametrize("group", ["turnover_fixed", "turnover_median"])
def test_turnover_at_capacity(group):
    sn, scs, batch, res = run_group(group)
    for k, (sc, r) in enumerate(zip(scs, res)):
        if sc.oracle == "none":
            assert r.status == EQF_E_CAPACITY
            for a, b in zip(r.eqf, r.before):
                assert np.array_equal(a, b)
            continue
        check(sc, r, REMOVED_OLD | ADDED | UPDATED)
        assert len(r.ids_dev) == 64
        if not sn.useMedianDepth or sc.name == "turnover64":
            assert r.depth == sn.initialSceneDepth
    rerun_alone(sn, scs[3], res[3])  # every landmark replaced: Ns = 0, nnew = 64


def test_outlier_ranking_under_the_cap():
    sn, scs, batch, res = run_group("rank")
    for sc, r in zip(scs, res):
        d = bs.describe(sn, sc)
        check(sc, r, d["flags"])
        assert sorted(set(sc.state[2].tolist()) - set(r.ids_dev.tolist())) == sorted(d["discarded"]), sc.name


def test_invalid_landmarks_at_the_ends():
    sn, scs, batch, res = run_group("invalid_ends")
    for sc, r in zip(scs, res):
        check(sc, r, UPDATED | (REMOVED_INVALID if sc.plan["invalid"] else 0))
        assert sorted(set(sc.state[2].tolist()) - set(r.ids_dev.tolist())) == [int(sc.state[2][i]) for i in sc.plan["invalid"]]
    rerun_alone(sn, scs[3], res[3])


def test_failure_paths_keep_their_promise():
    sn, scs, batch, res = run_group("failures")
    by = {sc.name: k for k, sc in enumerate(scs)}
    for name in ("good_a", "good_b", "good_c"):  # the good neighbours of the step match their oracles
        sc = scs[by[name]]
        check(sc, res[by[name]], (REMOVED_OLD | ADDED if sc.plan["new"] else 0) | UPDATED)
    for name in ("not_spd", "nonfinite"):
        sc, r = scs[by[name]], res[by[name]]
        # not_spd: the first pivot. nonfinite: under Normal the planted cross term reaches S as well (tests/test_batch_normal_cases.py), so the update
        # fails at a pivot, not at Gamma - the slot holds the frame's propagation and bookkeeping without the update all the same
        assert r.status == EQF_E_NOT_SPD, (name, r.status)
        assert np.array_equal(r.ids_dev, r.ids_orc) and len(r.ids_dev) == 64 and set(sc.plan["new"]) <= set(r.ids_dev.tolist())
        assert r.flags == REMOVED_OLD | ADDED and r.depth == sn.initialSceneDepth
        e_sigma, n_big = sigma_close(r.eqf[5], r.orc.get_sigma())
        print(f"{name}: status {r.status}, parity state {r.parity[0]:.2e}, Sigma {e_sigma:.2e} ({n_big} entries beyond 1e150)")
        assert r.parity[0] < TOL and e_sigma < TOL, (name, r.parity[0], e_sigma)
    rerun_alone(sn, scs[by["nonfinite"]], res[by["nonfinite"]])


def test_unequal_imu_counts():
    sn, scs, batch, res = run_group("unequal_imu")
    for sc, r in zip(scs, res):
        check(sc, r, UPDATED)


# ------------------------------------------------------------------------------------------------ 3. the per-sample modes
def context_discrete_walk(sd, sc):
    """the context path's Normal discrete walk on a case (eqf_integrate_riccati_discrete between the same two congruences, eqf_integrate_observer)"""
    core = EqfCore(max(sc.N, 1), COORD_NORMAL)
    core.set_state(*sc.state)
    core.set_sigma(sc.Sigma)
    dts = imu_selection(sc.imus, sc.t0, sc.stamp)[0]
    for u, dt in zip(sc.imus, dts):
        if dt > 0:
            core.integrate_riccati_discrete(u, dt, sd.input_gain_diag12(), sd.state_gain_diag8())
        core.integrate_observer(u[None, :], np.array([dt]), bool(sd.useDiscreteVelocityLift))
    return core.get_sigma()


@pytest.mark.parametrize("mode", ["accurate", "discrete"])
def test_per_sample_modes_on_the_planted_cases(mode):
    sn, so, sd, cases = bn.riccati()
    st = so if mode == "accurate" else sd
    # the propagation alone: an empty measurement and removeLostLandmarks = 0
    keep = bn.normal(removeLostLandmarks=0)
    keep_o = rc.oracle_settings(keep) if mode == "accurate" else dc.oracle_settings(keep)
    batch = bn.make_batch(keep, len(cases))
    set_mode(batch, None, mode)
    res = bs.run(batch, keep_o, [rc.propagation_only(sc) for sc in cases])
    worst = 0.0
    for k, (sc, r) in enumerate(zip(cases, res)):
        tol = TOL if mode == "accurate" else dc.tol(sc)
        assert r.status == 0 and r.flags == EMPTY and np.array_equal(r.ids_dev, sc.state[2]), (sc.name, r.status, r.flags)
        S = r.eqf[5]
        sym = np.max(np.abs(S - S.T)) / np.max(np.abs(S))
        print(f"{mode} {sc.name}: propagation alone, parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e}, asymmetry {sym:.1e}, riccati {batch.last_riccati(k)}")
        if mode == "discrete" and sc.name.endswith("n40_k10"):
            # the ten-sample case: the context path conjugates the same way; if it is itself past 1e-8 here, twice its error is this one case's bound
            e_ctx = rel_fro(context_discrete_walk(sd, sc), dc.walk(sd, sc).get_sigma())
            print(f"discrete {sc.name}: Sigma error of the batch {r.parity[1]:.2e}, of the context path {e_ctx:.2e}")
            if e_ctx > dc.TOL_FRAME:
                tol = 2.0 * e_ctx
        assert r.parity[0] < tol and r.parity[1] < tol, (sc.name, r.parity, tol)
        assert sym <= 1e-13 and batch.last_riccati(k)[0] == rc.expected_samples(sc)
        worst = max(worst, r.parity[1])
    print(f"{mode}: largest Sigma error of the propagation alone {worst:.2e}")
    # whole frames
    batch = bn.make_batch(sn, len(cases))
    set_mode(batch, None, mode)
    res = bs.run(batch, st, cases)
    for sc, r in zip(cases, res):
        d = bs.describe(st, sc)
        tol = TOL if mode == "accurate" else dc.tol(sc)
        assert r.status == 0 and np.array_equal(r.ids_dev, r.ids_orc), (sc.name, r.status)
        print(f"{mode} {sc.name}: whole frame N {sc.N} -> {len(r.ids_dev)}, flags {r.flags}, parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e}")
        assert r.flags == d["flags"], (sc.name, r.flags, d["flags"])
        assert r.parity[0] < tol and r.parity[1] < tol, (sc.name, r.parity)


def test_all_samples_at_dt_zero():
    """no sample moves Sigma: no congruence either - the gathered Sigma, bit for bit"""
    keep = bn.normal(removeLostLandmarks=0)
    _, _, _, cases = bn.riccati()
    sc = rc.propagation_only(next(c for c in cases if c.name.endswith("zero_dt_mid")))
    for step in ("step_accurate", "step_discrete"):
        batch = bn.make_batch(keep, 1)
        batch.start_slot(0, sc.state[0], NONE, np.zeros((0, 3)), sc.t0)
        batch.slot(0).force_eqf(*sc.state, sc.Sigma)
        before = batch.slot(0).get_sigma()
        sel, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
        assert getattr(BatchCore.of(batch), step)([(0, sc.cam, sc.imus, np.zeros(len(sc.imus)), sc.mid, sc.y, mean, total)])[0] == 0
        assert batch.slot(0).get_sigma().tobytes() == before.tobytes() and batch.last_riccati(0) == (0, 0)


# ------------------------------------------------------------------------------------------------ 4. charts and modes in one step
def test_three_charts_and_three_modes_in_one_step():
    sn, _, _, cases = bn.riccati()
    sc = next(c for c in cases if c.name.endswith("n40_k10"))
    charts = (COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL)
    combos = [(c, m) for m in MODES for c in charts]
    order = np.random.default_rng(3).permutation(len(combos))  # Normal slots between the others, modes interleaved

    def planted(batch, k, chart, mode):
        batch.set_slot_chart(k, chart)
        set_mode(batch, k, mode)
        batch.start_slot(k, sc.state[0], NONE, np.zeros((0, 3)), sc.t0)
        batch.slot(k).force_eqf(*sc.state, sc.Sigma)
        for u in sc.imus:
            batch.process_imu(k, u)

    mixed = VIOFilterBatch(bn.batch_settings(sn), len(combos), 64)
    for k, j in enumerate(order):
        planted(mixed, k, *combos[j])
    assert np.all(mixed.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k in range(len(combos))]) == 0)
    seen = {}
    for k, j in enumerate(order):
        alone = VIOFilterBatch(bn.batch_settings(sn), 1, 64)
        planted(alone, 0, *combos[j])
        assert alone.process_vision([(0, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
        assert same_bytes(arrays(mixed.slot(k)), arrays(alone.slot(0))), combos[j]
        assert mixed.last_riccati(k) == alone.last_riccati(0)
        seen[combos[j]] = arrays(mixed.slot(k))
    # nine different results
    for a in combos:
        for b in combos:
            assert a == b or not np.array_equal(seen[a][5], seen[b][5]), (a, b)
    # a Euclidean and an InvDepth slot beside Normal neighbours give the bytes they give in a batch that never sees the Normal chart
    others = [(c, m) for m in MODES for c in (COORD_EUCLIDEAN, COORD_INVDEPTH)]
    plain = VIOFilterBatch(bn.batch_settings(sn), len(others), 64)
    for k, (chart, mode) in enumerate(others):
        planted(plain, k, chart, mode)
    assert np.all(plain.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k in range(len(others))]) == 0)
    for k, combo in enumerate(others):
        assert same_bytes(arrays(plain.slot(k)), seen[combo]), combo


def device_entry(k, sc):
    """the case as a device-level frame (BatchCore.step / step_accurate / step_discrete)"""
    sel, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
    return (k, sc.cam, sc.imus, sel, sc.mid, sc.y, mean, total)


@pytest.mark.parametrize("step", ["step", "step_accurate", "step_discrete"])
def test_one_device_call_lists_all_three_charts(step):
    """eqf_batch_step* itself with E / N / I / N / N / E interleaved in ONE list (the filter level never sends such a list: it groups by chart): the Normal
    entries move behind the others in the packet and run on their part of it. Every slot has the bytes, status, flags and counters of the same slot in a call
    of its own, the listed order notwithstanding, and a slot that is not listed is untouched."""
    sn, _, _, cases = bn.riccati()
    by = {c.name.split("_", 1)[1]: c for c in cases}
    layout = [(COORD_EUCLIDEAN, by["n40_k10"]), (COORD_NORMAL, by["n64_k2"]), (COORD_INVDEPTH, by["turnover"]), (COORD_NORMAL, by["n40_k10"]),
              (COORD_NORMAL, by["n1_k2"]), (COORD_EUCLIDEAN, by["outliers"]), (COORD_NORMAL, by["turnover"])]
    B = len(layout) + 1

    def planted(batch, k, chart, sc):
        batch.set_slot_chart(k, chart)
        batch.slot(k).force_eqf(*sc.state, sc.Sigma)

    mixed = VIOFilterBatch(bn.batch_settings(sn), B, 64)
    for k, (chart, sc) in enumerate(layout):
        planted(mixed, k, chart, sc)
    planted(mixed, B - 1, COORD_NORMAL, by["n40_k1"])  # not listed
    idle = arrays(mixed.slot(B - 1))
    core = BatchCore.of(mixed)
    listed = [3, 0, 6, 2, 1, 5, 4]  # not in slot order either: packet position, slot and chart are three different things
    st = getattr(core, step)([device_entry(k, layout[k][1]) for k in listed])
    assert np.all(st == 0), st
    for k, (chart, sc) in enumerate(layout):
        alone = VIOFilterBatch(bn.batch_settings(sn), 1, 64)
        planted(alone, 0, chart, sc)
        c1 = BatchCore.of(alone)
        assert getattr(c1, step)([device_entry(0, sc)])[0] == 0
        assert same_bytes(arrays(mixed.slot(k)), arrays(alone.slot(0))), (step, k, chart, sc.name)
        assert core.last_result(k) == c1.last_result(0) and core.last_riccati(k) == c1.last_riccati(0), (step, k)
        assert mixed.last_innovation(k) == alone.last_innovation(0)
    assert same_bytes(arrays(mixed.slot(B - 1)), idle)
    # a second call on the same batch with the groups the other way round in the list, and a refused entry between them: the remap holds
    for k, (chart, sc) in enumerate(layout):
        planted(mixed, k, chart, sc)  # (its own chart is accepted on a slot that holds landmarks)
    entries = [device_entry(k, layout[k][1]) for k in (1, 4, 0)] + [device_entry(1, layout[1][1])] + [device_entry(k, layout[k][1]) for k in (6, 2)]
    st = getattr(core, step)(entries)
    assert st.tolist() == [0, 0, 0, EQF_E_BAD_ARG, 0, 0], st  # the repeated slot is refused, the rest is done
    for k in (1, 4, 0, 6, 2):
        chart, sc = layout[k]
        alone = VIOFilterBatch(bn.batch_settings(sn), 1, 64)
        planted(alone, 0, chart, sc)
        assert getattr(BatchCore.of(alone), step)([device_entry(0, sc)])[0] == 0
        assert same_bytes(arrays(mixed.slot(k)), arrays(alone.slot(0))), (step, k)


# ------------------------------------------------------------------------------------------------ 5. a slot against a context
@pytest.mark.parametrize("mode", ["fast", "accurate", "discrete"])
def test_slot_against_normal_context(mode):
    sn, so, sd, cases = bn.riccati()
    sc = next(c for c in cases if c.name.endswith("n40_k10"))
    batch = bn.make_batch(sn, 1)
    set_mode(batch, 0, mode)
    r = bs.run(batch, {"fast": sn, "accurate": so, "discrete": sd}[mode], [sc])[0]
    assert r.status == 0 and r.flags == UPDATED and np.array_equal(r.ids_dev, sc.state[2])
    core = EqfCore(sc.N, COORD_NORMAL)
    core.set_state(*sc.state)
    core.set_sigma(sc.Sigma)
    dts, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
    Qd, Pd = sn.input_gain_diag12(), sn.state_gain_diag8()
    if mode == "fast":
        core.integrate_riccati_fast(mean, total, Qd, Pd)
    for u, dt in zip(sc.imus, dts):
        if dt > 0 and mode != "fast":
            getattr(core, f"integrate_riccati_{mode}")(u, dt, Qd, Pd)
        core.integrate_observer(u[None, :], np.array([dt]), bool(sn.useDiscreteVelocityLift))
    core.vision_update(sc.cam, sc.mid, sc.y, sn.measurementNoise**2, bool(sn.useEquivariantOutput), bool(sn.useDiscreteInnovationLift))
    e = rel_fro(r.eqf[5], core.get_sigma())
    _, Xc, idc, _, Qc = core.get_state()
    ex = max(np.max(np.abs(r.eqf[1][[0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 20, 21, 22]] - Xc[[0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 20, 21, 22]])),
             np.max(np.abs(r.eqf[4][:, 4] / Qc[:, 4] - 1)))
    print(f"{mode}: slot against context, Sigma {e:.2e}, X / landmark scale {ex:.2e}")
    tol = TOL if mode != "discrete" else dc.TOL_FRAME
    assert np.array_equal(idc, r.ids_dev) and e < tol and ex < tol, (mode, e, ex)


# ------------------------------------------------------------------------------------------------ 6. NEES and consistency
def test_nees_and_consistency():
    sn = bn.with_chart(bs.reference_defaults(), COORD_NORMAL)
    rng = np.random.default_rng(41)
    Ns = [0, 1, 7, 40, 64, 20]
    batch = bn.make_batch(sn, len(Ns))
    entries, orcs, states = [], [], []
    for k, N in enumerate(Ns):
        st, V, lam = plant_state(rng, N, COORD_NORMAL)
        if k == len(Ns) - 1:
            # indefinite: a pivot of the Cholesky is <= 0 and the partial-pivot elimination answers. The eigenvalue is planted at -0.3, not at the -1e-9 of
            # tests/test_gpu_batch_nees.py: there cond(Sigma) is 9e9 and the oracle's own value is 1.8e-7 from the one formed in the planted eigenbasis, so no
            # implementation can be asked for 1e-9 of it; here cond(Sigma) is 7e3 (the oracle is within 3e-14 of that value) and the bound is the flat one
            lam[3] = -0.3
        S = spd(V, lam)
        batch.slot(k).force_eqf(*st, S)
        orc = OracleFilter(sn)
        orc.set_eqf(*st, S)
        entries.append((k, *cc.truth_with_extras(orc, rng)))
        orcs.append(orc)
        states.append(st)
    vals, status = batch.compute_nees(entries)
    assert np.all(status == 0)
    recs, status = batch.consistency(entries)
    assert np.all(status == 0)
    for k, N in enumerate(Ns):
        ref = orcs[k].compute_nees(*entries[k][1:])
        lu = k == len(Ns) - 1
        print(f"N {N}: NEES {vals[k]!r} oracle {ref!r} lu {recs[k]['lu']}")
        assert abs(vals[k] - ref) <= TOL * abs(ref), (N, vals[k], ref)
        assert batch.nees_lu_fallbacks(k) == (2 if lu else 0) and recs[k]["lu"] == int(lu)
        assert np.float64(recs[k]["nees"]).tobytes() == np.float64(vals[k]).tobytes()
        exp = cc.expected_record(orcs[k], states[k], entries[k][1:])
        d = cc.worst_deviation(recs[k], exp, show=f"N {N}", floor=cc.eps_floor(states[k], COORD_NORMAL))
        assert d <= TOL, (N, d)
        assert np.array_equal(recs[k]["sigma_diag"], exp["sigma_diag"]) and np.array_equal(recs[k]["ids"], exp["ids"])


# ------------------------------------------------------------------------------------------------ 7. predictions, estimates, augment, copy
def test_predictions_estimates_augment_copy():
    sn = bn.normal()
    rng = np.random.default_rng(43)
    scs = [bs.make(sn, f"p{N}", 8100 + N, N) for N in (1, 17, 64)]
    batch = bn.make_batch(sn, 5)
    orcs = []
    for k, sc in enumerate(scs):
        batch.slot(k).force_eqf(*sc.state, sc.Sigma)
        orc = OracleFilter(sn)
        orc.set_eqf(*sc.state, sc.Sigma)
        orcs.append(orc)
    cam = bs.PINHOLE
    rec, status = batch.predictions([(k, cam, np.zeros((0, 13)), np.zeros(0)) for k in range(3)])
    assert np.all(status == 0)
    est, _, st2 = batch.state_estimates([0, 1, 2])
    assert np.all(st2 == 0)
    for k, sc in enumerate(scs):
        r = rec[k].trimmed()
        sensor, ids, p = orcs[k].state_estimate()
        want = orcs[k].output_cov_all(cam)
        d_cov = float(np.max(np.abs(r["out_cov"] - want))) / np.abs(want).max()
        d_p = float(np.max(np.abs(r["p"] - p) / np.maximum(1.0, np.abs(p))))
        d_s = float(np.max(np.abs(r["sensor"] - sensor) / np.maximum(1.0, np.abs(sensor))))
        print(f"N {sc.N}: out_cov {d_cov:.2e} of its largest entry, p {d_p:.2e}, sensor {d_s:.2e}")
        np.testing.assert_allclose(r["out_cov"], want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
        assert np.array_equal(r["ids"], ids) and d_p <= TOL and d_s <= TOL
        e = est[k].trimmed()
        s1, i1, p1 = batch.slot(k).state_estimate()
        assert np.array_equal(e["sensor"], s1) and np.array_equal(e["ids"], i1)
        assert np.array_equal(e["sigma_sensor"], batch.slot(k).get_sigma()[:21, :21])
        assert np.max(np.abs(e["p"] - p1)) <= 1e-12 * max(1.0, np.abs(p1).max())
    # augmentLandmarkStates on a Normal slot against the oracle: kept landmarks gathered, new ones with initialPointVariance I
    keep = scs[2].state[2][::2]
    fresh = (10 ** 5 + np.arange(10)).astype(np.int32)
    new_ids = np.concatenate([keep, fresh]).astype(np.int32)
    pts = rng.uniform(-1, 1, (10, 3)) * 3.0 + np.array([0, 0, 8.0])
    assert batch.augment_landmark_states([(2, new_ids, fresh, pts)])[0] == 0
    orcs[2].augment_landmark_states(new_ids, np.zeros(23), fresh, pts)
    assert max(parity(batch.slot(2), orcs[2])) < TOL and rel_fro(batch.slot(2).get_sigma(), orcs[2].get_sigma()) == 0.0
    # copy_slots between Normal slots: bit for bit
    assert batch.copy_slots([(2, 3), (1, 4)]) == [0, 0]
    assert same_bytes(arrays(batch.slot(3)), arrays(batch.slot(2))) and same_bytes(arrays(batch.slot(4)), arrays(batch.slot(1)))
    assert batch.slot_chart(3) == COORD_NORMAL


# ------------------------------------------------------------------------------------------------ 8. the chart rules
def test_chart_rules():
    sn = bn.normal()
    sc = bs.make(sn, "rules", 8200, 12)
    batch = VIOFilterBatch(bn.batch_settings(sn), 4, 64)
    core = BatchCore.of(batch)
    assert [batch.slot_chart(k) for k in range(4)] == [COORD_EUCLIDEAN] * 4
    batch.slot(0).chart = COORD_NORMAL  # accepted on an empty slot
    assert batch.slot(0).chart == COORD_NORMAL and batch.get_slot_settings(0).coordinateChoice == COORD_NORMAL and core.slot_chart(0) == COORD_NORMAL
    assert batch.get_slot_settings(1).coordinateChoice == COORD_EUCLIDEAN
    batch.slot(0).force_eqf(*sc.state, sc.Sigma)
    batch.slot(1).force_eqf(*sc.state, sc.Sigma)
    before = [arrays(batch.slot(k)) for k in range(2)]
    for k, chart in ((0, COORD_EUCLIDEAN), (0, COORD_INVDEPTH), (1, COORD_NORMAL)):  # a slot with landmarks keeps its chart
        with pytest.raises(BatchError) as err:
            batch.set_slot_chart(k, chart)
        assert err.value.code == EQF_E_BAD_ARG
    with pytest.raises(BatchError) as err:
        batch.set_slot_chart(None, COORD_NORMAL)  # every slot or none
    assert err.value.code == EQF_E_BAD_ARG and [batch.slot_chart(k) for k in range(4)] == [COORD_NORMAL, COORD_EUCLIDEAN, COORD_EUCLIDEAN, COORD_EUCLIDEAN]
    batch.set_slot_chart(0, COORD_NORMAL)  # its own chart: accepted, nothing happens
    for k in range(2):
        assert same_bytes(arrays(batch.slot(k)), before[k])
    # the settings calls still refuse Normal; an accepted one replaces the chart under the existing rule
    with pytest.raises(BatchError) as err:
        batch.set_slot_settings(2, sn)
    assert err.value.code == EQF_E_UNSUPPORTED
    batch.set_slot_chart(2, COORD_NORMAL)
    batch.set_slot_settings(2, bn.with_chart(sn, COORD_INVDEPTH))
    assert batch.slot_chart(2) == COORD_INVDEPTH
    with pytest.raises(BatchError) as err:
        batch.set_slot_settings(0, bn.with_chart(sn, COORD_INVDEPTH))  # slot 0 holds landmarks under Normal
    assert err.value.code == EQF_E_BAD_ARG and batch.slot_chart(0) == COORD_NORMAL
    # a copy from a Normal slot into a Euclidean slot with landmarks, and into an empty InvDepth one: the chart rule; an empty Normal source copies anywhere
    assert batch.copy_slots([(0, 1), (0, 2)]) == [EQF_E_BAD_ARG, EQF_E_BAD_ARG]
    assert same_bytes(arrays(batch.slot(1)), before[1])
    batch.set_slot_chart(3, COORD_NORMAL)
    assert batch.copy_slots([(0, 3), (3, 2)]) == [0, 0] and same_bytes(arrays(batch.slot(3)), before[0])
    # the bridge: a Normal context is refused whole, a Normal slot with landmarks does not go into a Euclidean context
    ctx_n, ctx_e = EqfCore(16, COORD_NORMAL), EqfCore(16, COORD_EUCLIDEAN)
    with pytest.raises(BatchError) as err:
        batch.load_core(ctx_n, [3])
    assert err.value.code == EQF_E_UNSUPPORTED
    elib = batch.elib
    assert elib.eqf_batch_store_ctx(batch.core_handle(), 0, ctx_n.h) == EQF_E_UNSUPPORTED
    assert elib.eqf_batch_store_ctx(batch.core_handle(), 0, ctx_e.h) == EQF_E_BAD_ARG
    assert same_bytes(arrays(batch.slot(0)), before[0]) and same_bytes(arrays(batch.slot(3)), before[0])


def test_chart_and_slot_checked_on_a_batch():
    """a chart outside the enum and a bad slot through the C-ABI of the filter level, slot < 0 included"""
    import ctypes as C

    from eqvio_amd.batch import load_batch_protos

    _, flib = load_batch_protos()
    s = Settings.defaults()
    s.coordinateChoice, s.fastRiccati = COORD_INVDEPTH, 1
    h = C.c_void_p()
    assert flib.eqvio_batch_create(C.byref(h), C.byref(s), 0, 3, 8) == 0
    try:
        assert [flib.eqvio_batch_get_slot_chart(h, k) for k in range(3)] == [COORD_INVDEPTH] * 3
        for chart in (3, -1):
            assert flib.eqvio_batch_set_slot_chart(h, 1, chart) == EQF_E_BAD_ARG and flib.eqvio_batch_set_slot_chart(h, -1, chart) == EQF_E_BAD_ARG
        assert flib.eqvio_batch_set_slot_chart(h, 3, COORD_NORMAL) == EQF_E_BAD_ARG and flib.eqvio_batch_get_slot_chart(h, 3) == EQF_E_BAD_ARG
        assert [flib.eqvio_batch_get_slot_chart(h, k) for k in range(3)] == [COORD_INVDEPTH] * 3
        assert flib.eqvio_batch_set_slot_chart(h, 1, COORD_NORMAL) == 0
        assert [flib.eqvio_batch_get_slot_chart(h, k) for k in range(3)] == [COORD_INVDEPTH, COORD_NORMAL, COORD_INVDEPTH]
        assert flib.eqvio_batch_set_slot_chart(h, -1, COORD_EUCLIDEAN) == 0 and [flib.eqvio_batch_get_slot_chart(h, k) for k in range(3)] == [COORD_EUCLIDEAN] * 3
    finally:
        flib.eqvio_batch_destroy(h)


# ------------------------------------------------------------------------------------------------ 9. a simulated sequence and the tool
def test_simulated_sequence_teacher_forced():
    """four slots with the charts E / I / N / N on four simulated sequences, starting without landmarks, every slot against its own oracle"""
    base = bs.shipped_euroc()
    charts = [COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, COORD_NORMAL]
    B, F = 4, 20
    ws = [SimWorld(seed=700 + k, num_points=600, max_features=12, trajectory=("wave" if k % 2 == 0 else "hover"), noise_px=2.0) for k in range(B)]
    batch = VIOFilterBatch(bn.batch_settings(base), B, 64)
    orcs = []
    for k, w in enumerate(ws):
        batch.set_slot_chart(k, charts[k])
        sensor = w.true_state(0.0, NONE)[0]
        batch.start_slot(k, sensor, NONE, np.zeros((0, 3)), 0.0)
        orcs.append(OracleFilter(bn.with_chart(base, charts[k]), sensor, NONE, np.zeros((0, 3)), 0.0))
    worst, seen = [[0.0, 0.0] for _ in range(B)], 0
    for frame in zip(*[w.frames(F) for w in ws]):
        entries = []
        for k, (imus, stamp, mid, y) in enumerate(frame):
            for imu in imus:
                batch.process_imu(k, imu)
                orcs[k].process_imu(imu)
            entries.append((k, stamp, ws[k].cam, mid, y))
        assert np.all(batch.process_vision(entries) == 0)
        for (k, stamp, cam, mid, y) in entries:
            orcs[k].process_vision(stamp, cam, mid, y)
            e = parity(batch.slot(k), orcs[k])  # asserts identical ids
            worst[k] = [max(worst[k][0], e[0]), max(worst[k][1], e[1])]
            seen |= batch.last_result(k)[0]
            teacher_force(batch.slot(k), orcs[k])
    print("worst parity per slot (E, I, N, N):", [[f"{v:.2e}" for v in w] for w in worst], "flags seen", seen)
    assert max(max(w) for w in worst) < TOL, worst
    assert seen & UPDATED and seen & ADDED


def test_eqvio_sim_batch_chart():
    sim = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    out = subprocess.run([sim, "--batch", "3", "--fastRiccati", "1", "--batchChart", "euclidean,invdepth,normal", "--duration", "1.0", "--maxFeatures", "12", "--numWalls", "4",
                          "--quiet"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(r"run (\d+) seed (\d+) chart (euclidean|invdepth|normal): mean NEES (\S+) over (\d+) frames", out.stdout)
    assert [r[2] for r in rows] == ["euclidean", "invdepth", "normal"] and len({r[1] for r in rows}) == 3, out.stdout
    assert all(np.isfinite(float(r[3])) for r in rows) and len({r[3] for r in rows}) == 3
    # the same seed in every slot (a sweep whose values are equal): the chart is then the only difference between the runs
    out = subprocess.run([sim, "--batch", "3", "--fastRiccati", "1", "--batchChart", "euclidean,invdepth,normal", "--duration", "1.0", "--maxFeatures", "12", "--numWalls", "4",
                          "--seed", "5", "--sweep", "measurementNoise=1.5,1.5,1.5", "--quiet"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(r"run (\d+) seed 5 measurementNoise=1.5 chart (euclidean|invdepth|normal): mean NEES (\S+) over (\d+) frames", out.stdout)
    assert [r[:2] for r in rows] == [("0", "euclidean"), ("1", "invdepth"), ("2", "normal")], out.stdout
    means = [float(r[2]) for r in rows]
    print("mean NEES of the same seed under the three charts:", means)
    assert all(np.isfinite(means)) and len(set(means)) == 3 and int(rows[0][3]) >= 5
