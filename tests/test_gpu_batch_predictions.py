"""The filter batch's feature predictions (eqf_batch_predictions, k_batch_predict; eqvio_batch_feature_predictions) on the GPU, against the CPU oracle:
stateEstimate taken through integrateSystemFunction step by step and projected (VIO_eqf::predictState, measureSystemState), getOutputCovById for every
landmark, and the oracle filter's own getFeaturePredictions; on both buffer halves, read-only, independent of the call a slot is part of; the refusals; packet
growth; and `eqvio_opt --batch B --predictions` against the same loop over the Python API.

Tolerances (set by the issue, from the suite's existing rules):
  sensor, p   the project's flat 1e-9 relative to max(1, |.|): a few dozen fp64 operations per step on numbers of size <= 30; the device applies the steps'
              folded pose T to a point, the oracle the steps' poses one by one - the same quantity in another order of operations;
  y           atol 1e-7 px: 1e-9 of O(100) px (tests/test_gpu_filter.py::test_feature_predictions_match). The projection divides by depth, so the tests first
              assert, by the oracle alone, that every predicted point has z >= 0.5 and |x / z|, |y / z| <= 1: the division then amplifies p's error by
              at most f / z * 2 <= 2000, which 1e-14-sized errors of p leave far below the bound;
  out_cov     rtol 1e-10, atol 1e-12 max|oracle|, symmetric to 1e-13 max (tests/test_gpu_parity.py::test_output_cov_all)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
from batch_scenarios import shipped_euroc
from eqvio_amd.batch import BatchPredictionEntry, BatchPredictionRecord, VIOFilterBatch
from eqvio_amd.capi import COORD_INVDEPTH, Settings, c_double_p
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter, load_oracle, oracle_cam_project
from test_gpu_batch_estimates import PLANTED, planted, planted_batch, slot_snapshot  # noqa: F401  (planted is a fixture)
from test_gpu_batch_filter import run_lockstep, start_empty, worlds
from util import euroc_camera, euroc_radtan_camera, imu_selection, random_imu, teacher_force, uzhfpv_equidistant_camera

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM, OPT = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
EQF_E_BAD_ARG = -3
TOL, TOL_PX = 1e-9, 1e-7
REC = C.sizeof(BatchPredictionRecord)
CAMS = {"pinhole": euroc_camera(), "radtan": euroc_radtan_camera(), "equidistant": uzhfpv_equidistant_camera()}


def record_bytes(rec, e):
    return C.string_at(C.addressof(rec[e]), REC)


def dev(a, b):
    """worst entry of |a - b| relative to max(1, |b|)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def steps_for(rng, k):
    """k IMU samples (bias velocities included) and their dts; one dt of a three-step list is 0"""
    imus = np.stack([random_imu(rng, stamp=0.01 * j, bias_vel=True) for j in range(k)]) if k else np.zeros((0, 13))
    dts = {0: [], 1: [0.02], 3: [0.015, 0.0, 0.025]}.get(k, [0.01] * k)
    return imus, np.array(dts, float)


def expected(orc, cam, imus, dts):
    """what the oracle alone makes of a prediction request: predictState's loop over integrateSystemFunction, measureSystemState, getOutputCovById. The
    conditioning the projection checks rest on is asserted here."""
    lib = load_oracle()
    sensor, ids, p = orc.state_estimate()
    sensor, p = sensor.copy(), np.ascontiguousarray(p, dtype=np.float64).copy()
    for u, dt in zip(imus, dts):
        u = np.ascontiguousarray(u, dtype=np.float64)
        lib.orc_integrate_system_function(sensor.ctypes.data_as(c_double_p), ids.ctypes.data_as(C.POINTER(C.c_int)), p.ctypes.data_as(c_double_p), len(ids),
                                          u.ctypes.data_as(c_double_p), float(dt))
    if len(ids):
        assert np.min(p[:, 2]) >= 0.5 and np.max(np.abs(p[:, :2] / p[:, 2:3])) <= 1.0, "a planted landmark leaves the well-conditioned cone: plant other points"
    y = np.array([oracle_cam_project(cam, q) for q in p]).reshape(-1, 2)
    return dict(sensor=sensor, ids=ids, p=p, y=y, out_cov=orc.output_cov_all(cam))


def check_record(rec, want, show="", sigma_symmetric=True):
    """one record against expected(); returns the deviations (sensor, p, y in px, out_cov relative to its largest entry). v01 and v10 of an output covariance
    are separate sums of C0 Sigma_ii C0^T: they agree to rounding where Sigma_ii is symmetric, which a planted Sigma is exactly (sigma_symmetric)."""
    r = rec.trimmed()
    N = len(want["ids"])
    assert rec.N == N and rec.reserved == 0
    assert np.array_equal(r["ids"], want["ids"])
    assert not np.any(np.array(rec.ids)[N:]) and not np.any(np.array(rec.p)[3 * N:]) and not np.any(np.array(rec.y)[2 * N:]) and not np.any(np.array(rec.out_cov)[4 * N:])
    d = [dev(r["sensor"], want["sensor"]), dev(r["p"], want["p"]), float(np.max(np.abs(r["y"] - want["y"]))) if N else 0.0, 0.0]
    if N:
        g, o = r["out_cov"], want["out_cov"]
        d[3] = float(np.max(np.abs(g - o))) / np.abs(o).max()
        print(f"{show} N {N}: sensor {d[0]:.2e}, p {d[1]:.2e}, y {d[2]:.2e} px, out_cov {d[3]:.2e} of its largest entry")
        np.testing.assert_allclose(g, o, rtol=1e-10, atol=1e-12 * np.abs(o).max())
        if sigma_symmetric:
            assert np.allclose(g, np.transpose(g, (0, 2, 1)), rtol=0, atol=1e-13 * np.abs(g).max())
    assert d[0] <= TOL and d[1] <= TOL and d[2] <= TOL_PX, (show, d)
    return d


def test_planted_slots_in_one_call(planted):
    batch = planted_batch(planted)
    rng = np.random.default_rng(15)
    order = [6, 2, 7, 0, 4, 1, 3]  # a permutation, count < B; slot 5 is not listed
    ks = [3, 0, 1, 1, 0, 3, 3]
    cam = CAMS["pinhole"]
    reqs = [steps_for(rng, k) for k in ks]
    want = [expected(planted[s]["orc"], cam, *reqs[e]) for e, s in enumerate(order)]  # the conditioning, by the oracle alone, before the device is asked
    rec, status = batch.predictions([(s, cam, *reqs[e]) for e, s in enumerate(order)])
    assert np.all(status == 0)
    worst = np.zeros(4)
    for e, s in enumerate(order):
        assert rec[e].N == planted[s]["N"]
        worst = np.maximum(worst, check_record(rec[e], want[e], show=f"slot {s} chart {planted[s]['chart']} k {ks[e]}"))
        if ks[e] == 0:  # the current estimate: eqf_batch_state_estimate's sensor bit for bit, its p to rounding
            se, ids, p = batch.slot(s).state_estimate()
            assert np.array(rec[e].sensor).tobytes() == se.tobytes() and dev(rec[e].trimmed()["p"], p) <= TOL
    print(f"worst: sensor {worst[0]:.2e}, p {worst[1]:.2e}, y {worst[2]:.2e} px, out_cov {worst[3]:.2e}")
    # out_cov does not depend on the steps
    again, status = batch.predictions([(s, cam, *steps_for(rng, 0)) for s in order])
    assert np.all(status == 0)
    for e in range(len(order)):
        assert np.array(again[e].out_cov).tobytes() == np.array(rec[e].out_cov).tobytes()


def test_three_camera_models_in_one_call(planted):
    batch = planted_batch(planted)
    rng = np.random.default_rng(16)
    slots = [2, 4, 5, 7]  # N = 5 and 64, both charts
    for name, cam in CAMS.items():
        reqs = [steps_for(rng, 3) for _ in slots]
        want = [expected(planted[s]["orc"], cam, *reqs[e]) for e, s in enumerate(slots)]
        rec, status = batch.predictions([(s, cam, *reqs[e]) for e, s in enumerate(slots)])
        assert np.all(status == 0)
        for e, s in enumerate(slots):
            check_record(rec[e], want[e], show=f"{name} slot {s}")
    # and the three models among the entries of ONE call
    names = ["pinhole", "radtan", "equidistant", "radtan"]
    reqs = [steps_for(rng, 1) for _ in slots]
    want = [expected(planted[s]["orc"], CAMS[names[e]], *reqs[e]) for e, s in enumerate(slots)]
    rec, status = batch.predictions([(s, CAMS[names[e]], *reqs[e]) for e, s in enumerate(slots)])
    assert np.all(status == 0)
    for e, s in enumerate(slots):
        check_record(rec[e], want[e], show=f"mixed {names[e]} slot {s}")


def test_both_buffer_halves(planted):
    rng = np.random.default_rng(17)
    cam = CAMS["radtan"]
    # (a) a slot that copy_slots just wrote: the copy goes into the destination's other buffer pair
    c = planted[3]  # N = 63, InvDepth
    batch = planted_batch(planted, B=2, at=[(0, c)])
    batch.set_slot_settings(1, c["settings"])
    assert batch.copy_slots([(0, 1)]) == [0]
    req = steps_for(rng, 3)
    want = expected(c["orc"], cam, *req)
    rec, status = batch.predictions([(1, cam, *req), (0, cam, *req)])
    assert np.all(status == 0)
    check_record(rec[0], want, show="copied")
    check_record(rec[1], want, show="source")
    assert record_bytes(rec, 0) == record_bytes(rec, 1)
    # (b) a slot after a real step that dropped an invalid landmark (removeInvalidLandmarks compacts into the other pair): test_gpu_batch_estimates.py's pattern
    s = shipped_euroc()
    ws = worlds(1, "pinhole")
    batch = VIOFilterBatch(s, 1, 64)
    orcs = start_empty(batch, s, ws)
    frames = [list(w.frames(9)) for w in ws]
    run_lockstep(batch, [0], orcs, [f[:8] for f in frames], ws, check=False)
    xi0, Xs, ids, q0, Q = orcs[0].get_eqf()
    victim = [i for i, lid in enumerate(ids) if lid in set(frames[0][8][2].tolist())][0]
    Q[victim, 4] = 5e-9
    S = orcs[0].get_sigma()
    orcs[0].set_eqf(xi0, Xs, ids, q0, Q, S, time=frames[0][7][1])
    batch.slot(0).force_eqf(xi0, Xs, ids, q0, Q, S)
    flags = []
    run_lockstep(batch, [0], orcs, [f[8:9] for f in frames], ws, check=False, statuses=flags)  # teacher forced: the slot holds the oracle's state
    assert flags[0][0] & 32, flags
    req = steps_for(rng, 1)
    want = expected(orcs[0], ws[0].cam, *req)
    rec, status = batch.predictions([(0, ws[0].cam, *req)])
    assert status[0] == 0 and rec[0].N >= 10 and ids[victim] not in rec[0].trimmed()["ids"].tolist()
    # This Sigma went through a real update and is symmetric to about 1e-17 only; rows of C0 of size 1e2 .. 1e3 carry that into v01 - v10, and the oracle's own
    # output covariances are asymmetric to 5.8e-12 of their largest entry here. So no symmetry is asked of this record: entry by entry it is still the oracle's.
    check_record(rec[0], want, show="after removeInvalidLandmarks", sigma_symmetric=False)


def test_read_only(planted):
    # slots with a history: a few simulated frames (innovation totals, last result), then the calls
    s = shipped_euroc(useFeaturePredictions=1)
    B = 3
    ws = [SimWorld(seed=500 + k, num_points=600, max_features=30, noise_px=1.0) for k in range(B)]
    batch = VIOFilterBatch(s, B, 64)
    for k, w in enumerate(ws):
        batch.start_slot(k, w.true_state(0.0, np.zeros(0, np.int32))[0], np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    stamp = 0.0
    for j, frame in enumerate(zip(*[w.frames(5) for w in ws])):
        entries = []
        for k, (imus, stamp, mid, y) in enumerate(frame):
            for imu in imus:
                batch.process_imu(k, imu)
            entries.append((k, stamp, ws[k].cam, mid, y))
        if j == 4:
            break  # the last frame's IMU samples are buffered, its measurement is not processed
        assert np.all(batch.process_vision(entries) == 0)
    before = [slot_snapshot(batch, k) for k in range(B)]
    times = [batch.slot(k).get_time() for k in range(B)]
    assert all(b[-2][0] > 0 for b in before)  # the totals are not empty
    rng = np.random.default_rng(18)
    rec1, st1 = batch.feature_predictions([(k, ws[k].cam, stamp) for k in (2, 0, 1)])
    rec2, st2 = batch.feature_predictions([(k, ws[k].cam, stamp) for k in (2, 0, 1)])
    rec3, st3 = batch.predictions([(k, ws[k].cam, *steps_for(rng, 3)) for k in (1, 2, 0)])
    assert np.all(st1 == 0) and np.all(st2 == 0) and np.all(st3 == 0) and rec1[0].N > 10
    assert bytes(rec1) == bytes(rec2)
    assert before == [slot_snapshot(batch, k) for k in range(B)] and times == [batch.slot(k).get_time() for k in range(B)]
    assert np.all(batch.process_vision(entries) == 0)  # the buffered samples are still there: the frame runs
    assert all(batch.last_result(k)[0] & 16 for k in range(B))
    # the planted batch: every slot untouched by a call over all of them
    pb = planted_batch(planted)
    before = [slot_snapshot(pb, k) for k in range(8)]
    _, st8 = pb.predictions([(k, CAMS["equidistant"], *steps_for(rng, 1)) for k in range(8)])
    assert np.all(st8 == 0) and before == [slot_snapshot(pb, k) for k in range(8)]


def test_record_does_not_depend_on_its_call(planted):
    rng = np.random.default_rng(19)
    cam = CAMS["radtan"]
    req = steps_for(rng, 3)
    others = [steps_for(rng, 1) for _ in range(8)]
    for c in (planted[5], planted[3], planted[2]):  # N = 64 InvDepth, 63 InvDepth, 5 Euclidean
        one = planted_batch(planted, B=1, at=[(0, c)])
        alone, st = one.predictions([(0, cam, *req)])
        assert st[0] == 0 and alone[0].N == c["N"]
        eight = planted_batch(planted, B=8, at=[(k, c if k == 5 else planted[k]) for k in range(8)])
        rest = [k for k in range(8) if k != 5]
        first, st = eight.predictions([(5, cam, *req)] + [(k, CAMS["pinhole"], *others[k]) for k in rest])
        assert np.all(st == 0)
        last, st = eight.predictions([(k, CAMS["equidistant"], *others[k]) for k in rest] + [(5, cam, *req)])
        assert np.all(st == 0)
        assert record_bytes(alone, 0) == record_bytes(first, 0) == record_bytes(last, 7)


def test_refusals_on_the_device(planted):
    batch = planted_batch(planted)
    rng = np.random.default_rng(20)
    cam = CAMS["pinhole"]
    imus, dts = steps_for(rng, 3)
    neg, nan = dts.copy(), dts.copy()
    neg[1], nan[2] = -1e-3, np.nan
    bad_cam = type(cam).from_buffer_copy(cam)
    bad_cam.model = 7
    # (slot, cam, k, samples, dts): slot 4 twice, slot 8 and -1 out of range, k = -1, k = 2 without samples, a negative and a NaN dt, a bad camera
    spec = [(4, cam, 3, imus, dts), (8, cam, 0, None, None), (1, cam, -1, imus, dts), (4, cam, 0, None, None), (3, cam, 2, None, dts), (2, cam, 3, imus, neg),
            (5, cam, 3, imus, nan), (-1, cam, 0, None, None), (6, cam, 2, imus, None), (7, bad_cam, 0, None, None), (0, cam, 1, imus, dts)]
    accepted = {0: 4, 10: 0}  # entry -> slot
    n = len(spec)
    ent = (BatchPredictionEntry * n)()
    for e, (slot, c, k, u, d) in enumerate(spec):
        ent[e].slot, ent[e].cam, ent[e].k = slot, c, k
        ent[e].imu13_k = u.ctypes.data_as(c_double_p) if u is not None else None
        ent[e].dt_k = d.ctypes.data_as(c_double_p) if d is not None else None
    rec = (BatchPredictionRecord * n)()
    C.memset(rec, 0xA5, C.sizeof(rec))
    status = (C.c_int * n)()
    want = {e: expected(planted[s]["orc"], cam, imus[: spec[e][2]], dts[: spec[e][2]]) for e, s in accepted.items()}
    assert batch.elib.eqf_batch_predictions(batch.core_handle(), n, ent, rec, status) == 0
    assert list(status) == [0 if e in accepted else EQF_E_BAD_ARG for e in range(n)]
    for e in range(n):
        if e in accepted:
            check_record(rec[e], want[e], show=f"entry {e}")
        else:
            assert record_bytes(rec, e) == b"\xa5" * REC, e
    # count == 0 touches nothing; null arguments with count > 0, and count < 0, are refused
    C.memset(rec, 0xA5, C.sizeof(rec))
    assert batch.elib.eqf_batch_predictions(batch.core_handle(), 0, None, None, None) == 0
    assert batch.elib.eqf_batch_predictions(batch.core_handle(), 0, ent, rec, status) == 0 and bytes(rec) == b"\xa5" * C.sizeof(rec)
    assert batch.elib.eqf_batch_predictions(batch.core_handle(), 1, None, rec, status) == EQF_E_BAD_ARG
    assert batch.elib.eqf_batch_predictions(batch.core_handle(), 1, ent, None, status) == EQF_E_BAD_ARG
    assert batch.elib.eqf_batch_predictions(batch.core_handle(), 1, ent, rec, None) == EQF_E_BAD_ARG
    assert batch.elib.eqf_batch_predictions(batch.core_handle(), -1, ent, rec, status) == EQF_E_BAD_ARG
    # filter level: a slot listed twice and a slot out of range, among entries that are done
    recs = (BatchPredictionRecord * 4)()
    C.memset(recs, 0xA5, C.sizeof(recs))
    for k in range(8):
        s = batch.get_slot_settings(k)
        s.useFeaturePredictions = 1
        batch.set_slot_settings(k, s)
    recs, st = batch.feature_predictions([(2, cam, 0.5), (2, cam, 0.5), (9, cam, 0.5), (7, cam, 0.5)], recs)
    assert st.tolist() == [0, EQF_E_BAD_ARG, EQF_E_BAD_ARG, 0]
    assert record_bytes(recs, 1) == record_bytes(recs, 2) == b"\xa5" * REC
    for e, k in ((0, 2), (3, 7)):  # the planted slots have no IMU sample: the current estimate
        check_record(recs[e], expected(planted[k]["orc"], cam, [], []), show=f"filter level, slot {k}")


def test_packets_grow_and_are_reused():
    """tests/test_gpu_batch_packets.py's pattern: 66 slots (more than any packet holds when the batch is made), calls with 1, 66 and 1 entries; slots 0 and 65
    must give the bytes the same planted slot gives alone in a fresh one-slot batch."""
    B, LAST = 66, 65
    s = shipped_euroc()
    scs = [bs.make(s, f"predict{k}", 9500 + k, 2, k=4) for k in range(B)]
    reqs = [(sc.cam, sc.imus, imu_selection(sc.imus, sc.t0, sc.stamp)[0]) for sc in scs]
    big = VIOFilterBatch(s, B, 64)
    for k, sc in enumerate(scs):
        big.slot(k).force_eqf(*sc.state, sc.Sigma)
    want = {}
    for k in (0, LAST):
        one = VIOFilterBatch(s, 1, 64)
        one.slot(0).force_eqf(*scs[k].state, scs[k].Sigma)
        rec, st = one.predictions([(0, *reqs[k])])
        assert st[0] == 0 and rec[0].N == 2 and np.all(np.isfinite(rec[0].trimmed()["y"]))
        want[k] = record_bytes(rec, 0)
    assert want[0] != want[LAST]
    for slots in ([0], list(range(B)), [LAST]):
        rec, st = big.predictions([(k, *reqs[k]) for k in slots])
        assert np.all(st == 0)
        for k in want:
            if k in slots:
                assert record_bytes(rec, slots.index(k)) == want[k], (len(slots), k)


def test_filter_level_follows_the_oracle_filter():
    on, off = shipped_euroc(useFeaturePredictions=1), shipped_euroc()
    ws = [SimWorld(seed=900 + k, num_points=800, max_features=25, trajectory="wave" if k == 0 else "hover", noise_px=0.5) for k in range(2)]
    batch = VIOFilterBatch(on, 3, 64)
    batch.set_slot_settings(2, off)
    orcs = {}
    for k in range(3):
        w = ws[k % 2]
        sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
        batch.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        orcs[k] = OracleFilter(on, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    checked, worst = [0, 0], 0.0
    for frame in zip(*[w.frames(12) for w in ws]):
        frame = list(frame) + [frame[0]]  # slot 2 runs slot 0's sequence with the predictions switched off
        entries = []
        for k, (imus, stamp, mid, y) in enumerate(frame):
            for imu in imus:
                batch.process_imu(k, imu)
                orcs[k].process_imu(imu)
            entries.append((k, stamp, ws[k % 2].cam, mid, y))
        # the IMU buffers now reach the image stamps: ONE call for the three slots, before the step
        rec, st = batch.feature_predictions([(k, cam, stamp) for (k, stamp, cam, _, _) in entries])
        assert np.all(st == 0)
        for k in range(2):
            io, yo = orcs[k].get_feature_predictions(entries[k][2], entries[k][1])
            r = rec[k].trimmed()
            order = np.argsort(r["ids"], kind="stable")  # the oracle's measurement is a map: ascending ids
            assert np.array_equal(r["ids"][order], io)
            if len(io):
                worst = max(worst, float(np.max(np.abs(r["y"][order].reshape(-1) - yo))))
                ids_b, y_b, cov_b = batch.slot(k).feature_predictions(entries[k][2], entries[k][1])
                assert np.array_equal(ids_b, r["ids"]) and y_b.tobytes() == r["y"].tobytes() and cov_b.tobytes() == r["out_cov"].tobytes()
                cov_o = orcs[k].output_cov_all(entries[k][2])
                np.testing.assert_allclose(r["out_cov"], cov_o, rtol=1e-10, atol=1e-12 * np.abs(cov_o).max())
            checked[k] += len(io)
        # the slot with the predictions off: the reference's empty measurement, its sensor still the current estimate
        assert rec[2].N == 0 and not np.any(np.array(rec[2].ids)) and not np.any(np.array(rec[2].p)) and not np.any(np.array(rec[2].y)) and not np.any(np.array(rec[2].out_cov))
        assert np.array(rec[2].sensor).tobytes() == batch.slot(2).state_estimate()[0].tobytes()
        assert np.all(batch.process_vision(entries) == 0)
        for (k, stamp, cam, mid, y) in entries:
            orcs[k].process_vision(stamp, cam, mid, y)
            teacher_force(batch.slot(k), orcs[k])
    print(f"filter level: {checked} predictions checked, worst pixel deviation {worst:.2e}")
    assert min(checked) >= 100, checked
    assert worst <= TOL_PX, worst
    # a call whose listed slots all have the predictions off launches nothing: records all zero apart from sensor
    quiet = VIOFilterBatch(off, 2, 64)
    c = bs.make(off, "quiet", 77, 5)
    for k in range(2):
        quiet.slot(k).force_eqf(*c.state, c.Sigma)
    rec, st = quiet.feature_predictions([(1, c.cam, 1.0), (0, c.cam, 1.0)])
    assert np.all(st == 0)
    for e, k in enumerate((1, 0)):
        assert np.array(rec[e].sensor).tobytes() == quiet.slot(k).state_estimate()[0].tobytes()
        rec[e].sensor[:] = [0.0] * 23
    assert bytes(rec) == bytes(2 * REC)


# ------------------------------------------------------------------------------------------------ the command line
PRED_LINE = r"slot (\d+) measurementNoise=(\S+): prediction RMSE (\S+) px over (\d+) features"


def test_eqvio_opt_predictions(tmp_path):
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([SIM, "--duration", "2", "--maxFeatures", "20", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    offset = [0.5, -0.5, 0.5, -0.5, 0.0, 0.0, 0.0]
    files = ["--imu", ds + "/imu.csv", "--features", run + "/features.csv"]
    values = ["0.5", "5"]
    replay = [OPT, *files, "--cameraOffset", *[repr(v) for v in offset], *common, "--batch", "2", "--sweep", "measurementNoise=" + ",".join(values)]
    with_p = subprocess.run(replay + ["--predictions"], capture_output=True, text=True, timeout=120)
    assert with_p.returncode == 0, with_p.stderr[-2000:]
    rows = re.findall(PRED_LINE, with_p.stdout)
    assert [(r[0], r[1]) for r in rows] == [("0", values[0]), ("1", values[1])], with_p.stdout
    # the same loop over the Python API: the IMU samples, ONE feature_predictions call, then the step
    meas = subprocess.run([OPT, *files, "--dumpMeasurements"], capture_output=True, text=True, timeout=60)
    assert meas.returncode == 0, meas.stderr
    cam = euroc_camera()  # eqvio_opt's default camera
    settings = []
    for v in values:
        s = Settings.defaults()
        s.coordinateChoice, s.fastRiccati, s.initialPointVariance, s.useMedianDepth, s.initialSceneDepth = COORD_INVDEPTH, 1, 1.0, 0, 3.0
        s.useFeaturePredictions, s.measurementNoise = 1, float(v)
        s.cameraOffset[:] = offset
        settings.append(s)
    batch = VIOFilterBatch(settings[0], 2, 64)
    batch.set_slot_settings(1, settings[1])
    sq, cnt, frames = [0.0, 0.0], [0, 0], 0
    for tok in (ln.split() for ln in meas.stdout.splitlines()):
        if tok[0] == "IMU":
            for k in range(2):
                batch.process_imu(k, np.array([float(v) for v in tok[1:8]] + [0.0] * 6))
            continue
        assert tok[0] == "IMG"
        M, stamp = int(tok[2]), float(tok[1])
        ids = np.array([int(tok[3 + 3 * j]) for j in range(M)], np.int32)
        y = np.array([[float(tok[4 + 3 * j]), float(tok[5 + 3 * j])] for j in range(M)])
        rec, st = batch.feature_predictions([(k, cam, stamp) for k in range(2)])
        assert np.all(st == 0)
        for k in range(2):
            r = rec[k].trimmed()
            for i, lid in enumerate(r["ids"].tolist()):
                j = np.flatnonzero(ids == lid)
                if len(j):
                    d = r["y"][i] - y[j[0]]
                    sq[k] += float(d[0]) * float(d[0]) + float(d[1]) * float(d[1])
                    cnt[k] += 1
        assert np.all(batch.process_vision([(k, stamp, cam, ids, y.reshape(-1)) for k in range(2)]) == 0)
        frames += 1
    assert frames >= 30 and min(cnt) >= 300, (frames, cnt)
    for k in range(2):
        got, n = float(rows[k][2]), int(rows[k][3])
        ref = np.sqrt(sq[k] / cnt[k])
        print(f"slot {k}: printed RMSE {got:.9g} px over {n} features, from the Python loop {ref:.9g} over {cnt[k]}")
        assert n == cnt[k]
        assert abs(got - ref) <= 1e-8 * ref, (k, got, ref)
    assert rows[0][2] != rows[1][2]  # the two tunings predict differently
    # without --predictions the run prints its other lines unchanged
    plain = subprocess.run(replay, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr[-2000:]
    timing = lambda t: re.sub(r"(Time taken: |updates/s )\S+", r"\1*", t)  # the two numbers of the output that are timings
    assert "prediction RMSE" not in plain.stdout
    assert [ln for ln in timing(with_p.stdout).splitlines() if "prediction RMSE" not in ln] == timing(plain.stdout).splitlines()
