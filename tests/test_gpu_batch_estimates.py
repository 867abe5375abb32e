"""The filter batch's estimate records (eqf_batch_estimates, k_batch_estimate) on the GPU: against eqf_batch_state_estimate / eqf_batch_get_sigma (N, ids, sensor
and the sensor block of Sigma bit for bit), against the CPU oracle's stateEstimate, on both buffer halves, read-only, independent of the batch a slot is in;
the recorded replay (eqvio_batch_run_prepared_recorded) against the same loop over the per-call API, and `eqvio_opt --batch B --record DIR --groundtruth FILE`.

Tolerance of p and p_world: the project's flat 1e-9 relative to max(1, |p|), entry by entry. Both sides form (1 / a) R(Q)^T q0 and R p + x in fp64 from the same
inputs - a few dozen operations on numbers of size <= 30, so each keeps about 1e-14; they differ by the order of operations and by fused multiply-adds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from batch_scenarios import reference_defaults, shipped_euroc
from eqvio_amd.batch import BatchEstimateRecord, VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, PreparedFrames
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from test_gpu_batch_filter import run_lockstep, start_empty, worlds
from test_gpu_batch_nees import eqf_arrays, plant, spd
from util import quat_mul, quat_rot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM, OPT = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
EQF_E_BAD_ARG = -3
TOL = 1e-9
FILES = ["IMUState.csv", "camera.csv", "bias.csv", "points.csv"]
E, I = COORD_EUCLIDEAN, COORD_INVDEPTH
PLANTED = [(0, E), (1, I), (5, E), (63, I), (64, E), (64, I), (63, E), (5, I)]  # (N, chart) of the 8 slots


def record_bytes(rec, e):
    return C.string_at(C.addressof(rec[e]), C.sizeof(BatchEstimateRecord))


def dev(a, b):
    """worst entry of |a - b| relative to max(1, |b|)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def world_points(sensor, p):
    """pose * cameraOffset * p in numpy, from the 23 sensor doubles and camera-frame points"""
    R = quat_mul(sensor[6:10], sensor[16:20])
    x = sensor[10:13] + quat_rot(sensor[6:10], sensor[20:23])
    return np.array([quat_rot(R, q) + x for q in p]).reshape(-1, 3)


def check_record(rec, slot, orc, show=""):
    """one record against the slot's per-call route (bit for bit where the issue says so) and against the oracle; returns the worst deviation of p / p_world"""
    r = rec.trimmed()
    s, ids, p = slot.state_estimate()
    N = len(ids)
    assert rec.N == N and rec.reserved == 0
    assert np.array_equal(r["ids"], ids)
    assert np.array(rec.sensor).tobytes() == s.tobytes()  # bit for bit
    assert r["sigma_sensor"].tobytes() == np.ascontiguousarray(slot.get_sigma()[:21, :21]).tobytes()  # bit for bit
    # entries beyond N read 0
    assert not np.any(np.array(rec.ids)[N:]) and not np.any(np.array(rec.p)[3 * N:]) and not np.any(np.array(rec.p_world)[3 * N:])
    so, ido, po = orc.state_estimate()
    assert np.array_equal(ido, ids)
    d = [dev(r["p"], p), dev(r["p"], po), dev(r["p_world"], world_points(so, po)), dev(r["sensor"], so)]
    print(f"{show} N {N}: p vs state_estimate {d[0]:.2e}, p vs oracle {d[1]:.2e}, p_world vs oracle {d[2]:.2e}, sensor vs oracle {d[3]:.2e}")
    return max(d)


@pytest.fixture(scope="module")
def planted():
    """the planted states, Sigmas and oracles of the 8 slots: computed once, shared, never changed"""
    rng = np.random.default_rng(1414)
    out = []
    for N, chart in PLANTED:
        s = reference_defaults(coordinateChoice=chart)
        st, V, lam = plant(rng, N, chart)
        S = spd(V, lam)
        orc = OracleFilter(s)
        orc.set_eqf(*st, S)
        out.append(dict(N=N, chart=chart, settings=s, state=st, S=S, orc=orc))
    return out


def planted_batch(planted, B=8, at=None):
    batch = VIOFilterBatch(planted[0]["settings"], B, 64)
    for k, c in enumerate(planted) if at is None else at:
        batch.set_slot_settings(k, c["settings"])
        batch.slot(k).force_eqf(*c["state"], c["S"])
    return batch


def test_planted_slots_in_one_call(planted):
    batch = planted_batch(planted)
    order = [6, 2, 7, 0, 4, 1, 3]  # a permutation, count < B; slot 5 is not listed
    rec, times, status = batch.state_estimates(order)
    assert np.all(status == 0) and np.all(times == -1.0)  # planted through the core: the slots have not initialised
    worst = 0.0
    for e, k in enumerate(order):
        c = planted[k]
        assert rec[e].N == c["N"]
        worst = max(worst, check_record(rec[e], batch.slot(k), c["orc"], show=f"slot {k} chart {c['chart']}"))
    assert worst <= TOL, worst


def test_both_buffer_halves(planted):
    # (a) a slot that copy_slots just wrote: the copy goes into the destination's other buffer pair
    c = planted[3]  # N = 63, InvDepth
    batch = planted_batch(planted, B=2, at=[(0, c)])
    batch.set_slot_settings(1, c["settings"])
    assert batch.copy_slots([(0, 1)]) == [0]
    rec, _, status = batch.state_estimates([1, 0])
    assert np.all(status == 0)
    worst = max(check_record(rec[0], batch.slot(1), c["orc"], show="copied"), check_record(rec[1], batch.slot(0), c["orc"], show="source"))
    assert record_bytes(rec, 0) == record_bytes(rec, 1)
    # (b) a slot after a step that dropped an invalid landmark (removeInvalidLandmarks compacts into the other pair): test_gpu_batch_filter.py's planted Q.a
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
    rec, times, status = batch.state_estimates([0])
    assert status[0] == 0 and times[0] == batch.slot(0).get_time() == frames[0][8][1]
    assert ids[victim] not in rec[0].trimmed()["ids"].tolist() and rec[0].N >= 10
    worst = max(worst, check_record(rec[0], batch.slot(0), orcs[0], show="after removeInvalidLandmarks"))
    assert worst <= TOL, worst


def slot_snapshot(batch, k):
    s = batch.get_slot_settings(k)
    fields = [np.array(getattr(s, name)).tobytes() for name, _ in s._fields_]  # field by field: padding bytes carry nothing
    return [a.tobytes() for a in eqf_arrays(batch.slot(k))] + [fields, batch.last_result(k), batch.last_innovation(k), batch.innovation_totals(k),
                                                              batch.nees_lu_fallbacks(k)]


def test_read_only_and_deterministic(planted):
    # slots with a history: a few simulated frames (innovation totals, last result), then the call
    s = shipped_euroc()
    B = 3
    ws = [SimWorld(seed=500 + k, num_points=600, max_features=30, noise_px=1.0) for k in range(B)]
    batch = VIOFilterBatch(s, B, 64)
    for k, w in enumerate(ws):
        batch.start_slot(k, w.true_state(0.0, np.zeros(0, np.int32))[0], np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    for frame in zip(*[w.frames(4) for w in ws]):
        entries = []
        for k, (imus, stamp, mid, y) in enumerate(frame):
            for imu in imus:
                batch.process_imu(k, imu)
            entries.append((k, stamp, ws[k].cam, mid, y))
        assert np.all(batch.process_vision(entries) == 0)
    before = [slot_snapshot(batch, k) for k in range(B)]
    assert all(b[-2][0] > 0 for b in before)  # the totals are not empty
    rec1, t1, st1 = batch.state_estimates([2, 0, 1])
    rec2, t2, st2 = batch.state_estimates([2, 0, 1])
    assert np.all(st1 == 0) and np.all(st2 == 0) and np.array_equal(t1, t2) and t1[0] == batch.slot(2).get_time() > 0
    assert rec1[0].N > 10
    assert bytes(rec1) == bytes(rec2)
    assert before == [slot_snapshot(batch, k) for k in range(B)]
    # the planted batch: every slot untouched by a call over all of them
    pb = planted_batch(planted)
    before = [slot_snapshot(pb, k) for k in range(8)]
    rec8, _, st8 = pb.state_estimates(list(range(8)))
    assert np.all(st8 == 0) and before == [slot_snapshot(pb, k) for k in range(8)]
    # a slot's record does not depend on the call or the batch: alone, last of 8, and in slot 5 of a batch of 70 with the same planted state
    alone, _, st = pb.state_estimates([7])
    assert st[0] == 0 and record_bytes(alone, 0) == record_bytes(rec8, 7)
    c = planted[7]
    big = planted_batch(planted, B=70, at=[(k, c if k == 5 else planted[k % 8]) for k in range(70)])
    rec70, _, st70 = big.state_estimates(list(range(69, -1, -1)))
    assert np.all(st70 == 0) and record_bytes(rec70, 64) == record_bytes(rec8, 7)  # entry 64 of the descending list is slot 5
    for k in (3, 5):  # the large planted sizes too
        c = planted[k]
        one = planted_batch(planted, B=1, at=[(0, c)])
        r1, _, s1 = one.state_estimates([0])
        assert s1[0] == 0 and record_bytes(r1, 0) == record_bytes(rec8, k)


def test_refusals_on_the_device(planted):
    batch = planted_batch(planted)
    slots = [4, 8, 1, 4, 3, -1]  # slot 8 and -1 are out of range, the second 4 is a repeat
    rec = (BatchEstimateRecord * len(slots))()
    C.memset(rec, 0xA5, C.sizeof(rec))
    untouched = record_bytes(rec, 0)
    assert untouched == b"\xa5" * C.sizeof(BatchEstimateRecord)
    rec, times, status = batch.state_estimates(slots, rec)
    assert status.tolist() == [0, EQF_E_BAD_ARG, 0, EQF_E_BAD_ARG, 0, EQF_E_BAD_ARG]
    for e in (1, 3, 5):
        assert record_bytes(rec, e) == untouched
    worst = max(check_record(rec[e], batch.slot(slots[e]), planted[slots[e]]["orc"], show=f"entry {e}") for e in (0, 2, 4))
    assert worst <= TOL, worst
    # count == 0 on a valid batch
    assert batch.lib.eqvio_batch_estimates(batch.h, 0, (C.c_int * 1)(), rec, None, (C.c_int * 1)()) == 0
    assert batch.lib.eqvio_batch_estimates(batch.h, 1, None, rec, None, (C.c_int * 1)()) == EQF_E_BAD_ARG


# ------------------------------------------------------------------------------------------------ the recorded replay
def prepared(world, n):
    fr = list(world.frames(n))
    return PreparedFrames(world.cam, np.array([len(f[0]) for f in fr], np.int32), np.concatenate([f[0] for f in fr]).reshape(-1), np.array([f[1] for f in fr]),
                          np.array([len(f[2]) for f in fr], np.int32), np.concatenate([f[2] for f in fr]).astype(np.int32), np.concatenate([f[3] for f in fr]))


def fmt(v):
    return "%d" % v if isinstance(v, (int, np.integer)) else "%g" % v  # a default-precision std::ostream


def expected_rows(stamp, rec):
    """the rows VIOWriter writes for one record, file by file"""
    r = rec.trimmed()
    s = r["sensor"]
    points = []
    for i, w in zip(r["ids"].tolist(), r["p_world"]):
        points += [int(i), *w]
    vals = {"IMUState.csv": [*s[10:13], *s[6:10], *s[13:16]], "camera.csv": [*s[20:23], *s[16:20]], "bias.csv": [*s[0:6]], "points.csv": points}
    return {name: ", ".join(["%.20g" % stamp] + [fmt(v) for v in row]) for name, row in vals.items()}


def test_recorded_replay(tmp_path):
    s = shipped_euroc()
    lengths = [12, 12, 9]  # slot 2's sequence ends early: it sits the last steps out and writes no row there
    B = len(lengths)
    ws = [SimWorld(seed=700 + k, num_points=400, max_features=20, trajectory="wave" if k % 2 == 0 else "hover", noise_px=2.5) for k in range(B)]
    seqs = [prepared(w, n) for w, n in zip(ws, lengths)]

    def fresh():
        b = VIOFilterBatch(s, B, 64)
        if fresh.settings:
            b.set_slot_settings(1, fresh.settings)
        for k, w in enumerate(ws):
            b.start_slot(k, w.true_state(0.0, np.zeros(0, np.int32))[0], np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        return b

    fresh.settings = shipped_euroc(measurementNoise=4.0)  # slot 1 under another tuning
    plain, recorded, looped = fresh(), fresh(), fresh()
    assert plain.run_prepared(seqs) == 12
    assert recorded.run_prepared(seqs, record_dir=str(tmp_path / "rec")) == 12
    for k in range(B):  # the recorded replay leaves the same filters, bit for bit
        for a, b in zip(eqf_arrays(plain.slot(k)), eqf_arrays(recorded.slot(k))):
            assert a.tobytes() == b.tobytes()
    rows = [{name: [] for name in FILES} for _ in range(B)]
    sizes = [set() for _ in range(B)]
    for j in range(12):
        assert looped.run_prepared(seqs, first=j, count=1) == 1
        live = [k for k in range(B) if j < lengths[k]]
        rec, times, status = looped.state_estimates(live)
        assert np.all(status == 0)
        for e, k in enumerate(live):
            assert times[e] == looped.slot(k).get_time()
            sizes[k].add(tuple(rec[e].trimmed()["ids"].tolist()))
            for name, row in expected_rows(times[e], rec[e]).items():
                rows[k][name].append(row)
    assert all(len(z) >= 3 and max(len(t) for t in z) >= 10 for z in sizes), "landmarks did not enter and leave"
    single = tmp_path / "single"  # the headers of a single filter's --output run
    out = subprocess.run([SIM, "--fastRiccati", "1", "--duration", "0.3", "--quiet", "--output", str(single)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "rec")) == [f"run_{k}" for k in range(B)]
    for k in range(B):
        assert sorted(os.listdir(tmp_path / "rec" / f"run_{k}")) == sorted(FILES)
        for name in FILES:
            lines = (tmp_path / "rec" / f"run_{k}" / name).read_text().splitlines()
            assert lines[0] == (single / name).read_text().splitlines()[0], name
            assert lines[1:] == rows[k][name], (k, name)
            assert len(lines) == lengths[k] + 1
    assert rows[0]["IMUState.csv"] != rows[1]["IMUState.csv"]
    # each call starts its files anew
    again = fresh()
    assert again.run_prepared(seqs, first=0, count=2, record_dir=str(tmp_path / "rec")) == 2
    for k in range(B):
        for name in FILES:
            assert (tmp_path / "rec" / f"run_{k}" / name).read_text().splitlines()[1:] == rows[k][name][:2]
    # an output directory that cannot be created: raised before any frame runs
    blocker = tmp_path / "file"
    blocker.write_text("x")
    stuck = fresh()
    before = [[a.tobytes() for a in eqf_arrays(stuck.slot(k))] for k in range(B)]
    with pytest.raises(Exception, match="cannot create the output directory"):
        stuck.run_prepared(seqs, record_dir=str(blocker / "sub"))
    assert before == [[a.tobytes() for a in eqf_arrays(stuck.slot(k))] for k in range(B)] and all(stuck.slot(k).get_time() == 0.0 for k in range(B))


# ------------------------------------------------------------------------------------------------ the command line
def numpy_rmse(imu_state_csv, gt_csv):
    """trajectoryPositionRMSE restated: stamps < 0 skipped, the nearest ground-truth pose (the earlier on a tie), aligned on the first kept frame"""
    est = np.loadtxt(imu_state_csv, delimiter=",", skiprows=1, ndmin=2)
    gt = np.loadtxt(gt_csv, delimiter=",", skiprows=1, ndmin=2)
    gt_t = gt[:, 0] * 1e-9
    est = est[est[:, 0] >= 0]
    conj = np.array([1, -1, -1, -1])
    A, sq, biggest = None, [], 0.0
    for row in est:
        g = gt[int(np.argmin(np.abs(gt_t - row[0])))]  # argmin returns the first of equal minima
        gq = g[4:8] / np.linalg.norm(g[4:8])
        if A is None:
            R = quat_mul(gq, row[4:8] * conj)
            A = (R, g[1:4] - quat_rot(R, row[1:4]))
        sq.append(float(np.sum((quat_rot(A[0], row[1:4]) + A[1] - g[1:4]) ** 2)))
        biggest = max(biggest, float(np.max(np.abs(g[1:4]))), float(np.max(np.abs(row[1:4]))))
    return np.sqrt(np.mean(sq)), len(sq), biggest


def test_eqvio_opt_records_and_scores(tmp_path):
    run, ds, rec = str(tmp_path / "run"), str(tmp_path / "ds"), tmp_path / "rec"
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([SIM, "--duration", "3", "--maxFeatures", "20", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    gt = ds + "/groundtruth.csv"
    out = subprocess.run([OPT, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common,
                          "--batch", "3", "--sweep", "measurementNoise=0.5,0.5,50", "--record", str(rec), "--groundtruth", gt], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    frames = int(re.search(r"and (\d+) vision measurements in 3 slots", out.stdout).group(1))
    assert frames >= 50
    assert sorted(os.listdir(rec)) == ["run_0", "run_1", "run_2"]
    for k in range(3):
        assert sorted(os.listdir(rec / f"run_{k}")) == sorted(FILES)
        for name in FILES:
            assert len((rec / f"run_{k}" / name).read_text().splitlines()) == frames + 1, (k, name)
    lines = re.findall(r"slot (\d) measurementNoise=(\S+): position RMSE (\S+) over (\d+) frames", out.stdout)
    assert [(l[0], l[1]) for l in lines] == [("0", "0.5"), ("1", "0.5"), ("2", "50")], out.stdout
    assert out.stdout.index("position RMSE") > out.stdout.rindex("log-likelihood")  # after the existing per-slot lines
    for name in FILES:
        assert (rec / "run_0" / name).read_bytes() == (rec / "run_1" / name).read_bytes()
    assert lines[0][2:] == lines[1][2:]
    assert (rec / "run_2" / "IMUState.csv").read_bytes() != (rec / "run_0" / "IMUState.csv").read_bytes() and lines[2][2] != lines[0][2]
    for k in range(3):
        ref, n, biggest = numpy_rmse(rec / f"run_{k}" / "IMUState.csv", gt)
        got = float(lines[k][2])
        print(f"slot {k}: printed RMSE {got:.9g}, from the files {ref:.9g}, over {n} frames, max |position| {biggest:.3g}")
        assert int(lines[k][3]) == n and 0 < n <= frames
        assert abs(got - ref) <= 1e-4 * (1 + biggest), (k, got, ref)
