"""Per-slot settings of the filter batch on the GPU (eqf_batch_set_slot_settings, include/eqf_batch.h): ONE step of one batch in which every slot runs its
own tuning (tests/slot_settings_cases.py; tests/test_batch_slot_settings_api.py shows on the CPU that each tuning is told apart from the batch's by far more
than the bar here), every slot against ITS OWN oracle at the project's flat 1e-9 on state and Sigma with identical ids and flag words; bit identity for slots
whose settings are the batch's; a change between two frames; NEES and augment with a slot's chart and initialPointVariance; the refusals; the filter layer on a
simulated sequence, run_sim and a self-initialising slot; `eqvio_sim --sweep`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import slot_settings_cases as ssc
from batch_scenarios import ADDED, REMOVED_OLD, REMOVED_OUTLIERS, UPDATED
from eqvio_amd.batch import BatchError, VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, Settings, SimSettings, SimulationDataServer
from oracle_binding import OracleFilter
from run_configs import parity
from util import rel_fro, teacher_force

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG, EQF_E_UNSUPPORTED = -3, -6
TOL = 1e-9


def plant(batch, k, sc):
    batch.start_slot(k, sc.state[0], np.zeros(0, np.int32), np.zeros((0, 3)), sc.t0)
    batch.slot(k).force_eqf(*sc.state, sc.Sigma)
    for u in sc.imus:
        batch.process_imu(k, u)


def one_step(base, cs, modify=True):
    """every case in its own slot of ONE batch created with the batch's settings, the slots' settings set while they are empty, ONE process_vision"""
    batch = VIOFilterBatch(base, len(cs), 64)
    for k, c in enumerate(cs):
        if modify and c.call:
            batch.set_slot_settings(k, c.settings)
    for k, c in enumerate(cs):
        plant(batch, k, c.sc)
    status = batch.process_vision([(k, c.sc.stamp, c.sc.cam, c.sc.mid, c.sc.y) for k, c in enumerate(cs)])
    return batch, status, [bs.slot_arrays(batch.slot(k)) for k in range(len(cs))], [batch.last_result(k) for k in range(len(cs))]


@pytest.fixture(scope="module")
def step():
    base, cs = ssc.cases()
    batch, status, arrays, results = one_step(base, cs)
    orcs = [ssc.oracle_frame(c.settings, c.sc) for c in cs]
    return base, cs, batch, status, arrays, results, orcs


def test_one_step_runs_every_slot_with_its_own_settings(step):
    base, cs, batch, status, arrays, results, orcs = step
    assert len([c for c in cs if not ssc.same_bytes(c.settings, base)]) >= 10
    for k, (c, orc) in enumerate(zip(cs, orcs)):
        assert status[k] == 0, (c.name, status[k])
        ids_dev, ids_orc = arrays[k][2], orc.get_eqf()[2]
        assert np.array_equal(ids_dev, ids_orc), (c.name, ids_dev, ids_orc)
        d = bs.describe(c.settings, c.sc)
        assert results[k][0] == d["flags"], (c.name, results[k][0], d["flags"])
        assert ids_dev.tolist() == d["ids_predicted"], c.name  # the discard set, the lost landmarks and the new ids, by the oracle's statistics
        e = parity(batch.slot(k), orc)
        print(f"{c.name}: N {c.sc.N} -> {len(ids_dev)}, flags {results[k][0]}, parity state {e[0]:.2e} Sigma {e[1]:.2e}")
        assert e[0] < TOL and e[1] < TOL, (c.name, e)
    by = {c.name: k for k, c in enumerate(cs)}
    for cap in ssc.CAPS:
        k = by[f"cap{cap}"]
        assert len(arrays[k][2]) == 16 - cap and bool(results[k][0] & REMOVED_OUTLIERS) == (cap > 0)
    assert len(arrays[by["thresholds"]][2]) == 16 and not results[by["thresholds"]][0] & REMOVED_OUTLIERS
    assert len(arrays[by["removeLostLandmarks"]][2]) == 12 and not results[by["removeLostLandmarks"]][0] & REMOVED_OLD
    for name in ("fixed_depth", "median_depth"):  # the depth the slot's new landmarks got, against its oracle's
        k = by[name]
        depth = ssc.new_depth(orcs[k], cs[k].sc)
        print(f"{name}: depth device {results[k][1]!r} oracle {depth!r}")
        assert results[k][0] == REMOVED_OLD | ADDED | UPDATED
        assert abs(results[k][1] - depth) <= 1e-12 * depth, (name, results[k][1], depth)
    assert results[by["fixed_depth"]][1] == 7.5
    # the new landmarks' diagonal of Sigma before the update is the slot's initialPointVariance: through the 1e-9 against its oracle above, and the chart
    assert batch.get_slot_settings(by["euclidean"]).coordinateChoice == COORD_EUCLIDEAN


def test_get_returns_what_set_stored(step):
    base, cs, batch, *_ = step
    for k, c in enumerate(cs):
        assert ssc.same_bytes(batch.get_slot_settings(k), c.settings), c.name
        assert ssc.same_bytes(batch.slot(k).get_slot_settings(), c.settings), c.name
        out = Settings()
        assert batch.elib.eqf_batch_get_slot_settings(batch.core_handle(), k, C.byref(out)) == 0
        assert ssc.same_bytes(out, c.settings), c.name


def test_slots_with_the_batch_settings_keep_their_bits(step):
    """a batch in which no slot was ever given settings, on the same frames: the slots that were never touched and the slot that was set to settings equal
    to the batch's hold the same bits as there"""
    base, cs, batch, status, arrays, results, _ = step
    _, status0, arrays0, results0 = one_step(base, cs, modify=False)
    same = [k for k, c in enumerate(cs) if ssc.same_bytes(c.settings, base)]
    assert sorted(cs[k].name for k in same) == ["equal_to_batch", "unmodified", "unmodified_b"]
    for k in same:
        assert status[k] == status0[k] and results[k] == results0[k]
        for a, b in zip(arrays[k], arrays0[k]):
            assert np.array_equal(a, b), cs[k].name
    differ = [k for k in range(len(cs)) if k not in same and not all(np.array_equal(a, b) for a, b in zip(arrays[k], arrays0[k]))]
    assert len(differ) == len(cs) - len(same)  # and every other slot shows its settings


def test_settings_changed_between_two_frames():
    base = bs.shipped_euroc()
    s2 = ssc.clone(base, measurementNoise=0.4)
    sc = bs.make(base, "two_frames", 9300, 14, sigma_edit=ssc.tracking)
    batch = VIOFilterBatch(base, 2, 64)
    plant(batch, 1, sc)
    orc = OracleFilter(base)
    orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    for u in sc.imus:
        orc.process_imu(u)
    assert batch.process_vision([(1, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    orc.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
    e = parity(batch.slot(1), orc)
    assert max(e) < TOL, e
    teacher_force(batch.slot(1), orc)
    # the change: the slot's settings, and an oracle with the new settings that takes over the old one's state
    batch.set_slot_settings(1, s2)
    orc2, other = OracleFilter(s2), OracleFilter(base)
    for o in (orc2, other):
        o.set_eqf(*orc.get_eqf(), orc.get_sigma(), time=sc.stamp)
    rng = np.random.default_rng(5)
    stamp2 = sc.stamp + bs.FRAME_DT
    imus = bs.frame_imus(rng, sc.stamp, stamp2, 2)
    y2 = sc.y + rng.normal(size=sc.y.shape) * 0.5
    for u in imus:
        batch.process_imu(1, u)
        orc2.process_imu(u)
        other.process_imu(u)
    assert batch.process_vision([(1, stamp2, sc.cam, sc.mid, y2)])[0] == 0
    orc2.process_vision(stamp2, sc.cam, sc.mid, y2)
    other.process_vision(stamp2, sc.cam, sc.mid, y2)
    e = parity(batch.slot(1), orc2)
    print(f"second frame: parity state {e[0]:.2e} Sigma {e[1]:.2e}; the old settings would be off by {rel_fro(other.get_sigma(), orc2.get_sigma()):.2e}")
    assert max(e) < TOL, e
    assert rel_fro(other.get_sigma(), orc2.get_sigma()) > 1e-6


def test_nees_and_augment_use_the_slots_own_chart_and_variance():
    from test_gpu_batch_nees import plant as plant_nees, spd, true_of

    base = bs.shipped_euroc()
    rng = np.random.default_rng(21)
    se, sv = ssc.clone(base, coordinateChoice=COORD_EUCLIDEAN), ssc.clone(base, initialPointVariance=0.37)
    batch = VIOFilterBatch(base, 3, 64)
    batch.set_slot_settings(1, se)  # empty: the chart may change
    batch.set_slot_settings(2, sv)
    entries, refs, wrong = [], [], []
    for k, s in enumerate((base, se, sv)):
        st, V, lam = plant_nees(rng, 9, s.coordinateChoice)
        S = spd(V, lam)
        batch.slot(k).force_eqf(*st, S)
        orc, o2 = OracleFilter(s), OracleFilter(base)
        orc.set_eqf(*st, S)
        o2.set_eqf(*st, S)
        tr = true_of(orc, rng)
        entries.append((k, *tr))
        refs.append(orc.compute_nees(*tr))
        wrong.append(o2.compute_nees(*tr))
    vals, status = batch.compute_nees(entries)
    assert np.all(status == 0)
    for k in range(3):
        print(f"slot {k}: NEES {vals[k]!r} oracle {refs[k]!r}")
        assert abs(vals[k] - refs[k]) <= TOL * abs(refs[k]), (k, vals[k], refs[k])
    assert abs(wrong[1] - refs[1]) > 1e-6 * abs(refs[1])  # the batch's chart gives another number
    # augment: two new landmarks per slot; Sigma's new diagonal is the slot's own initialPointVariance
    new = np.array([10 ** 5, 10 ** 5 + 1], np.int32)
    pts = rng.uniform(-1, 1, (2, 3)) * 2.0 + np.array([0, 0, 6.0])
    aug = []
    for k in range(3):
        ids = batch.slot(k).get_eqf()[2]
        aug.append((k, np.concatenate([ids, new]).astype(np.int32), new, pts))
    assert np.all(batch.augment_landmark_states(aug) == 0)
    for k, s in enumerate((base, se, sv)):
        S = batch.slot(k).get_sigma()
        assert S.shape[0] == 21 + 3 * 11
        assert np.array_equal(np.diag(S)[-6:], np.full(6, s.initialPointVariance)), (k, np.diag(S)[-6:])
        assert not np.any(S[-6:, :-6]) and not np.any(S[-6:, -6:] - np.diag(np.diag(S)[-6:]))
    assert sv.initialPointVariance != base.initialPointVariance


def test_refusals_leave_the_slot_untouched():
    base = bs.shipped_euroc()
    sc = bs.make(base, "refusal", 9400, 6)
    batch = VIOFilterBatch(base, 2, 64)
    given = ssc.clone(base, measurementNoise=0.9)
    batch.set_slot_settings(0, given)
    plant(batch, 0, sc)
    before = bs.slot_arrays(batch.slot(0))
    elib, core = batch.elib, batch.core_handle()
    refused = [(ssc.clone(base, coordinateChoice=COORD_NORMAL), 0, EQF_E_UNSUPPORTED), (ssc.clone(base, fastRiccati=0), 0, EQF_E_UNSUPPORTED),
               (ssc.clone(base, coordinateChoice=7), 0, EQF_E_BAD_ARG), (ssc.clone(base, coordinateChoice=COORD_EUCLIDEAN), 0, EQF_E_BAD_ARG),  # it holds landmarks
               (ssc.clone(base, measurementNoise=0.3), 2, EQF_E_BAD_ARG), (ssc.clone(base, measurementNoise=0.3), -1, EQF_E_BAD_ARG)]
    for s, k, code in refused:
        assert elib.eqf_batch_set_slot_settings(core, k, C.byref(s)) == code, (k, code)
        assert batch.lib.eqvio_batch_set_slot_settings(batch.h, k, C.byref(s)) == code, (k, code)
        with pytest.raises(BatchError) as ei:
            batch.set_slot_settings(k, s)
        assert ei.value.code == code
        for a, b in zip(before, bs.slot_arrays(batch.slot(0))):
            assert np.array_equal(a, b)
        for kk, want in ((0, given), (1, base)):
            assert ssc.same_bytes(batch.get_slot_settings(kk), want)
    out = Settings()
    assert elib.eqf_batch_get_slot_settings(core, 2, C.byref(out)) == EQF_E_BAD_ARG
    # ... and the slot still runs its frame with the settings it was given
    assert batch.process_vision([(0, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    e = parity(batch.slot(0), ssc.oracle_frame(given, sc))
    assert max(e) < TOL, e
    # the empty slot may change its chart
    batch.set_slot_settings(1, ssc.clone(base, coordinateChoice=COORD_EUCLIDEAN))


NOISES = (0.2, 0.5, 1.5, 4.0)


def sweep_settings():
    from test_simulator import filter_settings, make_server

    fs = filter_settings(COORD_INVDEPTH)
    srv, fs = make_server(fs, duration=2.0, maxFeatures=20, numWalls=4)
    return srv, fs, [ssc.clone(fs, measurementNoise=v) for v in NOISES]


def test_filter_layer_sweeps_one_sequence():
    """four slots, the same simulated sequence, four measurementNoise values: 30 frames, teacher forced, each slot against its own oracle"""
    srv, fs, per = sweep_settings()
    s0, ids0, p0 = srv.true_state(0.0, True)
    batch = VIOFilterBatch(fs, 4, 64)
    orcs = []
    for k, s in enumerate(per):
        batch.set_slot_settings(k, s)
        batch.start_slot(k, s0, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        orcs.append(OracleFilter(s, s0, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0))
    frames, worst = 0, 0.0
    while frames < 30:
        if srv.next_measurement_type() == srv.IMU:
            u = srv.get_imu()
            for k in range(4):
                batch.process_imu(k, u)
                orcs[k].process_imu(u)
            continue
        stamp, ids, y = srv.get_vision()
        s, tids, tp = srv.true_state(stamp, True)
        assert np.all(batch.augment_landmark_states([(k, ids, tids, tp) for k in range(4)]) == 0)
        assert np.all(batch.process_vision([(k, stamp, srv.cam, ids, y) for k in range(4)]) == 0)
        for k in range(4):
            orcs[k].augment_landmark_states(ids, s, tids, tp)
            orcs[k].process_vision(stamp, srv.cam, ids, y)
            e = parity(batch.slot(k), orcs[k])
            worst = max(worst, *e)
            assert max(e) < TOL, (frames, k, e)
            teacher_force(batch.slot(k), orcs[k])
        frames += 1
    print(f"30 frames, 4 tunings: worst parity {worst:.2e}")
    sig = [o.get_sigma() for o in orcs]
    assert all(rel_fro(sig[k], sig[k + 1]) > 1e-6 for k in range(3))


def test_run_sim_with_per_slot_settings_is_the_python_loop():
    from test_gpu_batch_nees import python_main_sim, sim_pair

    fs, ss = sim_pair(61, duration=1.5)
    per = [ssc.clone(fs, measurementNoise=v) for v in NOISES]
    runs = []
    for loop in (False, True):
        batch = VIOFilterBatch(fs, 4, 64)
        for k, s in enumerate(per):
            batch.set_slot_settings(k, s)
        sims = [SimulationDataServer(ss, fs) for _ in range(4)]  # the same seed in every slot
        runs.append(python_main_sim(batch, sims, 40) if loop else batch.run_sim(sims, 40))
    a, b = runs
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    rows = a[np.all(np.isfinite(a), axis=1)]
    assert len(rows) > 20
    assert all(np.any(rows[:, k] != rows[:, k + 1]) for k in range(3))  # four tunings, four NEES columns


def test_self_initialising_slot_uses_its_own_initial_values():
    base = bs.shipped_euroc()
    own = ssc.clone(base, initialAttitudeVariance=0.03, initialPositionVariance=0.07, initialVelocityVariance=0.11, initialCameraAttitudeVariance=0.13,
                    initialCameraPositionVariance=0.17, initialBiasOmegaVariance=0.19, initialBiasAccelVariance=0.23)
    own.cameraOffset[:] = [1.0, 0.0, 0.0, 0.0, 0.1, -0.2, 0.3]
    batch = VIOFilterBatch(base, 2, 64)
    batch.set_slot_settings(1, own)
    imu = np.array([0.5, 0.01, -0.02, 0.03, 0.3, -0.2, 9.7, 0, 0, 0, 0, 0, 0])
    for k, s in enumerate((base, own)):
        assert not batch.slot(k).is_initialised()
        batch.process_imu(k, imu)
        assert batch.slot(k).is_initialised()
        orc = OracleFilter(s)
        orc.process_imu(imu)
        xi0, Xs, ids, q0, Q = batch.slot(k).get_eqf()
        o = orc.get_eqf()
        assert np.array_equal(xi0[16:23], np.array(s.cameraOffset[:]))
        assert np.allclose(xi0, o[0], rtol=0, atol=1e-12) and np.array_equal(Xs, o[1])
        assert np.array_equal(batch.slot(k).get_sigma(), np.diag(s.initial_cov_diag(0)))
        assert np.array_equal(batch.slot(k).get_sigma(), orc.get_sigma())
    # an initialised slot keeps its state and Sigma when its settings change
    before = bs.slot_arrays(batch.slot(1))
    batch.set_slot_settings(1, ssc.clone(own, initialPositionVariance=0.5, measurementNoise=0.8))
    for a, b in zip(before, bs.slot_arrays(batch.slot(1))):
        assert np.array_equal(a, b)


def test_uninitialised_slot_is_reset_only_by_a_change_of_its_initial_values():
    """a state planted on an uninitialised, empty slot survives a call that changes filter parameters only; a call that changes an initial-value field puts
    the slot back to VIOFilter(const Settings&) of the new settings. Both layers return the one copy of the slot's settings."""
    base = bs.shipped_euroc()
    batch = VIOFilterBatch(base, 1, 64)
    xi0, Xs, _, _, _ = batch.slot(0).get_eqf()
    xi0[0:3] = [0.01, -0.02, 0.03]
    S = np.diag(np.linspace(0.5, 2.5, 21))
    batch.slot(0).force_eqf(xi0, Xs, np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 5)), S)
    planted = bs.slot_arrays(batch.slot(0))
    tuned = ssc.clone(base, measurementNoise=0.8, outlierThresholdAbs=9.0)
    batch.set_slot_settings(0, tuned)
    assert not batch.slot(0).is_initialised()
    for a, b in zip(planted, bs.slot_arrays(batch.slot(0))):
        assert np.array_equal(a, b)
    dev = Settings()
    assert batch.elib.eqf_batch_get_slot_settings(batch.core_handle(), 0, C.byref(dev)) == 0
    assert ssc.same_bytes(dev, tuned) and ssc.same_bytes(batch.get_slot_settings(0), tuned)
    own = ssc.clone(tuned, initialPositionVariance=0.07)
    batch.set_slot_settings(0, own)
    xi0r, Xsr, ids, _, _ = batch.slot(0).get_eqf()
    assert len(ids) == 0 and np.array_equal(xi0r[0:3], np.zeros(3)) and np.array_equal(xi0r[16:23], np.array(own.cameraOffset[:]))
    assert np.array_equal(batch.slot(0).get_sigma(), np.diag(own.initial_cov_diag(0)))


def test_eqvio_sim_sweep_prints_one_slot_batches():
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    common = ["--fastRiccati", "1", "--duration", "2", "--seed", "3"]
    values = ["0.05", "0.1", "0.4", "1.6"]
    out = subprocess.run([exe, "--batch", "4"] + common + ["--sweep", "measurementNoise=" + ",".join(values)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(r"run (\d+) seed (\d+) measurementNoise=(\S+): mean NEES (\S+) over (\d+) frames", out.stdout)
    assert [r[0] for r in rows] == ["0", "1", "2", "3"] and {r[1] for r in rows} == {"3"} and [r[2] for r in rows] == values
    printed = [r[3] for r in rows]
    assert len(set(printed)) == 4, printed
    for k, v in enumerate(values):  # slot k is the one-slot batch run with that value, to the printed precision
        one = subprocess.run([exe, "--batch", "1"] + common + ["--measurementNoise", v], capture_output=True, text=True, timeout=600)
        assert one.returncode == 0, one.stderr[-2000:]
        m = re.search(r"run 0 seed 3: mean NEES (\S+) over (\d+) frames", one.stdout)
        assert m and m.group(1) == printed[k] and m.group(2) == rows[k][4], (k, m and m.group(1), printed[k])
