"""The filter batch's accurate Riccati mode on the GPU (eqf_batch_step_accurate: k_batch_riccati in front of k_batch_frame_tail, eqvio_amd/csrc/eqf_batch.hpp;
eqvio_batch_set_slot_riccati; `--batchRiccati`): the per-sample propagation alone and whole frames against the CPU oracle with fastRiccati = 0, on the planted
cases of tests/riccati_cases.py (tests/test_batch_riccati_cases.py shows on the CPU that each is the edge it claims) and on simulated sequences, teacher forced;
both modes in one batch; placement; refusals; the filter layer and the tools. The bar is the project's flat 1e-9 relative on state and Sigma with identical
landmark ids."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import riccati_cases as rc
from batch_scenarios import ADDED, EMPTY, EQF_E_CAPACITY, EQF_E_NOT_SPD, REMOVED_INVALID, REMOVED_OLD, REMOVED_OUTLIERS, UPDATED
from eqvio_amd.batch import RICCATI_ACCURATE, RICCATI_FAST, BatchCore, VIOFilterBatch
from eqvio_amd.capi import PreparedFrames
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from run_configs import parity
from util import imu_selection, rel_fro, teacher_force

pytestmark = pytest.mark.gpu
TOL = 1e-9
EQF_E_BAD_ARG = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARTS = ["euclid", "invdepth"]
NONE = np.zeros(0, np.int32)


def plant(batch, k, sc):
    """slot k holds the case's state and Sigma and has the case's IMU samples buffered"""
    batch.start_slot(k, sc.state[0], NONE, np.zeros((0, 3)), sc.t0)
    batch.slot(k).force_eqf(*sc.state, sc.Sigma)
    for u in sc.imus:
        batch.process_imu(k, u)


def entry(k, sc):
    return (k, sc.stamp, sc.cam, sc.mid, sc.y)


def arrays(slot):
    return tuple(slot.get_eqf()) + (slot.get_sigma(),)


def same_bytes(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def device_entry(k, sc, dts=None):
    """the case as a device-level frame (BatchCore.step / step_accurate)"""
    sel, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
    return (k, sc.cam, sc.imus, sel if dts is None else dts, sc.mid, sc.y, mean, total)


# ------------------------------------------------------------------------------------------------ 1. the propagation alone
@pytest.mark.parametrize("chart", CHARTS)
def test_propagation_alone(chart):
    """every planted case as a frame with an empty measurement and removeLostLandmarks = 0: the frame is integrateUpToTime and nothing else"""
    s, so, cases = rc.cases(chart, removeLostLandmarks=0)
    batch = VIOFilterBatch(s, len(cases), 64)
    batch.set_slot_riccati(None, RICCATI_ACCURATE)
    res = bs.run(batch, so, [rc.propagation_only(sc) for sc in cases])
    worst = 0.0
    for k, (sc, r) in enumerate(zip(cases, res)):
        assert r.status == 0 and r.flags == EMPTY, (sc.name, r.status, r.flags)
        assert np.array_equal(r.ids_dev, sc.state[2])
        S = r.eqf[5]
        sym = np.max(np.abs(S - S.T)) / np.max(np.abs(S))
        samples, squarings = batch.last_riccati(k)
        print(f"{sc.name}: parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e}, asymmetry {sym:.1e}, samples {samples}, squarings {squarings}")
        assert r.parity[0] < TOL and r.parity[1] < TOL, (sc.name, r.parity)
        assert sym <= 1e-13, (sc.name, sym)
        assert samples == rc.expected_samples(sc), (sc.name, samples)
        assert (squarings >= 1) if rc.is_long(sc) else (squarings == 0), (sc.name, squarings)
        # the oracle of the sample-by-sample walk is the same filter
        walked, _ = rc.walk(so, sc)
        assert rel_fro(S, walked.get_sigma()) < TOL
        worst = max(worst, r.parity[1])
    print(f"{chart}: largest Sigma error of the propagation alone {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 2. whole frames
@pytest.mark.parametrize("chart", CHARTS)
def test_planted_whole_frames(chart):
    s, so, cases = rc.cases(chart)
    batch = VIOFilterBatch(s, len(cases), 64)
    batch.set_slot_riccati(None, RICCATI_ACCURATE)
    res = bs.run(batch, so, cases)
    for k, (sc, r) in enumerate(zip(cases, res)):
        d = bs.describe(so, sc)
        assert r.status == 0, (sc.name, r.status)
        assert np.array_equal(r.ids_dev, r.ids_orc), (sc.name, r.ids_dev, r.ids_orc)
        print(f"{sc.name}: N {sc.N} -> {len(r.ids_dev)}, flags {r.flags}, parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e}")
        assert r.flags == d["flags"], (sc.name, r.flags, d["flags"])
        assert r.parity[0] < TOL and r.parity[1] < TOL, (sc.name, r.parity)
        assert batch.last_riccati(k)[0] == rc.expected_samples(sc)
    by = {sc.name.split("_", 1)[1]: r for sc, r in zip(cases, res)}
    assert by["turnover"].flags == REMOVED_OLD | ADDED | UPDATED and by["outliers"].flags == REMOVED_OUTLIERS | UPDATED and by["n0_k1"].flags == EMPTY


def expected_flags(before, mid, after, remove_lost, flags):
    """the oracle's bookkeeping of one frame as the bits it decides"""
    before, mid, after = set(before.tolist()), set(mid.tolist()), set(after.tolist())
    assert bool(flags & REMOVED_OLD) == bool(remove_lost and before - mid)
    assert bool(flags & ADDED) == bool(mid - before)
    stayed = before & mid if remove_lost else before
    assert bool(flags & (REMOVED_OUTLIERS | REMOVED_INVALID)) == bool((stayed | mid) - after)
    assert bool(flags & UPDATED) != bool(flags & EMPTY)


@pytest.mark.parametrize("config", ["shipped_euroc", "reference_defaults"])
def test_simulated_sequences_teacher_forced(config):
    """four slots on four simulated sequences, starting without landmarks, every slot against its own OracleFilter(fastRiccati = 0)"""
    s = getattr(bs, config)()
    so = rc.oracle_settings(s)
    B, F = 4, 25
    ws = [SimWorld(seed=300 + k, num_points=1500, max_features=40, trajectory=("wave" if k % 2 == 0 else "hover"), noise_px=2.5) for k in range(B)]
    batch = VIOFilterBatch(s, B, 64)
    batch.set_slot_riccati(None, RICCATI_ACCURATE)
    orcs = {}
    for k, w in enumerate(ws):
        sensor = w.true_state(0.0, NONE)[0]
        batch.start_slot(k, sensor, NONE, np.zeros((0, 3)), 0.0)
        orcs[k] = OracleFilter(so, sensor, NONE, np.zeros((0, 3)), 0.0)
    worst, seen = [0.0, 0.0], 0
    for frame in zip(*[w.frames(F) for w in ws]):
        entries = []
        for k, (imus, stamp, mid, y) in enumerate(frame):
            for imu in imus:
                batch.process_imu(k, imu)
                orcs[k].process_imu(imu)
            entries.append((k, stamp, ws[k].cam, mid, y))
        before = [orcs[k].get_eqf()[2] for k in range(B)]
        assert np.all(batch.process_vision(entries) == 0)
        for (k, stamp, cam, mid, y) in entries:
            orcs[k].process_vision(stamp, cam, mid, y)
            e = parity(batch.slot(k), orcs[k])  # asserts identical ids
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
            flags = batch.last_result(k)[0]
            expected_flags(before[k], mid, orcs[k].get_eqf()[2], s.removeLostLandmarks, flags)
            seen |= flags
            assert 1 <= batch.last_riccati(k)[0] <= len(imus) + 1  # (the buffer keeps the last sample before the frame's start)
            teacher_force(batch.slot(k), orcs[k])
    print(f"{config}: worst parity state {worst[0]:.2e} Sigma {worst[1]:.2e}, flags seen {seen}")
    assert worst[0] < TOL and worst[1] < TOL, worst
    assert seen & UPDATED and seen & ADDED and seen & REMOVED_OLD


# ------------------------------------------------------------------------------------------------ 3. both modes in one batch
def free_run(batch, ws, slots, F):
    for k in slots:
        batch.start_slot(k, ws[k].true_state(0.0, NONE)[0], NONE, np.zeros((0, 3)), 0.0)
    for frame in zip(*[ws[k].frames(F) for k in slots]):
        entries = []
        for k, (imus, stamp, mid, y) in zip(slots, frame):
            for imu in imus:
                batch.process_imu(k, imu)
            entries.append((k, stamp, ws[k].cam, mid, y))
        assert np.all(batch.process_vision(entries) == 0)


def test_both_modes_in_one_batch():
    s = bs.shipped_euroc()
    so = rc.oracle_settings(s)
    worlds = lambda: [SimWorld(seed=400 + k, num_points=1500, max_features=40, noise_px=1.0) for k in range(4)]  # noqa: E731 - a world draws its noise as it goes
    mixed = VIOFilterBatch(s, 4, 64)
    for k in (2, 3):
        mixed.slot(k).riccati = RICCATI_ACCURATE
    assert [mixed.slot_riccati(k) for k in range(4)] == [RICCATI_FAST, RICCATI_FAST, RICCATI_ACCURATE, RICCATI_ACCURATE]
    free_run(mixed, worlds(), [0, 1, 2, 3], 10)
    fast_only = VIOFilterBatch(s, 2, 64)  # never sees an accurate call
    free_run(fast_only, worlds(), [0, 1], 10)
    for k in (0, 1):
        assert same_bytes(arrays(mixed.slot(k)), arrays(fast_only.slot(k))), k
        assert mixed.last_riccati(k) == (0, 0)
    for k in (2, 3):
        assert mixed.last_riccati(k)[0] > 0
        assert not np.array_equal(mixed.slot(k).get_sigma()[:21, :21], fast_only.slot(k - 2).get_sigma()[:21, :21])
    # a slot that alternates modes frame by frame, against an oracle doing the same; each frame planted from the oracle's state before it
    batch = VIOFilterBatch(s, 2, 64)
    w = worlds()[0]
    orc = OracleFilter(so, w.true_state(0.0, NONE)[0], NONE, np.zeros((0, 3)), 0.0)
    t, worst = 0.0, [0.0, 0.0]
    for j, (imus, stamp, mid, y) in enumerate(w.frames(10)):
        mode = RICCATI_ACCURATE if j % 2 else RICCATI_FAST
        sc = bs.Scenario(f"frame{j}", orc.get_eqf(), orc.get_sigma(), w.cam, t, stamp, np.array(imus), np.asarray(mid, np.int32), np.asarray(y, float))
        batch.set_slot_riccati(1, mode)
        r = bs.run(batch, so if mode else s, [sc], slots=[1])[0]
        assert r.status == 0 and np.array_equal(r.ids_dev, r.ids_orc)
        assert (batch.last_riccati(1)[0] > 0) == bool(mode)
        worst = [max(worst[0], r.parity[0]), max(worst[1], r.parity[1])]
        orc, t = r.orc, stamp
    print(f"alternating slot: worst parity state {worst[0]:.2e} Sigma {worst[1]:.2e}")
    assert worst[0] < TOL and worst[1] < TOL, worst


# ------------------------------------------------------------------------------------------------ 4. placement
def test_placement_and_grown_packet():
    s, so, cases = rc.cases("invdepth")
    sc = next(c for c in cases if c.name.endswith("n40_k10"))
    alone = VIOFilterBatch(s, 1, 64)
    alone.set_slot_riccati(0, RICCATI_ACCURATE)
    plant(alone, 0, sc)
    assert alone.process_vision([entry(0, sc)])[0] == 0
    ref = arrays(alone.slot(0))
    fast1 = VIOFilterBatch(s, 1, 64)
    plant(fast1, 0, sc)
    assert fast1.process_vision([entry(0, sc)])[0] == 0
    ref_fast = arrays(fast1.slot(0))
    assert not same_bytes(ref, ref_fast)
    big = VIOFilterBatch(s, 70, 64)
    # accurate packets of 1, 66 and 1 entries: the packets grow behind the first call
    for listed in ([5], list(range(66)), [69]):
        for k in listed:
            big.set_slot_riccati(k, RICCATI_ACCURATE)
            plant(big, k, sc)
        assert np.all(big.process_vision([entry(k, sc) for k in listed]) == 0)
        for k in (listed[0], listed[len(listed) // 2], listed[-1]):
            assert same_bytes(arrays(big.slot(k)), ref), (len(listed), k)
    # slot 5 accurate beside 69 fast neighbours, one step
    big.set_slot_riccati(None, RICCATI_FAST)
    big.set_slot_riccati(5, RICCATI_ACCURATE)
    for k in range(70):
        plant(big, k, sc)
    assert np.all(big.process_vision([entry(k, sc) for k in range(70)]) == 0)
    assert same_bytes(arrays(big.slot(5)), ref)
    for k in (0, 4, 6, 69):
        assert same_bytes(arrays(big.slot(k)), ref_fast), k
    assert big.last_riccati(5) == (10, 0) and big.last_riccati(4) == (0, 0)


# ------------------------------------------------------------------------------------------------ 5. refusals and neighbours
def test_refusals_and_neighbours():
    s, so, cases = rc.cases("invdepth")
    sc = next(c for c in cases if c.name.endswith("n40_k10"))
    over = rc.make(s, "over", 903, 40, *rc.evenly(2), new=1)  # 40 stay + 1 new in a batch of capacity 40
    batch = VIOFilterBatch(s, 4, 40)
    core = BatchCore.of(batch)
    plant(batch, 2, over)
    small = rc.make(s, "n20", 900, 20, *rc.evenly(3))
    for k in (0, 1, 3):
        plant(batch, k, small)
    before = [arrays(batch.slot(k)) for k in range(4)]
    dts = imu_selection(small.imus, small.t0, small.stamp)[0]
    bad = [dts.copy() for _ in range(3)]
    bad[0][1], bad[1][2], bad[2][0] = -1e-3, np.nan, np.inf
    for d in bad:
        assert core.step_accurate([device_entry(0, small, d)])[0] == EQF_E_BAD_ARG
    # a repeated slot (the first entry is done), a frame past capacity; slot 3 is not listed
    st = core.step_accurate([device_entry(1, small), device_entry(1, small), device_entry(2, over), device_entry(0, small, bad[0])])
    assert st.tolist() == [0, EQF_E_BAD_ARG, EQF_E_CAPACITY, EQF_E_BAD_ARG]
    for k in (0, 2, 3):
        assert same_bytes(arrays(batch.slot(k)), before[k]), k
        assert core.last_riccati(k) == (0, 0)
    assert not same_bytes(arrays(batch.slot(1)), before[1]) and core.last_riccati(1) == (3, 0)
    # null imu13_mean and dt_total = 0 are accepted: the same bytes as with them
    again = VIOFilterBatch(s, 1, 40)
    plant(again, 0, small)
    assert BatchCore.of(again).step_accurate([device_entry(0, small)[:6]])[0] == 0
    assert same_bytes(arrays(again.slot(0)), arrays(batch.slot(1)))
    # eqf_batch_step on the same slot afterwards: the counters read 0 again
    plant(batch, 1, small)
    assert core.step([device_entry(1, small)])[0] == 0 and core.last_riccati(1) == (0, 0)

    # EQF_E_NOT_SPD: the propagation and the bookkeeping without the update, beside a good neighbour; NEES after an accurate step
    s2 = bs.shipped_euroc(outlierThresholdAbs=1e8, outlierThresholdProb=1e8)
    so2 = rc.oracle_settings(s2)
    good = rc.make(s2, "good", 901, 40, *rc.evenly(2))
    broken = rc.make(s2, "not_spd", 902, 40, *rc.evenly(2))
    bs.plant_not_spd(broken.Sigma)
    broken.oracle = "none"
    b2 = VIOFilterBatch(s2, 2, 64)
    b2.set_slot_riccati(None, RICCATI_ACCURATE)
    res = bs.run(b2, so2, [good, broken])
    assert res[0].status == 0 and res[0].flags == UPDATED and max(res[0].parity) < TOL
    assert res[1].status == EQF_E_NOT_SPD and res[1].flags == 0
    walked, _ = rc.walk(so2, broken)  # every landmark is measured and none is new: the frame without its update is the walk
    e = parity(b2.slot(1), walked)
    print(f"not_spd: propagation without the update, parity state {e[0]:.2e} Sigma {e[1]:.2e}")
    assert max(e) < TOL, e
    rng = np.random.default_rng(5)
    truth = bs.true_of(res[0].orc, rng)
    vals, st = b2.compute_nees([(0, *truth)])
    ref = res[0].orc.compute_nees(*truth)
    assert st[0] == 0 and abs(vals[0] - ref) <= TOL * abs(ref), (vals, ref)


# ------------------------------------------------------------------------------------------------ 6. all samples at dt = 0
@pytest.mark.parametrize("remove_lost", [0, 1])
def test_all_samples_at_dt_zero(remove_lost):
    s, so, cases = rc.cases("euclid", removeLostLandmarks=remove_lost)
    sc = rc.propagation_only(next(c for c in cases if c.name.endswith("zero_dt_mid")))
    batch = VIOFilterBatch(s, 1, 64)
    plant(batch, 0, sc)
    core = BatchCore.of(batch)
    before = batch.slot(0).get_sigma()
    assert core.step_accurate([device_entry(0, sc, np.zeros(len(sc.imus)))])[0] == 0
    after = batch.slot(0).get_sigma()
    n = 21 if remove_lost else 21 + 3 * sc.N  # an empty measurement: removeOldLandmarks takes every landmark, or none
    assert after.shape == (n, n) and after.tobytes() == np.asfortranarray(before[:n, :n]).tobytes()
    assert core.last_riccati(0) == (0, 0)
    assert core.last_result(0)[0] == (EMPTY | (REMOVED_OLD if remove_lost else 0))
    # the observer steps still ran (dt = 0: the identity on X, the landmarks' Q re-normalised at most)
    orc = OracleFilter(so)
    orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    for u in sc.imus:
        orc.integrate_observer(u, 0.0, bool(s.useDiscreteVelocityLift))
    if not remove_lost:
        assert parity(batch.slot(0), orc)[0] < TOL


# ------------------------------------------------------------------------------------------------ 7. the filter layer and the tools
def prepared(world, n):
    fr = list(world.frames(n))
    return fr, PreparedFrames(world.cam, np.array([len(f[0]) for f in fr], np.int32), np.concatenate([f[0] for f in fr]).reshape(-1), np.array([f[1] for f in fr]),
                              np.array([len(f[2]) for f in fr], np.int32), np.concatenate([f[2] for f in fr]).astype(np.int32), np.concatenate([f[3] for f in fr]))


def test_run_prepared_with_slot_modes():
    s = bs.shipped_euroc()
    so = rc.oracle_settings(s)
    w = SimWorld(seed=500, num_points=1500, max_features=40, noise_px=1.0)
    F = 12
    fr, seq = prepared(w, F)
    batch = VIOFilterBatch(s, 2, 64)
    batch.set_slot_riccati(1, RICCATI_ACCURATE)
    with pytest.raises(Exception):
        batch.set_slot_riccati(0, 2)
    with pytest.raises(Exception):
        batch.set_slot_riccati(2, RICCATI_FAST)
    assert [batch.slot(k).riccati for k in range(2)] == [RICCATI_FAST, RICCATI_ACCURATE]
    sensor = w.true_state(0.0, NONE)[0]
    orcs = []
    for k, st in enumerate((s, so)):
        batch.start_slot(k, sensor, NONE, np.zeros((0, 3)), 0.0)
        orcs.append(OracleFilter(st, sensor, NONE, np.zeros((0, 3)), 0.0))
    worst = [[0.0, 0.0], [0.0, 0.0]]
    for j, (imus, stamp, mid, y) in enumerate(fr):
        assert batch.run_prepared([seq, seq], first=j, count=1) == 1
        for k, orc in enumerate(orcs):
            for imu in imus:
                orc.process_imu(imu)
            orc.process_vision(stamp, w.cam, mid, y)
            e = parity(batch.slot(k), orc)
            worst[k] = [max(worst[k][0], e[0]), max(worst[k][1], e[1])]
            teacher_force(batch.slot(k), orc)
        assert batch.last_riccati(0) == (0, 0) and 1 <= batch.last_riccati(1)[0] <= len(imus) + 1
    print(f"run_prepared: fast slot {worst[0]}, accurate slot {worst[1]}")
    assert max(worst[0]) < TOL and max(worst[1]) < TOL, worst
    # copy_slots leaves the destination's mode alone
    assert batch.copy_slots([(0, 1)]) == [0]
    assert batch.slot(1).riccati == RICCATI_ACCURATE and batch.last_riccati(1) == (0, 0)


def test_eqvio_sim_batch_riccati(tmp_path):
    sim = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    common = ["--duration", "0.3", "--maxFeatures", "40", "--numWalls", "4", "--coordinateChoice", "InvDepth", "--quiet"]
    two = subprocess.run([sim, "--batch", "2", "--batchRiccati", "fast,accurate", "--seed", "3", "--record", str(tmp_path / "two"), *common], capture_output=True, text=True,
                         timeout=120)
    assert two.returncode == 0, two.stderr[-2000:]
    one = subprocess.run([sim, "--batch", "1", "--batchRiccati", "accurate", "--seed", "4", "--record", str(tmp_path / "one"), *common], capture_output=True, text=True,
                         timeout=120)
    assert one.returncode == 0, one.stderr[-2000:]
    line = r"run (\d+) seed (\d+) riccati (fast|accurate): mean NEES (\S+) over (\d+) frames"
    rows2, rows1 = re.findall(line, two.stdout), re.findall(line, one.stdout)
    assert [r[:3] for r in rows2] == [("0", "3", "fast"), ("1", "4", "accurate")] and [r[:3] for r in rows1] == [("0", "4", "accurate")], (two.stdout, one.stdout)
    assert rows2[1][3:] == rows1[0][3:] and int(rows1[0][4]) >= 5
    a, b = (tmp_path / "two" / "run_1" / "nees.csv").read_bytes(), (tmp_path / "one" / "run_0" / "nees.csv").read_bytes()
    assert a == b and len(a.splitlines()) >= 6
    # the fast slot of the mixed run is the run the tool makes without the flag
    plain = subprocess.run([sim, "--batch", "1", "--fastRiccati", "1", "--seed", "3", "--record", str(tmp_path / "plain"), *common], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "riccati" not in plain.stdout
    assert (tmp_path / "two" / "run_0" / "nees.csv").read_bytes() == (tmp_path / "plain" / "run_0" / "nees.csv").read_bytes()
    assert (tmp_path / "two" / "run_0" / "nees.csv").read_bytes() != a
