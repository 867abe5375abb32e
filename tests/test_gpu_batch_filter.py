"""The filter batch (include/eqvio_batch.h) on the GPU: every slot follows its own reference filter (the CPU oracle), teacher forced frame by frame; a slot's
result does not depend on the batch around it; errors stay in their slot."""
import numpy as np
import pytest

from batch_scenarios import CAMERAS, reference_defaults, shipped_euroc
from eqvio_amd.batch import VIOFilterBatch
from eqvio_amd.capi import COORD_INVDEPTH
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from run_configs import parity
from util import teacher_force

pytestmark = pytest.mark.gpu
EQF_E_NOT_SPD, EQF_E_CAPACITY = -2, -4
TOL = 1e-9


CONFIGS = {
    "shipped_euroc": (shipped_euroc, {}, "pinhole"),
    "reference_defaults": (reference_defaults, {}, "pinhole"),
    "continuous_lifts": (reference_defaults, dict(coordinateChoice=COORD_INVDEPTH, useDiscreteInnovationLift=0, useDiscreteVelocityLift=0, useEquivariantOutput=0), "pinhole"),
    "radtan": (shipped_euroc, {}, "radtan"),
    "equidistant": (shipped_euroc, {}, "equidistant"),
}


def worlds(B, cam, noise=2.5):
    return [SimWorld(seed=100 + k, num_points=1500, max_features=40, trajectory=("wave" if k % 2 == 0 else "hover"), noise_px=noise, camera=CAMERAS[cam]) for k in range(B)]


def run_lockstep(batch, slots, orcs, frame_iters, ws, check=True, force=True, statuses=None):
    """one frame of every slot per device step; compare with the oracles and teacher force"""
    worst = [0.0, 0.0]
    for frame in zip(*frame_iters):
        entries = []
        for k, (imus, stamp, mid, y) in zip(slots, frame):
            for imu in imus:
                batch.process_imu(k, imu)
                orcs[k].process_imu(imu)
            entries.append((k, stamp, ws[k].cam, mid, y))
        st = batch.process_vision(entries)
        assert np.all(st == 0), st
        for (k, stamp, cam, mid, y) in entries:
            orcs[k].process_vision(stamp, cam, mid, y)
            if check:
                e_state, e_sigma = parity(batch.slot(k), orcs[k])
                worst = [max(worst[0], e_state), max(worst[1], e_sigma)]
            if force:
                teacher_force(batch.slot(k), orcs[k])
        if statuses is not None:
            statuses.append([batch.last_result(k)[0] for k in slots])
    return worst


def start_empty(batch, orc_settings, ws):
    orcs = {}
    for k, w in enumerate(ws):
        sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
        batch.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        orcs[k] = OracleFilter(orc_settings, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    return orcs


@pytest.mark.parametrize("config", list(CONFIGS))
def test_slots_follow_their_oracles(config):
    make, kw, cam = CONFIGS[config]
    s = make(**kw)
    B, F = 8, 75
    ws = worlds(B, cam)
    batch = VIOFilterBatch(s, B, 64)
    orcs = start_empty(batch, s, ws)
    flags = []
    worst = run_lockstep(batch, list(range(B)), orcs, [w.frames(F) for w in ws], ws, statuses=flags)
    assert worst[0] < TOL and worst[1] < TOL, worst
    flags = np.array(flags)
    assert np.any(flags & 16), "no update happened"
    assert np.any(flags & 4) and np.any(flags & 1), "no landmark turnover"
    if config == "shipped_euroc":
        assert np.any(flags & 2), "no outlier was discarded"
    for k in range(B):
        assert len(batch.slot(k).state_estimate()[1]) > 10


def test_self_initialising_slots():
    s = shipped_euroc()
    B, F = 4, 40
    ws = worlds(B, "pinhole")
    batch = VIOFilterBatch(s, B, 64)
    orcs = {k: OracleFilter(s) for k in range(B)}
    for k in range(B):
        assert not batch.slot(k).is_initialised()
    worst = run_lockstep(batch, list(range(B)), orcs, [w.frames(F) for w in ws], ws)
    assert worst[0] < TOL and worst[1] < TOL, worst
    for k in range(B):
        assert batch.slot(k).is_initialised()
        assert batch.slot(k).get_time() == pytest.approx(F / 20.0)


def free_run(batch, k, w, F):
    sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
    batch.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    for imus, stamp, mid, y in w.frames(F):
        for imu in imus:
            batch.process_imu(k, imu)
        st = batch.process_vision([(k, stamp, w.cam, mid, y)])
        assert st[0] == 0
    sl = batch.slot(k)
    return sl.get_eqf(), sl.get_sigma()


def test_slot_does_not_depend_on_its_batch():
    s = shipped_euroc()
    F = 30
    (e1, S1) = free_run(VIOFilterBatch(s, 1, 64), 0, SimWorld(seed=7, num_points=1500, max_features=40, noise_px=0.5), F)
    big = VIOFilterBatch(s, 300, 64)
    # the other 299 slots run the same steps on other sequences
    ws = [SimWorld(seed=200 + k, num_points=1500, max_features=40, noise_px=0.5) for k in range(300)]
    ws[5] = SimWorld(seed=7, num_points=1500, max_features=40, noise_px=0.5)
    for k, w in enumerate(ws):
        sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
        big.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    its = [w.frames(F) for w in ws]
    for frame in zip(*its):
        entries = []
        for k, (imus, stamp, mid, y) in enumerate(frame):
            for imu in imus:
                big.process_imu(k, imu)
            entries.append((k, stamp, ws[k].cam, mid, y))
        assert np.all(big.process_vision(entries) == 0)
    e2, S2 = big.slot(5).get_eqf(), big.slot(5).get_sigma()
    for a, b in zip(e1, e2):
        assert np.array_equal(a, b)
    assert np.array_equal(S1, S2)
    # a slot left out of a step is not touched
    before = (big.slot(9).get_eqf(), big.slot(9).get_sigma())
    nxt = [next(w.frames(1, t0=F / 20.0)) for w in ws]
    entries = []
    for k in range(300):
        if k == 9:
            continue
        imus, stamp, mid, y = nxt[k]
        for imu in imus:
            big.process_imu(k, imu)
        entries.append((k, stamp, ws[k].cam, mid, y))
    assert np.all(big.process_vision(entries) == 0)
    after = (big.slot(9).get_eqf(), big.slot(9).get_sigma())
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(before[1], after[1])


def test_per_slot_errors():
    s = shipped_euroc()
    B = 3
    ws = worlds(B, "pinhole")
    batch = VIOFilterBatch(s, B, 40)
    orcs = start_empty(batch, s, ws)
    its = [w.frames(12) for w in ws]
    run_lockstep(batch, list(range(B)), orcs, [[next(it) for _ in range(8)] for it in its], ws)
    # capacity: slot 1's measurement has more features than the slot can hold -> refused, slot untouched
    before = (batch.slot(1).get_eqf(), batch.slot(1).get_sigma(), batch.slot(1).get_time())
    frame = [next(it) for it in its]
    entries = []
    for k, (imus, stamp, mid, y) in enumerate(frame):
        for imu in imus:
            batch.process_imu(k, imu)
            if k != 1:
                orcs[k].process_imu(imu)
        if k == 1:
            extra = max(1, 41 - len(mid))
            mid = np.concatenate([mid, 100000 + np.arange(extra)]).astype(np.int32)
            y = np.concatenate([np.asarray(y).ravel(), np.full(2 * extra, 300.0)])
        entries.append((k, stamp, ws[k].cam, mid, y))
    st = batch.process_vision(entries)
    assert st.tolist() == [0, EQF_E_CAPACITY, 0]
    after = (batch.slot(1).get_eqf(), batch.slot(1).get_sigma(), batch.slot(1).get_time())
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]
    for k in (0, 2):
        orcs[k].process_vision(entries[k][1], entries[k][2], entries[k][3], entries[k][4])
        e = parity(batch.slot(k), orcs[k])
        assert max(e) < TOL, e
        teacher_force(batch.slot(k), orcs[k])
    # not SPD: slot 2 forced to a Sigma whose landmark blocks are negative definite
    xi0, Xs, ids, q0, Q = batch.slot(2).get_eqf()
    S = batch.slot(2).get_sigma()
    S[21:, 21:] = -1e6 * np.eye(S.shape[0] - 21)
    batch.slot(2).force_eqf(xi0, Xs, ids, q0, Q, S)
    frame = [next(it) for it in its]
    entries = []
    for k, (imus, stamp, mid, y) in enumerate(frame):
        if k == 1:
            continue
        for imu in imus:
            batch.process_imu(k, imu)
            if k == 0:
                orcs[k].process_imu(imu)
        entries.append((k, stamp, ws[k].cam, mid, y))
    st = batch.process_vision(entries)
    assert st.tolist() == [0, EQF_E_NOT_SPD]
    orcs[0].process_vision(entries[0][1], entries[0][2], entries[0][3], entries[0][4])
    e = parity(batch.slot(0), orcs[0])
    assert max(e) < TOL, e


def test_invalid_landmark_leaves_the_slot():
    """removeInvalidLandmarks (phase 5: compaction into the other buffer pair): a landmark whose scale a is forced below 1e-8 is removed after the update, as the
    oracle removes it; the neighbouring slot is not affected, and both keep following their oracles afterwards."""
    s = shipped_euroc()
    B = 2
    ws = worlds(B, "pinhole")
    batch = VIOFilterBatch(s, B, 64)
    orcs = start_empty(batch, s, ws)
    frames = [list(w.frames(14)) for w in ws]
    run_lockstep(batch, list(range(B)), orcs, [f[:8] for f in frames], ws)
    nxt_ids = frames[0][8][2]
    xi0, Xs, ids, q0, Q = orcs[0].get_eqf()
    victim = [i for i, lid in enumerate(ids) if lid in set(nxt_ids.tolist())][0]
    Q[victim, 4] = 5e-9
    S = orcs[0].get_sigma()
    orcs[0].set_eqf(xi0, Xs, ids, q0, Q, S, time=frames[0][7][1])
    batch.slot(0).force_eqf(xi0, Xs, ids, q0, Q, S)
    flags = []
    worst = run_lockstep(batch, list(range(B)), orcs, [f[8:9] for f in frames], ws, statuses=flags)
    assert worst[0] < TOL and worst[1] < TOL, worst
    assert flags[0][0] & 32 and not flags[0][1] & 32, flags[0]
    assert ids[victim] not in set(batch.slot(0).state_estimate()[1].tolist())
    worst = run_lockstep(batch, list(range(B)), orcs, [f[9:] for f in frames], ws)  # the id comes back as a new landmark
    assert worst[0] < TOL and worst[1] < TOL, worst
