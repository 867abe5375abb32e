"""The filter batch's packet buffers (BatchPacket, eqvio_amd/csrc/eqf_batch_host.hpp): growth past what eqf_batch_create pre-allocates, and reuse of a grown
buffer by a smaller call. One batch of 66 slots (64 frame entries are pre-allocated), 2 planted landmarks per slot, 16 IMU samples per frame (66 * 16 = 1056
observer steps; 1024 are pre-allocated). Each of step, compute_nees, consistency, estimates, augment and copy_slots is called three times: with 1 entry
(the buffer as created), with all 66 (the buffer grows) and with 1 entry again (the grown buffer, reused). What comes back for slot 0 and slot 65 is
compared with np.array_equal against the same planted frame taken through the same calls in a fresh one-slot batch: a slot's arithmetic does not depend on
the batch it is part of (test_gpu_batch_filter.py::test_slot_does_not_depend_on_its_batch), so every byte must agree."""
import numpy as np
import pytest

import batch_scenarios as bs
from eqvio_amd.batch import VIOFilterBatch

pytestmark = pytest.mark.gpu
B, LAST, K_IMU = 66, 65, 16


def plant_and_step(batch, entries):
    """entries: (slot, scenario). Every listed slot planted anew with its scenario, then ONE step over all of them; the per-entry status codes."""
    for k, sc in entries:
        batch.start_slot(k, sc.state[0], np.zeros(0, np.int32), np.zeros((0, 3)), sc.t0)
        batch.slot(k).force_eqf(*sc.state, sc.Sigma)
        for u in sc.imus:
            batch.process_imu(k, u)
    return batch.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k, sc in entries])


def after_step(batch, k):
    return bs.slot_arrays(batch.slot(k)) + (np.array(batch.last_result(k)), np.array(batch.last_innovation(k)), np.array(batch.slot(k).get_time()))


def same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True), (what, i)


def same_record(a, b, what):
    assert a.keys() == b.keys(), what
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


def augment_entry(batch, k, r):
    """round r's augmentLandmarkStates of slot k: its first landmark leaves, one new id comes with a provided point"""
    ids = batch.slot(k).get_eqf()[2]
    assert len(ids) == 2
    return (k, [int(ids[-1]), 500 + r], [500 + r], np.array([[0.3 * r, -0.2, 4.0 + r]]))


def test_packets_grow_and_are_reused():
    s = bs.shipped_euroc()
    scs = [bs.make(s, f"packet{k}", 9000 + k, 2, k=K_IMU) for k in range(B)]
    assert all(len(sc.imus) == K_IMU and sc.N == 2 for sc in scs)
    big = VIOFilterBatch(s, B, 64)
    ref = {k: VIOFilterBatch(s, 1, 64) for k in (0, LAST)}  # the same frame, alone in a fresh batch
    everyone = list(range(B))

    # ---- step
    want = {}
    for k in ref:
        assert plant_and_step(ref[k], [(0, scs[k])])[0] == 0
        want[k] = after_step(ref[k], 0)
        assert len(want[k][2]) == 2
    for slots in ([0], everyone, [LAST]):
        assert np.all(plant_and_step(big, [(k, scs[k]) for k in slots]) == 0)
        for k in ref:
            if k in slots:
                same(after_step(big, k), want[k], ("step", len(slots), k))

    # ---- compute_nees, consistency: every slot against a true state near its own estimate
    rng = np.random.default_rng(11)
    truth = {k: bs.true_of(big.slot(k), rng) for k in everyone}
    nees_ref, cons_ref = {}, {}
    for k in ref:
        nees_ref[k] = ref[k].slot(0).compute_nees(*truth[k])
        cons_ref[k] = ref[k].slot(0).consistency(*truth[k])
        assert np.isfinite(nees_ref[k])
    for slots in ([0], everyone, [LAST]):
        entries = [(k, *truth[k]) for k in slots]
        vals, st = big.compute_nees(entries)
        assert np.all(st == 0)
        recs, st = big.consistency(entries)
        assert np.all(st == 0)
        for k in ref:
            if k in slots:
                assert vals[slots.index(k)] == nees_ref[k], ("nees", len(slots), k)
                same_record(recs[slots.index(k)], cons_ref[k], ("consistency", len(slots), k))

    # ---- estimates
    est_ref = {}
    for k in ref:
        rec, times, st = ref[k].state_estimates([0])
        assert st[0] == 0
        est_ref[k] = (rec[0].trimmed(), times[0])
    for slots in ([0], everyone, [LAST]):
        rec, times, st = big.state_estimates(slots)
        assert np.all(st == 0)
        for k in ref:
            if k in slots:
                same_record(rec[slots.index(k)].trimmed(), est_ref[k][0], ("estimates", len(slots), k))
                assert times[slots.index(k)] == est_ref[k][1]

    # ---- augment: round r changes every listed slot, so the one-slot batches take the rounds their slot is part of
    for r, slots in enumerate(([0], everyone, [LAST])):
        assert np.all(big.augment_landmark_states([augment_entry(big, k, r) for k in slots]) == 0)
        for k in ref:
            if k in slots:
                assert ref[k].augment_landmark_states([augment_entry(ref[k], 0, r)])[0] == 0
                same(bs.slot_arrays(big.slot(k)), bs.slot_arrays(ref[k].slot(0)), ("augment", len(slots), k))

    # ---- copy_slots: one pair, the reversal of all 66 slots (0 <-> 65 among them), one pair
    held = {k: bs.slot_arrays(ref[k].slot(0)) for k in ref}
    assert big.copy_slots([(0, 1)]) == [0]
    same(bs.slot_arrays(big.slot(1)), held[0], ("copy", 1, 0))
    assert big.copy_slots([(k, LAST - k) for k in everyone]) == [0] * B
    same(bs.slot_arrays(big.slot(LAST)), held[0], ("copy", B, 0))
    same(bs.slot_arrays(big.slot(0)), held[LAST], ("copy", B, LAST))
    same(bs.slot_arrays(big.slot(LAST - 1)), held[0], ("copy", B, 1))
    assert big.copy_slots([(0, LAST)]) == [0]
    same(bs.slot_arrays(big.slot(LAST)), held[LAST], ("copy", 1, LAST))
