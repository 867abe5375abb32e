"""The filter batch's discrete-state-matrix mode on the GPU (eqf_batch_step_discrete: k_batch_discrete in front of k_batch_frame_tail, eqvio_amd/csrc/
eqf_batch.hpp; eqvio_batch_set_slot_state_matrix; `--batchRiccati discrete`): the per-sample propagation alone and whole frames against the CPU oracle with
fastRiccati = 0 and useDiscreteStateMatrix = 1, on the planted cases of tests/riccati_cases.py (tests/test_batch_discrete_cases.py shows on the CPU that they
serve) and on simulated sequences, teacher forced; the three modes in one batch; placement; refusals; a context against a slot; the tool.

The bounds are the project's own for this mode (discrete_cases.TOL_SHORT / TOL_FRAME): 5e-9 relative in Sigma for a propagation of at most two samples, 1e-8 for
state and Sigma of a ten-sample walk or a whole frame, teacher forced - A_d is a central difference with h = 6e-6 in the reference itself. Landmark ids, flags
and outlier decisions are identical everywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import discrete_cases as dc
import riccati_cases as rc
from batch_scenarios import ADDED, EMPTY, EQF_E_CAPACITY, EQF_E_NOT_SPD, REMOVED_OLD, REMOVED_OUTLIERS, UPDATED
from eqvio_amd.batch import RICCATI_ACCURATE, RICCATI_FAST, STATE_MATRIX_CONTINUOUS, STATE_MATRIX_DISCRETE, BatchCore, VIOFilterBatch
from eqvio_amd.capi import EqfCore
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from run_configs import parity
from util import CHARTS as CHART_IDS
from util import imu_selection, rel_fro, teacher_force

pytestmark = pytest.mark.gpu
EQF_E_BAD_ARG = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARTS = ["euclid", "invdepth"]
NONE = np.zeros(0, np.int32)


def discrete_batch(s, slots, cap=64):
    batch = VIOFilterBatch(s, slots, cap)
    batch.set_slot_riccati(None, RICCATI_ACCURATE)
    batch.set_slot_state_matrix(None, STATE_MATRIX_DISCRETE)
    return batch


def set_mode(batch, k, word):
    batch.set_slot_riccati(k, RICCATI_FAST if word == "fast" else RICCATI_ACCURATE)
    batch.set_slot_state_matrix(k, STATE_MATRIX_DISCRETE if word == "discrete" else STATE_MATRIX_CONTINUOUS)


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
    """the case as a device-level frame (BatchCore.step / step_accurate / step_discrete)"""
    sel, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
    return (k, sc.cam, sc.imus, sel if dts is None else dts, sc.mid, sc.y, mean, total)


# ------------------------------------------------------------------------------------------------ 1. the propagation alone
@pytest.mark.parametrize("chart", CHARTS)
def test_propagation_alone(chart):
    """every planted case as a frame with an empty measurement and removeLostLandmarks = 0: the frame is integrateUpToTime and nothing else"""
    s, _, cases = rc.cases(chart, removeLostLandmarks=0)
    sd = dc.oracle_settings(s)
    batch = discrete_batch(s, len(cases))
    res = bs.run(batch, sd, [rc.propagation_only(sc) for sc in cases])
    worst = {dc.TOL_SHORT: 0.0, dc.TOL_FRAME: 0.0}
    for k, (sc, r) in enumerate(zip(cases, res)):
        assert r.status == 0 and r.flags == EMPTY, (sc.name, r.status, r.flags)
        assert np.array_equal(r.ids_dev, sc.state[2])
        S = r.eqf[5]
        sym = np.max(np.abs(S - S.T)) / np.max(np.abs(S))
        walked = dc.walk(sd, sc)  # the oracle of the sample-by-sample walk is the same filter
        dw = rel_fro(S, walked.get_sigma())
        tol = dc.tol(sc)
        print(f"{sc.name}: parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e} (walk {dw:.2e}; bound {tol:.0e}), asymmetry {sym:.1e}, last_riccati {batch.last_riccati(k)}")
        assert r.parity[0] < tol and r.parity[1] < tol and dw < tol, (sc.name, r.parity, dw)
        assert sym <= 1e-13, (sc.name, sym)
        assert batch.last_riccati(k) == (rc.expected_samples(sc), 0), (sc.name, batch.last_riccati(k))
        worst[tol] = max(worst[tol], r.parity[1])
    print(f"{chart}: largest Sigma error of the propagation alone: at most two samples {worst[dc.TOL_SHORT]:.2e}, beyond {worst[dc.TOL_FRAME]:.2e}")


# ------------------------------------------------------------------------------------------------ 2. whole frames
@pytest.mark.parametrize("chart", CHARTS)
def test_planted_whole_frames(chart):
    s, _, cases = rc.cases(chart)
    sd = dc.oracle_settings(s)
    batch = discrete_batch(s, len(cases))
    res = bs.run(batch, sd, cases)
    for k, (sc, r) in enumerate(zip(cases, res)):
        d = bs.describe(sd, sc)
        assert r.status == 0, (sc.name, r.status)
        assert np.array_equal(r.ids_dev, r.ids_orc), (sc.name, r.ids_dev, r.ids_orc)
        print(f"{sc.name}: N {sc.N} -> {len(r.ids_dev)}, flags {r.flags}, parity state {r.parity[0]:.2e} Sigma {r.parity[1]:.2e}")
        assert r.flags == d["flags"], (sc.name, r.flags, d["flags"])
        assert r.parity[0] < dc.TOL_FRAME and r.parity[1] < dc.TOL_FRAME, (sc.name, r.parity)
        assert batch.last_riccati(k) == (rc.expected_samples(sc), 0)
    by = {sc.name.split("_", 1)[1]: r for sc, r in zip(cases, res)}
    assert by["turnover"].flags == REMOVED_OLD | ADDED | UPDATED and by["outliers"].flags == REMOVED_OUTLIERS | UPDATED and by["n0_k1"].flags == EMPTY


# ------------------------------------------------------------------------------------------------ 3. all samples at dt = 0
@pytest.mark.parametrize("remove_lost", [0, 1])
def test_all_samples_at_dt_zero(remove_lost):
    s, _, cases = rc.cases("euclid", removeLostLandmarks=remove_lost)
    sd = dc.oracle_settings(s)
    sc = rc.propagation_only(next(c for c in cases if c.name.endswith("zero_dt_mid")))
    batch = VIOFilterBatch(s, 1, 64)
    plant(batch, 0, sc)
    core = BatchCore.of(batch)
    before = batch.slot(0).get_sigma()
    assert core.step_discrete([device_entry(0, sc, np.zeros(len(sc.imus)))])[0] == 0
    after = batch.slot(0).get_sigma()
    n = 21 if remove_lost else 21 + 3 * sc.N  # an empty measurement: removeOldLandmarks takes every landmark, or none
    assert after.shape == (n, n) and after.tobytes() == np.asfortranarray(before[:n, :n]).tobytes()
    assert core.last_riccati(0) == (0, 0)
    assert core.last_result(0)[0] == (EMPTY | (REMOVED_OLD if remove_lost else 0))
    # the observer steps still ran (dt = 0: the identity on X, the landmarks' Q re-normalised at most)
    orc = OracleFilter(sd)
    orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    for u in sc.imus:
        orc.integrate_observer(u, 0.0, bool(s.useDiscreteVelocityLift))
    if not remove_lost:
        assert parity(batch.slot(0), orc)[0] < 1e-9


# ------------------------------------------------------------------------------------------------ 4. simulated sequences
def expected_flags(before, mid, after, remove_lost, flags):
    """the oracle's bookkeeping of one frame as the bits it decides"""
    before, mid, after = set(before.tolist()), set(mid.tolist()), set(after.tolist())
    assert bool(flags & REMOVED_OLD) == bool(remove_lost and before - mid)
    assert bool(flags & ADDED) == bool(mid - before)
    assert bool(flags & UPDATED) != bool(flags & EMPTY)


@pytest.mark.parametrize("config", ["shipped_euroc", "reference_defaults"])
def test_simulated_sequences_teacher_forced(config):
    """four slots on four short simulated sequences, starting without landmarks, every slot against its own OracleFilter(fastRiccati = 0, useDiscreteStateMatrix = 1)"""
    s = getattr(bs, config)()
    sd = dc.oracle_settings(s)
    B, F = 4, 30
    ws = [SimWorld(seed=600 + k, num_points=1500, max_features=20, trajectory=("wave" if k % 2 == 0 else "hover"), noise_px=2.5) for k in range(B)]
    batch = discrete_batch(s, B)
    orcs = {}
    for k, w in enumerate(ws):
        sensor = w.true_state(0.0, NONE)[0]
        batch.start_slot(k, sensor, NONE, np.zeros((0, 3)), 0.0)
        orcs[k] = OracleFilter(sd, sensor, NONE, np.zeros((0, 3)), 0.0)
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
            n, sq = batch.last_riccati(k)
            assert 1 <= n <= len(imus) + 1 and sq == 0  # (the buffer keeps the last sample before the frame's start)
            teacher_force(batch.slot(k), orcs[k])
    print(f"{config}: worst parity state {worst[0]:.2e} Sigma {worst[1]:.2e}, flags seen {seen}")
    assert worst[0] < dc.TOL_FRAME and worst[1] < dc.TOL_FRAME, worst
    assert seen & UPDATED and seen & ADDED and seen & REMOVED_OLD


# ------------------------------------------------------------------------------------------------ 5. the three modes in one batch
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


def test_three_modes_in_one_batch():
    s = bs.shipped_euroc()
    worlds = lambda: [SimWorld(seed=700 + k, num_points=1500, max_features=20, noise_px=1.0) for k in range(6)]  # noqa: E731 - a world draws its noise as it goes
    words = ["fast", "fast", "accurate", "accurate", "discrete", "discrete"]
    mixed = VIOFilterBatch(s, 6, 64)
    for k, w in enumerate(words):
        set_mode(mixed, k, w)
    assert [mixed.slot(k).riccati for k in range(6)] == [0, 0, 1, 1, 1, 1] and [mixed.slot(k).state_matrix for k in range(6)] == [0, 0, 0, 0, 1, 1]
    free_run(mixed, worlds(), range(6), 8)
    plain = VIOFilterBatch(s, 4, 64)  # never sees a discrete call
    for k in (2, 3):
        plain.set_slot_riccati(k, RICCATI_ACCURATE)
    free_run(plain, worlds(), range(4), 8)
    for k in range(4):
        assert same_bytes(arrays(mixed.slot(k)), arrays(plain.slot(k))), k
    assert [mixed.last_riccati(k)[0] > 0 for k in range(6)] == [False, False, True, True, True, True]
    # a fast slot ignores the state-matrix choice: slot 0 of a batch whose slots are all marked discrete but stay fast
    ignored = VIOFilterBatch(s, 1, 64)
    ignored.set_slot_state_matrix(None, STATE_MATRIX_DISCRETE)
    free_run(ignored, worlds(), [0], 8)
    assert same_bytes(arrays(ignored.slot(0)), arrays(plain.slot(0))) and ignored.last_riccati(0) == (0, 0)
    # the discrete slots are not the accurate ones run again: another seed each, so compare a discrete run of seed 702 against the accurate slot 2
    again = VIOFilterBatch(s, 3, 64)
    set_mode(again, 2, "discrete")
    free_run(again, worlds(), [2], 8)
    assert not np.array_equal(again.slot(2).get_sigma()[:21, :21], plain.slot(2).get_sigma()[:21, :21])
    # copy_slots leaves the destination's two choices alone
    assert mixed.copy_slots([(0, 5)]) == [0]
    assert (mixed.slot(5).riccati, mixed.slot(5).state_matrix) == (RICCATI_ACCURATE, STATE_MATRIX_DISCRETE) and mixed.last_riccati(5) == (0, 0)

    # a slot that alternates the three modes frame by frame, against an oracle doing the same; each frame planted from the oracle's state before it
    settings_of = {"fast": s, "accurate": rc.oracle_settings(s), "discrete": dc.oracle_settings(s)}
    batch = VIOFilterBatch(s, 2, 64)
    w = worlds()[0]
    orc = OracleFilter(settings_of["discrete"], w.true_state(0.0, NONE)[0], NONE, np.zeros((0, 3)), 0.0)
    t, worst = 0.0, [0.0, 0.0]
    for j, (imus, stamp, mid, y) in enumerate(w.frames(12)):
        word = ("fast", "accurate", "discrete")[j % 3]
        sc = bs.Scenario(f"frame{j}", orc.get_eqf(), orc.get_sigma(), w.cam, t, stamp, np.array(imus), np.asarray(mid, np.int32), np.asarray(y, float))
        set_mode(batch, 1, word)
        r = bs.run(batch, settings_of[word], [sc], slots=[1])[0]
        assert r.status == 0 and np.array_equal(r.ids_dev, r.ids_orc)
        assert (batch.last_riccati(1)[0] > 0) == (word != "fast")
        worst = [max(worst[0], r.parity[0]), max(worst[1], r.parity[1])]
        orc, t = r.orc, stamp
    print(f"alternating slot: worst parity state {worst[0]:.2e} Sigma {worst[1]:.2e}")
    assert worst[0] < dc.TOL_FRAME and worst[1] < dc.TOL_FRAME, worst


# ------------------------------------------------------------------------------------------------ 6. placement
def test_placement_beside_other_modes():
    s, _, cases = rc.cases("invdepth")
    sc = next(c for c in cases if c.name.endswith("n40_k10"))
    refs = {}
    for word in ("fast", "accurate", "discrete"):
        alone = VIOFilterBatch(s, 1, 64)
        set_mode(alone, 0, word)
        plant(alone, 0, sc)
        assert alone.process_vision([entry(0, sc)])[0] == 0
        refs[word] = arrays(alone.slot(0))
    assert not same_bytes(refs["discrete"], refs["accurate"]) and not same_bytes(refs["discrete"], refs["fast"])
    big = VIOFilterBatch(s, 70, 64)
    # discrete packets of 1 and 66 entries: the packets grow behind the first call
    for listed in ([5], list(range(66))):
        for k in listed:
            set_mode(big, k, "discrete")
            plant(big, k, sc)
        assert np.all(big.process_vision([entry(k, sc) for k in listed]) == 0)
        for k in (listed[0], listed[len(listed) // 2], listed[-1]):
            assert same_bytes(arrays(big.slot(k)), refs["discrete"]), (len(listed), k)
    # slot 5 discrete beside fast and accurate neighbours, one step of three device calls
    word_of = lambda k: "discrete" if k == 5 else "accurate" if k % 2 else "fast"  # noqa: E731
    for k in range(70):
        set_mode(big, k, word_of(k))
        plant(big, k, sc)
    assert np.all(big.process_vision([entry(k, sc) for k in range(70)]) == 0)
    for k in (0, 4, 5, 6, 7, 68, 69):
        assert same_bytes(arrays(big.slot(k)), refs[word_of(k)]), k
    assert big.last_riccati(5) == (10, 0) and big.last_riccati(4) == (0, 0) and big.last_riccati(7)[0] == 10


# ------------------------------------------------------------------------------------------------ 7. refusals and neighbours
def test_refusals_and_neighbours():
    s, _, cases = rc.cases("invdepth")
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
        assert core.step_discrete([device_entry(0, small, d)])[0] == EQF_E_BAD_ARG
    # a repeated slot (the first entry is done), a frame past capacity; slot 3 is not listed
    st = core.step_discrete([device_entry(1, small), device_entry(1, small), device_entry(2, over), device_entry(0, small, bad[0])])
    assert st.tolist() == [0, EQF_E_BAD_ARG, EQF_E_CAPACITY, EQF_E_BAD_ARG]
    for k in (0, 2, 3):
        assert same_bytes(arrays(batch.slot(k)), before[k]), k
        assert core.last_riccati(k) == (0, 0)
    assert not same_bytes(arrays(batch.slot(1)), before[1]) and core.last_riccati(1) == (3, 0)
    # null imu13_mean and dt_total = 0 are accepted: the same bytes as with them
    again = VIOFilterBatch(s, 1, 40)
    plant(again, 0, small)
    assert BatchCore.of(again).step_discrete([device_entry(0, small)[:6]])[0] == 0
    assert same_bytes(arrays(again.slot(0)), arrays(batch.slot(1)))
    # eqf_batch_step on the same slot afterwards: the counters read 0 again
    plant(batch, 1, small)
    assert core.step([device_entry(1, small)])[0] == 0 and core.last_riccati(1) == (0, 0)

    # EQF_E_NOT_SPD: the walk's propagation and the bookkeeping without the update, beside a good neighbour
    s2 = bs.shipped_euroc(outlierThresholdAbs=1e8, outlierThresholdProb=1e8)
    sd2 = dc.oracle_settings(s2)
    good = rc.make(s2, "good", 901, 40, *rc.evenly(2))
    broken = rc.make(s2, "not_spd", 902, 40, *rc.evenly(2))
    bs.plant_not_spd(broken.Sigma)
    broken.oracle = "none"
    b2 = discrete_batch(s2, 2)
    res = bs.run(b2, sd2, [good, broken])
    assert res[0].status == 0 and res[0].flags == UPDATED and max(res[0].parity) < dc.TOL_FRAME
    assert res[1].status == EQF_E_NOT_SPD and res[1].flags == 0
    walked = dc.walk(sd2, broken)  # every landmark is measured and none is new: the frame without its update is the walk
    e = parity(b2.slot(1), walked)
    print(f"not_spd: propagation without the update, parity state {e[0]:.2e} Sigma {e[1]:.2e}")
    assert max(e) < dc.TOL_SHORT, e


# ------------------------------------------------------------------------------------------------ 8. a context against a slot
@pytest.mark.parametrize("chart", CHARTS)
def test_context_against_slot(chart):
    """A context loaded into a slot (eqf_batch_load_ctx), then the same samples through eqf_integrate_riccati_discrete + the observer step on the context and
    through step_discrete (propagation only) on the slot: two device implementations of the mode, no oracle between them. Same bounds."""
    s, _, cases = rc.cases(chart, removeLostLandmarks=0)
    Q12, P8 = s.input_gain_diag12(), s.state_gain_diag8()
    cases = [sc for sc in cases if sc.N > 0]
    batch = VIOFilterBatch(s, len(cases), 64)
    bcore = BatchCore.of(batch)
    worst = {dc.TOL_SHORT: 0.0, dc.TOL_FRAME: 0.0}
    for k, sc in enumerate(cases):
        ctx = EqfCore(sc.N, CHART_IDS[chart])
        ctx.set_state(*sc.state)
        ctx.set_sigma(sc.Sigma)
        batch.start_slot(k, sc.state[0], NONE, np.zeros((0, 3)), sc.t0)
        assert batch.load_core(ctx, [k]) == [0]
        dts = imu_selection(sc.imus, sc.t0, sc.stamp)[0]
        for u, dt in zip(sc.imus, dts):
            if dt > 0:
                ctx.integrate_riccati_discrete(u, dt, Q12, P8)
            ctx.integrate_observer(u[None, :], np.array([dt]), bool(s.useDiscreteVelocityLift))
        assert bcore.step_discrete([device_entry(k, rc.propagation_only(sc))])[0] == 0
        assert bcore.last_riccati(k) == (rc.expected_samples(sc), 0)
        cs, ss = ctx.get_state(), bcore.get_state(k)
        assert np.array_equal(cs[2], ss[2])
        dstate = max(float(np.abs(a - b).max()) for a, b in zip((cs[1], cs[4]), (ss[1], ss[4])))
        d = rel_fro(bcore.get_sigma(k), ctx.get_sigma())
        tol = dc.tol(sc)
        print(f"{sc.name}: slot against context: Sigma {d:.2e}, X / Q {dstate:.2e} (bound {tol:.0e})")
        assert d < tol and dstate < tol, (sc.name, d, dstate)
        worst[tol] = max(worst[tol], d)
    print(f"{chart}: slot against context, largest Sigma difference: at most two samples {worst[dc.TOL_SHORT]:.2e}, beyond {worst[dc.TOL_FRAME]:.2e}")


# ------------------------------------------------------------------------------------------------ 9. the tool
def test_eqvio_sim_batch_discrete(tmp_path):
    sim = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    common = ["--duration", "0.3", "--maxFeatures", "20", "--numWalls", "4", "--coordinateChoice", "InvDepth", "--quiet"]

    def run(name, batch, words, seed):
        out = subprocess.run([sim, "--batch", str(batch), "--batchRiccati", words, "--seed", str(seed), "--record", str(tmp_path / name), *common], capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return re.findall(r"run (\d+) seed (\d+) riccati (fast|accurate|discrete): mean NEES (\S+) over (\d+) frames", out.stdout)

    two, fast, disc = run("two", 2, "fast,discrete", 3), run("fast", 1, "fast", 3), run("disc", 1, "discrete", 4)
    assert [r[:3] for r in two] == [("0", "3", "fast"), ("1", "4", "discrete")] and [r[:3] for r in fast] == [("0", "3", "fast")] and [r[:3] for r in disc] == [("0", "4", "discrete")]
    assert two[0][3:] == fast[0][3:] and two[1][3:] == disc[0][3:] and int(disc[0][4]) >= 5
    nees = lambda name, k: (tmp_path / name / f"run_{k}" / "nees.csv").read_bytes()  # noqa: E731
    assert nees("two", 0) == nees("fast", 0) and nees("two", 1) == nees("disc", 0) and len(nees("disc", 0).splitlines()) >= 6
    # the discrete run is not the accurate run of its seed
    acc = run("acc", 1, "accurate", 4)
    assert acc[0][:3] == ("0", "4", "accurate") and nees("acc", 0) != nees("disc", 0)
