"""Copying slots of the filter batch on the GPU (eqf_batch_copy_slots / k_batch_copy, eqvio_batch_copy_slots): a clone of a running slot equals it bit for bit
and stays so, and follows an oracle forced from the source; the sizes and buffer pairs at which the copy can go wrong, with stale memory of a larger state in
the destination, held through further frames and NEES; one call that swaps, cycles and fans out; the refusals; what a destination keeps; `eqvio_opt --warmup`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import slot_settings_cases as ssc
from eqvio_amd.batch import VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from run_configs import parity
from util import project, random_spd, reasonable_state, rel_fro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG = -3
TOL = 1e-9  # the project's flat parity bound


def snap(batch, k):
    """everything of slot k the API shows: xi0, X, ids, q0, Q, Sigma, time, initialised flag"""
    sl = batch.slot(k)
    return bs.slot_arrays(sl) + (np.float64(sl.get_time()), np.bool_(sl.is_initialised()))


def same(a, b):
    return len(a) == len(b) and all(np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y) for x, y in zip(a, b))


def plant(batch, k, sc):
    batch.start_slot(k, sc.state[0], np.zeros(0, np.int32), np.zeros((0, 3)), sc.t0)
    batch.slot(k).force_eqf(*sc.state, sc.Sigma)
    for u in sc.imus:
        batch.process_imu(k, u)


def no_outliers(**kw):
    return bs.shipped_euroc(outlierThresholdAbs=1e8, outlierThresholdProb=1e8, **kw)


# ------------------------------------------------------------------------------------------------ 1. clone
def test_clone_equals_its_source_and_stays_so():
    s = bs.shipped_euroc()
    B, F0, F1 = 5, 12, 5
    ws = [SimWorld(seed=100 + k, num_points=1500, max_features=40, trajectory=("wave" if k % 2 == 0 else "hover"), noise_px=2.5) for k in range(B)]
    batch = VIOFilterBatch(s, B, 64)
    for k, w in enumerate(ws):
        sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
        batch.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    frames = list(ws[0].frames(F0 + F1))

    def step(slots, fr):
        imus, stamp, mid, y = fr
        for k in slots:
            for u in imus:
                batch.process_imu(k, u)
        assert np.all(batch.process_vision([(k, stamp, ws[0].cam, mid, y) for k in slots]) == 0)

    for k in range(1, B):  # the other slots hold runs of their own, three frames long
        for imus, stamp, mid, y in ws[k].frames(3):
            for u in imus:
                batch.process_imu(k, u)
            assert batch.process_vision([(k, stamp, ws[k].cam, mid, y)])[0] == 0
    for fr in frames[:F0]:
        step([0], fr)
    before = [snap(batch, k) for k in range(B)]
    assert len(before[0][2]) > 10 and before[0][6] == pytest.approx(F0 / 20.0)
    assert batch.slot(0).copy_to([1, 3]) == [0, 0]
    after = [snap(batch, k) for k in range(B)]
    for k in (0, 2, 4):  # the source and the slots not listed: unchanged
        assert same(before[k], after[k]), k
    for k in (1, 3):
        assert same(before[0], after[k]), k
        assert not same(before[k], after[k])
    orc = OracleFilter(s)
    orc.set_eqf(*before[0][:6], time=float(before[0][6]))
    worst = 0.0
    for fr in frames[F0:]:
        step([0, 1, 3], fr)
        imus, stamp, mid, y = fr
        for u in imus:
            orc.process_imu(u)
        orc.process_vision(stamp, ws[0].cam, mid, y)
        a = snap(batch, 0)
        for k in (1, 3):
            assert same(a, snap(batch, k)), k
            assert batch.last_innovation(k) == batch.last_innovation(0) and batch.last_result(k) == batch.last_result(0)
        e = parity(batch.slot(1), orc)
        worst = max(worst, *e)
        print(f"stamp {stamp}: slot 1 against the oracle forced at the copy: state {e[0]:.2e} Sigma {e[1]:.2e}")
        assert max(e) < TOL, e
    assert batch.last_innovation(0)[0] > 0
    assert not same(snap(batch, 0), after[0])  # the five frames did move the filter


# ------------------------------------------------------------------------------------------------ 2. sizes, buffer pairs, stale memory
def prepare(batch, k, N, cur, seed):
    """slot k with N landmarks in buffer pair `cur`, BOTH of its pairs written at (about) that size: a planted frame (k_batch_frame writes both pairs), then, for
    cur = 1, one eqf_batch_augment call that changes the slot - it moves a slot to its other pair. N = 0 is planted only (pair 0).
    The pair is inferred from the code, not checked: the interface shows no `cur`. A planted frame that keeps all its N0 landmarks (asserted) leaves the slot
    in pair 0 as k_batch_frame stands; a frame that dropped a landmark would end in the other pair, and only the landmark count would show it."""
    s = batch.get_slot_settings(k)
    if N == 0:
        assert cur == 0
        rng = np.random.default_rng(seed)
        xi0, Xs, ids, q0, Q = reasonable_state(rng, 0)
        batch.start_slot(k, xi0, ids, q0, 2.0)
        batch.slot(k).force_eqf(xi0, Xs, ids, q0, Q, random_spd(rng, 21))
        return
    N0 = N if cur == 0 else (N + 1 if N < 64 else N - 1)
    sc = bs.make(s, f"prep{N0}", seed, N0)
    plant(batch, k, sc)
    assert batch.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    ids = batch.slot(k).get_eqf()[2]
    assert len(ids) == N0
    if cur == 1 and N0 > N:  # the last landmark leaves
        assert batch.augment_landmark_states([(k, ids[:N], np.zeros(0, np.int32), np.zeros((0, 3)))])[0] == 0
    elif cur == 1:  # one landmark comes
        new = np.array([int(ids.max()) + 1], np.int32)
        assert batch.augment_landmark_states([(k, np.concatenate([ids, new]), new, np.array([[0.3, -0.2, 5.0]]))])[0] == 0
    assert len(batch.slot(k).get_eqf()[2]) == N


def shared_frame(batch, slots, rng, drop, add):
    """one frame for all of `slots` (which hold the same filter): the landmarks at the state indices `drop` are not measured (they leave), `add` new ids come"""
    sl = batch.slot(slots[0])
    _, ids, p = sl.state_estimate()
    t0 = sl.get_time()
    stamp = t0 + bs.FRAME_DT
    imus = bs.frame_imus(rng, t0, stamp, 2)
    keep = [i for i in range(len(ids)) if i not in set(drop)]
    meas = {int(ids[i]): project(bs.PINHOLE, p[i:i + 1])[0] + rng.normal(size=2) * 0.5 for i in keep}
    top = int(ids.max()) + 1 if len(ids) else 1
    for j in range(add):
        meas[top + j] = np.array([rng.uniform(150, bs.PINHOLE.width - 150), rng.uniform(100, bs.PINHOLE.height - 100)])
    mid = np.array(sorted(meas), np.int32)
    y = np.array([meas[int(i)] for i in mid]).reshape(-1)
    for k in slots:
        for u in imus:
            batch.process_imu(k, u)
    st = batch.process_vision([(k, stamp, bs.PINHOLE, mid, y) for k in slots])
    assert np.all(st == 0), st


def nees_bits(batch, slots, rng):
    es, eids, ep = batch.slot(slots[0]).state_estimate()
    ts = es.copy()
    ts[0:6] += rng.normal(size=6) * 1e-3
    ts[13:16] += rng.normal(size=3) * 1e-2
    perm = rng.permutation(len(eids))
    tp = (ep * (1.0 + rng.normal(size=ep.shape) * 1e-3))[perm]
    vals, st = batch.compute_nees([(k, ts, eids[perm], tp) for k in slots])
    assert np.all(st == 0) and np.all(np.isfinite(vals)), (st, vals)
    return [np.float64(v).tobytes() for v in vals]


#            source N, destination N before, source pair, destination pair: all four pair combinations
PAIRINGS = [(0, 5, 0, 0), (1, 7, 0, 1), (64, 33, 1, 0), (3, 64, 1, 1), (64, 0, 0, 0), (3, 64, 0, 0), (64, 1, 1, 1)]


@pytest.mark.parametrize("Ns,Nd,scur,dcur", PAIRINGS)
def test_size_and_stale_memory_edges(Ns, Nd, scur, dcur):
    batch = VIOFilterBatch(no_outliers(), 2, 64)
    prepare(batch, 0, Ns, scur, 12000 + Ns)
    prepare(batch, 1, Nd, dcur, 12100 + Nd)
    src = snap(batch, 0)
    assert len(src[2]) == Ns and src[5].shape == (21 + 3 * Ns,) * 2
    assert batch.copy_slots([(0, 1)]) == [0]
    assert same(src, snap(batch, 0)) and same(src, snap(batch, 1))
    rng = np.random.default_rng(12200 + Ns)
    bits = nees_bits(batch, [0, 1], rng)
    assert bits[0] == bits[1]
    # three frames for both: up to capacity (first and last landmark leave), five leave and five come, all measured
    N = Ns
    for drop, add in (([0, N - 1] if N >= 3 else [], None), ([1, 20, 33, 50, 63], 5), ([], 0)):
        add = 64 - (N - len(drop)) if add is None else add
        shared_frame(batch, [0, 1], rng, drop, add)
        a, b = snap(batch, 0), snap(batch, 1)
        N = len(a[2])
        assert N == 64, N
        assert same(a, b)
        assert batch.last_innovation(0) == batch.last_innovation(1) and batch.last_result(0) == batch.last_result(1)
        assert batch.last_innovation(0)[0] > 0
        bits = nees_bits(batch, [0, 1], rng)
        assert bits[0] == bits[1]


# ------------------------------------------------------------------------------------------------ 3. one call, any mapping
def test_swap_cycle_and_fan_out_in_one_call():
    s = bs.shipped_euroc()
    sizes = [2, 9, 64, 17, 0, 33, 5, 40]
    batch = VIOFilterBatch(s, len(sizes), 64)
    rng = np.random.default_rng(13000)
    for k, N in enumerate(sizes):
        xi0, Xs, ids, q0, Q = reasonable_state(rng, N, id_offset=100 * k)
        batch.start_slot(k, xi0, np.zeros(0, np.int32), np.zeros((0, 3)), 1.0 + k)
        batch.slot(k).force_eqf(xi0, Xs, ids, q0, Q, random_spd(rng, 21 + 3 * N))
        if k in (1, 3, 6):  # these sit in their second buffer pair
            assert batch.augment_landmark_states([(k, ids[:-1], np.zeros(0, np.int32), np.zeros((0, 3)))])[0] == 0
    before = [snap(batch, k) for k in range(len(sizes))]
    pairs = [(0, 1), (1, 0), (2, 3), (3, 4), (4, 2), (5, 6), (5, 7)]
    assert batch.copy_slots(pairs) == [0] * len(pairs)
    after = [snap(batch, k) for k in range(len(sizes))]
    for src, dst in pairs:
        assert same(before[src], after[dst]), (src, dst)
        assert not same(before[dst], after[dst]), (src, dst)
    assert same(before[5], after[5])
    assert batch.copy_slots([(6, 6)]) == [0] and same(after[6], snap(batch, 6))  # onto itself: nothing happens


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_destination_untouched():
    base = bs.shipped_euroc()  # InvDepth
    batch = VIOFilterBatch(base, 4, 64)
    batch.set_slot_settings(1, ssc.clone(base, coordinateChoice=COORD_EUCLIDEAN))  # while it is empty
    rng = np.random.default_rng(14000)
    for k, N in enumerate((6, 4, 3, 0)):
        xi0, Xs, ids, q0, Q = reasonable_state(rng, N, id_offset=100 * k)
        batch.start_slot(k, xi0, np.zeros(0, np.int32), np.zeros((0, 3)), 1.0 + k)
        batch.slot(k).force_eqf(xi0, Xs, ids, q0, Q, random_spd(rng, 21 + 3 * N))
        batch.process_imu(k, np.array([1.0 + k, 0.01, 0.02, 0.03, 0.1, 0.2, 9.8, 0, 0, 0, 0, 0, 0]))
    before = [snap(batch, k) for k in range(4)]
    #        bad destination, bad source, valid, repeated destination, Euclidean destination of an InvDepth source with landmarks
    pairs = [(0, 9), (-1, 2), (0, 2), (3, 2), (0, 1)]
    assert batch.copy_slots(pairs) == [EQF_E_BAD_ARG, EQF_E_BAD_ARG, 0, EQF_E_BAD_ARG, EQF_E_BAD_ARG]
    after = [snap(batch, k) for k in range(4)]
    for k in (0, 1, 3):
        assert same(before[k], after[k]), k
    assert same(before[0], after[2]) and not same(before[2], after[2])
    assert batch.get_slot_settings(1).coordinateChoice == COORD_EUCLIDEAN
    # the same through the device layer alone, and its refusals of the call itself
    elib, core = batch.elib, batch.core_handle()
    src, dst, st = (C.c_int * 2)(0, 3), (C.c_int * 2)(1, 1), (C.c_int * 2)(7, 7)
    assert elib.eqf_batch_copy_slots(core, 2, src, dst, st) == 0 and list(st) == [EQF_E_BAD_ARG, 0]  # 0 -> 1 refused (chart), 3 -> 1 done: an empty source
    assert elib.eqf_batch_copy_slots(core, -1, src, dst, st) == EQF_E_BAD_ARG
    for args in ((None, dst, st), (src, None, st), (src, dst, None)):
        assert elib.eqf_batch_copy_slots(core, 2, *args) == EQF_E_BAD_ARG
    got = bs.slot_arrays(batch.slot(1))
    assert same(before[3][:6], got) and len(got[2]) == 0
    assert batch.get_slot_settings(1).coordinateChoice == COORD_EUCLIDEAN  # and into either chart
    assert batch.slot(1).get_time() == before[1][6]  # the device layer does not know the host half
    assert batch.copy_slots([(3, 1)]) == [0] and same(before[3], snap(batch, 1))


# ------------------------------------------------------------------------------------------------ 5. what a destination keeps
def test_destination_keeps_its_settings_and_totals():
    from test_gpu_batch_nees import plant as plant_nees, spd, true_of

    base = bs.shipped_euroc()
    own = ssc.clone(base, measurementNoise=0.4, outlierThresholdAbs=9.0, outlierThresholdProb=5.0)
    batch = VIOFilterBatch(base, 2, 64)
    batch.set_slot_settings(1, own)
    # a NEES of slot 1 that takes the partial-pivot fallback: its count is the slot's, not the state's
    rng = np.random.default_rng(15000)
    st, V, lam = plant_nees(rng, 20, base.coordinateChoice)
    lam[3] = -1e-9
    batch.slot(1).force_eqf(*st, spd(V, lam))
    orc = OracleFilter(base)
    orc.set_eqf(*st, spd(V, lam))
    assert batch.compute_nees([(1, *true_of(orc, rng))])[1][0] == 0 and batch.nees_lu_fallbacks(1) == 1
    first = [bs.make(base, "first_a", 15001, 14, sigma_edit=ssc.tracking), bs.make(own, "first_b", 15002, 9, sigma_edit=ssc.tracking)]
    for k, sc in enumerate(first):
        plant(batch, k, sc)
    assert np.all(batch.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k, sc in enumerate(first)]) == 0)
    totals, last = batch.innovation_totals(1), batch.last_innovation(1)
    assert totals[0] == 1 and last[0] > 0 and batch.last_result(1)[0] != 0
    src = snap(batch, 0)
    assert batch.copy_slots([(0, 1)]) == [0]
    assert same(src, snap(batch, 1))
    assert ssc.same_bytes(batch.get_slot_settings(1), own) and ssc.same_bytes(batch.get_slot_settings(0), base)
    assert batch.innovation_totals(1) == totals and batch.nees_lu_fallbacks(1) == 1
    assert batch.last_innovation(1) == (0, 0.0, 0.0) and batch.last_result(1) == (0, 0.0)
    assert batch.last_innovation(0)[0] > 0  # the source keeps its own
    # the next frame of the destination: its own settings on the source's state
    sc = first[0]
    orc, other = OracleFilter(own), OracleFilter(base)
    for o in (orc, other):
        o.set_eqf(*src[:6], time=float(src[6]))
    stamp2 = sc.stamp + bs.FRAME_DT
    imus = bs.frame_imus(rng, sc.stamp, stamp2, 2)
    y2 = sc.y + rng.normal(size=sc.y.shape) * 0.5
    for u in imus:
        batch.process_imu(1, u)
        orc.process_imu(u)
        other.process_imu(u)
    assert batch.process_vision([(1, stamp2, sc.cam, sc.mid, y2)])[0] == 0
    orc.process_vision(stamp2, sc.cam, sc.mid, y2)
    other.process_vision(stamp2, sc.cam, sc.mid, y2)
    e = parity(batch.slot(1), orc)
    # the source's settings on the same frame give another filter: other landmarks rejected (another size of Sigma), or the same ones and another Sigma
    So, Sb = orc.get_sigma(), other.get_sigma()
    off = np.inf if So.shape != Sb.shape else rel_fro(Sb, So)
    print(f"destination's next frame: parity state {e[0]:.2e} Sigma {e[1]:.2e}, n = {So.shape[0]}; the source's settings give n = {Sb.shape[0]}, Sigma off by {off:.2e}")
    assert max(e) < TOL, e
    assert off > 1e-6
    assert batch.innovation_totals(1)[0] == totals[0] + 1


# ------------------------------------------------------------------------------------------------ 6. the tool
SLOT_LINE = r"slot (\d+)(?: (\S+)=(\S+))?: (frames updated (\d+)  failed (\d+)  mean NIS/dof (\S+)  log-likelihood (\S+))"


def test_eqvio_opt_warmup_branches_identical_slots(tmp_path):
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([sim, "--duration", "2", "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    replay = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common]
    v = "1.0"  # the value the command line runs with
    sweep = ["--batch", "4", "--measurementNoise", v, "--sweep", "measurementNoise=" + ",".join([v] * 4)]
    plain = subprocess.run(replay + sweep, capture_output=True, text=True, timeout=120)
    warm = subprocess.run(replay + sweep + ["--warmup", "10"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and warm.returncode == 0, (plain.stderr[-2000:], warm.stderr[-2000:])
    total = int(re.search(r"and (\d+) vision measurements in 4 slots", warm.stdout).group(1))
    assert total == int(re.search(r"and (\d+) vision measurements in 4 slots", plain.stdout).group(1)) > 30
    m = re.search(r"warm-up: 10 frames in slot 0, then copied into 3 slots; scores over the (\d+) frames after the warm-up", warm.stdout)
    assert m and int(m.group(1)) == total - 10, warm.stdout
    assert "warm-up" not in plain.stdout
    rows, rows0 = re.findall(SLOT_LINE, warm.stdout), re.findall(SLOT_LINE, plain.stdout)
    assert [r[0] for r in rows] == ["0", "1", "2", "3"] and len(rows0) == 4, warm.stdout
    assert len({r[3] for r in rows}) == 1, rows  # four copies of one filter, one tuning: the same text
    # the frames of the warm-up are not scored: at most total - 10 updates, and the ten fewer than the run without a warm-up that updated there
    assert 20 < int(rows[0][4]) <= total - 10 and 0 < int(rows0[0][4]) - int(rows[0][4]) <= 10 and rows[0][5] == "0", (rows[0], rows0[0])
    assert rows[0][3] != rows0[0][3]


def test_eqvio_opt_warmup_in_a_batch_of_one(tmp_path):
    """B = 1 copies nothing, yet frame F is where the swept value arrives, the totals start again and the count of scored frames starts: the value differs from the
    command line's, so a run that never applied it scores like the command line's value, and a run that scored the warm-up too counts ten frames more."""
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([sim, "--duration", "2", "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    replay = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common,
              "--measurementNoise", "1.0"]

    def rows_of(args):
        o = subprocess.run(replay + args, capture_output=True, text=True, timeout=120)
        assert o.returncode == 0, o.stderr[-2000:]
        return o.stdout, re.findall(SLOT_LINE, o.stdout)

    one, r1 = rows_of(["--batch", "1", "--sweep", "measurementNoise=2.5", "--warmup", "10"])
    two, r2 = rows_of(["--batch", "2", "--sweep", "measurementNoise=1.0,2.5", "--warmup", "10"])
    base, r0 = rows_of(["--batch", "1", "--sweep", "measurementNoise=1.0", "--warmup", "10"])
    total = int(re.search(r"and (\d+) vision measurements in 1 slots", one).group(1))
    m = re.search(r"warm-up: 10 frames in slot 0, then copied into 0 slots; scores over the (\d+) frames after the warm-up", one)
    assert m and int(m.group(1)) == total - 10 > 20, one
    assert len(r1) == 1 and len(r2) == 2 and len(r0) == 1 and r1[0][1:3] == ("measurementNoise", "2.5")
    assert 20 < int(r1[0][4]) <= total - 10, r1
    # the same filter as slot 1 of the batch of two: the command line's value for ten frames, then 2.5, scored from there - and as slot 0 of it at 1.0
    assert r1[0][3] == r2[1][3], (r1, r2)
    assert r0[0][3] == r2[0][3] and r0[0][3] != r1[0][3], (r0, r2, r1)
