"""NEES (eqf_batch_nees, k_batch_nees) and augmentLandmarkStates (eqf_batch_augment, k_batch_augment) of the filter batch on the GPU, against the CPU oracle
(the reference's VIO_eqf::computeNEES and VIOFilter::augmentLandmarkStates), the context path's eqf_compute_nees, and each other; run_sim (the reference's
main_sim loop in lockstep) against the same loop written over the per-call API; `eqvio_sim --batch`."""
import os
import re
import subprocess

import numpy as np
import pytest

from batch_scenarios import reference_defaults, shipped_euroc
from eqvio_amd.batch import VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, EqfCore, SimSettings, SimulationDataServer
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from run_configs import parity
from util import reasonable_state, teacher_force

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG, EQF_E_CAPACITY = -3, -4
TOL = 1e-9


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def truth_entry(k, w, t, ids=None):
    s, tids, tp = w.true_state(t)
    return (k, s, tids, tp)


def eqf_arrays(slot):
    xi0, Xs, ids, q0, Q = slot.get_eqf()
    return xi0, Xs, ids, q0, Q, slot.get_sigma()


@pytest.mark.parametrize("chart", [COORD_EUCLIDEAN, COORD_INVDEPTH])
def test_simulated_nees_follows_the_oracle(chart):
    s = shipped_euroc(coordinateChoice=chart)
    B, F = 8, 30
    ws = [SimWorld(seed=300 + k, num_points=1500, max_features=40, trajectory=("wave" if k % 2 == 0 else "hover"), noise_px=1.0) for k in range(B)]
    batch = VIOFilterBatch(s, B, 64)
    orcs = {}
    for k, w in enumerate(ws):
        sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
        batch.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        orcs[k] = OracleFilter(s, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    # N = 0 before the first frame
    vals, st = batch.compute_nees([truth_entry(k, w, 0.0) for k, w in enumerate(ws)])
    assert np.all(st == 0)
    for k, w in enumerate(ws):
        assert rel(vals[k], orcs[k].compute_nees(*truth_entry(k, w, 0.0)[1:])) <= TOL
    worst, sizes = 0.0, set()
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
            teacher_force(batch.slot(k), orcs[k])
        t = entries[0][1]
        vals, st = batch.compute_nees([truth_entry(k, w, t) for k, w in enumerate(ws)])
        assert np.all(st == 0), st
        for k, w in enumerate(ws):
            ref = orcs[k].compute_nees(*truth_entry(k, w, t)[1:])
            worst = max(worst, rel(vals[k], ref))
            sizes.add(batch.slot(k).sigma_dim())
    assert worst <= TOL, worst
    assert max(sizes) > 21 + 3 * 30


def plant(rng, N, chart, lam_lo=1e-3, lam_hi=10.0):
    n = 21 + 3 * N
    xi0, Xs, ids, q0, Q = reasonable_state(rng, N)
    V, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.exp(rng.uniform(np.log(lam_lo), np.log(lam_hi), n))
    return (xi0, Xs, ids, q0, Q), V, lam


def spd(V, lam):
    S = (V * lam) @ V.T
    return 0.5 * (S + S.T)


def true_of(orc, rng):
    es, eids, ep = orc.state_estimate()
    ts = es.copy()
    ts[0:6] += rng.normal(size=6) * 1e-3
    ts[13:16] += rng.normal(size=3) * 1e-2
    perm = rng.permutation(len(eids))  # truth ids in any order
    return ts, eids[perm], (ep + rng.normal(size=ep.shape) * 1e-2)[perm]


@pytest.mark.parametrize("chart", [COORD_EUCLIDEAN, COORD_INVDEPTH])
def test_planted_states_match_oracle_and_context(chart):
    rng = np.random.default_rng(11 + chart)
    s = reference_defaults(coordinateChoice=chart)
    Ns = [0, 1, 7, 8, 40, 64]
    batch = VIOFilterBatch(s, len(Ns), 64)
    entries, refs, ctx = [], [], []
    for k, N in enumerate(Ns):
        st, V, lam = plant(rng, N, chart)
        S = spd(V, lam)
        batch.slot(k).force_eqf(*st, S)
        orc = OracleFilter(s)
        orc.set_eqf(*st, S)
        tr = true_of(orc, rng)
        core = EqfCore(max(N, 1), chart)
        core.set_state(*st)
        core.set_sigma(S)
        entries.append((k, *tr))
        refs.append(orc.compute_nees(*tr))
        ctx.append(core.compute_nees(*tr))
    vals, status = batch.compute_nees(entries)
    assert np.all(status == 0)
    for k in range(len(Ns)):
        assert rel(vals[k], refs[k]) <= TOL, (Ns[k], vals[k], refs[k])
        assert rel(vals[k], ctx[k]) <= TOL, (Ns[k], vals[k], ctx[k])
        assert batch.nees_lu_fallbacks(k) == 0


def test_lu_fallback_in_one_slot():
    rng = np.random.default_rng(77)
    s = reference_defaults(coordinateChoice=COORD_INVDEPTH)
    B = 8
    batch = VIOFilterBatch(s, B, 64)
    entries, refs = [], []
    for k in range(B):
        st, V, lam = plant(rng, 20, COORD_INVDEPTH)
        if k == 3:
            lam[3] = -1e-9  # slightly indefinite: what rounding leaves of a zero eigenvalue
        S = spd(V, lam)
        batch.slot(k).force_eqf(*st, S)
        orc = OracleFilter(s)
        orc.set_eqf(*st, S)
        tr = true_of(orc, rng)
        entries.append((k, *tr))
        refs.append(orc.compute_nees(*tr))
    vals, status = batch.compute_nees(entries)
    assert np.all(status == 0)
    assert np.isfinite(vals[3]) and rel(vals[3], refs[3]) <= 1e-6, (vals[3], refs[3])
    assert [batch.nees_lu_fallbacks(k) for k in range(B)] == [0, 0, 0, 1, 0, 0, 0, 0]
    for k in range(B):
        if k != 3:
            assert rel(vals[k], refs[k]) <= TOL
    without, st2 = batch.compute_nees([e for e in entries if e[0] != 3])
    assert np.all(st2 == 0)
    assert np.array_equal(without, np.delete(vals, 3))


def test_nees_is_read_only():
    s = shipped_euroc()
    B, F = 4, 30
    mk = lambda: [SimWorld(seed=500 + k, num_points=1500, max_features=40, noise_px=1.0) for k in range(B)]  # noqa: E731
    runs = []
    for with_nees in (False, True):
        ws = mk()
        batch = VIOFilterBatch(s, B, 64)
        for k, w in enumerate(ws):
            sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
            batch.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        for frame in zip(*[w.frames(F) for w in ws]):
            entries = []
            for k, (imus, stamp, mid, y) in enumerate(frame):
                for imu in imus:
                    batch.process_imu(k, imu)
                entries.append((k, stamp, ws[k].cam, mid, y))
            assert np.all(batch.process_vision(entries) == 0)
            if with_nees:
                before = [eqf_arrays(batch.slot(k)) for k in range(B)]
                _, st = batch.compute_nees([truth_entry(k, w, entries[0][1]) for k, w in enumerate(ws)])
                assert np.all(st == 0)
                for k in range(B):
                    for a, b in zip(before[k], eqf_arrays(batch.slot(k))):
                        assert np.array_equal(a, b)
        runs.append([eqf_arrays(batch.slot(k)) for k in range(B)])
    for k in range(B):
        for a, b in zip(runs[0][k], runs[1][k]):
            assert np.array_equal(a, b)


def test_slot_nees_does_not_depend_on_its_batch():
    rng = np.random.default_rng(5)
    s = reference_defaults(coordinateChoice=COORD_INVDEPTH)
    st, V, lam = plant(rng, 40, COORD_INVDEPTH)
    S = spd(V, lam)
    orc = OracleFilter(s)
    orc.set_eqf(*st, S)
    tr = true_of(orc, rng)
    one = VIOFilterBatch(s, 1, 64)
    one.slot(0).force_eqf(*st, S)
    v1, _ = one.compute_nees([(0, *tr)])
    big = VIOFilterBatch(s, 300, 64)
    entries = []
    for k in range(300):
        if k == 123:
            big.slot(k).force_eqf(*st, S)
            entries.append((k, *tr))
        else:
            stk, Vk, lk = plant(rng, int(rng.integers(0, 65)), COORD_INVDEPTH)
            big.slot(k).force_eqf(*stk, spd(Vk, lk))
            o = OracleFilter(s)
            o.set_eqf(*stk, spd(Vk, lk))
            entries.append((k, *true_of(o, rng)))
    v300, status = big.compute_nees(entries)
    assert np.all(status == 0)
    assert v300[123] == v1[0]


def test_per_entry_errors():
    rng = np.random.default_rng(9)
    s = reference_defaults(coordinateChoice=COORD_EUCLIDEAN)
    B = 4
    batch = VIOFilterBatch(s, B, 64)
    entries, refs = [], []
    for k in range(B):
        st, V, lam = plant(rng, 10, COORD_EUCLIDEAN)
        batch.slot(k).force_eqf(*st, spd(V, lam))
        orc = OracleFilter(s)
        orc.set_eqf(*st, spd(V, lam))
        tr = true_of(orc, rng)
        entries.append((k, *tr))
        refs.append(orc.compute_nees(*tr))
    k, ts, tids, tp = entries[1]
    entries[1] = (k, ts, tids[1:], tp[1:])  # a filter landmark is missing from the truth
    vals, status = batch.compute_nees(entries + [entries[2], (B + 5, *entries[0][1:])])  # repeated slot, slot out of range
    assert status.tolist() == [0, EQF_E_BAD_ARG, 0, 0, EQF_E_BAD_ARG, EQF_E_BAD_ARG]
    for k in (0, 2, 3):
        assert rel(vals[k], refs[k]) <= TOL


def sim_pair(seed, max_features=30, num_points=300, duration=3.0, chart=COORD_INVDEPTH, noise=0):
    fs = shipped_euroc(coordinateChoice=chart)
    ss = SimSettings.defaults(numPoints=num_points, maxFeatures=max_features, randomSeed=seed, duration=duration, trajectory="wave", initialNoise=noise,
                              inputNoise=noise, outputNoise=noise)
    return fs, ss


def test_augment_follows_the_oracle():
    B, F = 8, 40
    fs, _ = sim_pair(0)
    sims = [SimulationDataServer(sim_pair(40 + k)[1], fs) for k in range(B)]
    batch = VIOFilterBatch(fs, B, 64)
    orcs = {}
    for k, sd in enumerate(sims):
        s0, ids0, p0 = sd.true_state(0.0, True)
        batch.start_slot(k, s0, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        orcs[k] = OracleFilter(fs, s0, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    frames, grew = 0, False
    while frames < F:
        entries, aug = [], []
        for k, sd in enumerate(sims):
            while sd.next_measurement_type() == SimulationDataServer.IMU:
                u = sd.get_imu()
                batch.process_imu(k, u)
                orcs[k].process_imu(u)
            assert sd.next_measurement_type() == SimulationDataServer.IMAGE
            stamp, ids, y = sd.get_vision()
            _, tids, tp = sd.true_state(stamp, True)
            aug.append((k, ids, tids, tp))
            entries.append((k, stamp, sd.cam, ids, y))
        assert np.all(batch.augment_landmark_states(aug) == 0)
        for k, ids, tids, tp in aug:
            orcs[k].augment_landmark_states(ids, np.zeros(23), tids, tp)
            e_state, e_sigma = parity(batch.slot(k), orcs[k])
            assert e_state <= TOL and e_sigma <= TOL, (frames, k, e_state, e_sigma)
            grew = grew or len(ids) > 0
        assert np.all(batch.process_vision(entries) == 0)
        for (k, stamp, cam, ids, y) in entries:
            orcs[k].process_vision(stamp, cam, ids, y)
            e_state, e_sigma = parity(batch.slot(k), orcs[k])
            assert e_state <= TOL and e_sigma <= TOL, (frames, k, e_state, e_sigma)
            teacher_force(batch.slot(k), orcs[k])
        frames += 1
    assert grew
    # beyond capacity: refused, the slot untouched; a new id without a provided point: refused
    small = VIOFilterBatch(fs, 2, 8)
    sd = SimulationDataServer(sim_pair(7)[1], fs)
    s0, tids, tp = sd.true_state(0.0, True)
    small.start_slot(0, s0, tids[:5], tp[:5], 0.0)
    small.start_slot(1, s0, tids[:5], tp[:5], 0.0)
    before = eqf_arrays(small.slot(0))
    st = small.augment_landmark_states([(0, tids[:9], tids, tp), (1, np.array([tids[0], 10 ** 6], np.int32), tids, tp)])
    assert st.tolist() == [EQF_E_CAPACITY, EQF_E_BAD_ARG]
    for a, b in zip(before, eqf_arrays(small.slot(0))):
        assert np.array_equal(a, b)
    assert np.array_equal(small.slot(1).get_eqf()[2], tids[:5])


def python_main_sim(batch, sims, F):
    """eqvio_batch_run_sim's loop over the per-call API"""
    B = len(sims)
    nees = np.full((F, B), np.nan)
    image = {}
    for k, sd in enumerate(sims):
        s0, tids, tp = sd.true_state(0.0, True)
        held = []
        while sd.next_measurement_type() == SimulationDataServer.IMU:
            held.append(sd.get_imu())
        image[k] = sd.get_vision() if sd.next_measurement_type() == SimulationDataServer.IMAGE else None
        keep = np.isin(tids, image[k][1]) if image[k] is not None else np.zeros(len(tids), bool)
        batch.start_slot(k, s0, tids[keep], tp[keep], 0.0)
        for u in held:
            batch.process_imu(k, u)
    for f in range(F):
        act = [k for k in range(B) if image[k] is not None]
        if not act:
            return nees[:f]
        aug = []
        for k in act:
            stamp, ids, y = image[k]
            _, tids, tp = sims[k].true_state(stamp, True)
            aug.append((k, ids, tids, tp))
        assert np.all(batch.augment_landmark_states(aug) == 0)
        assert np.all(batch.process_vision([(k, image[k][0], sims[k].cam, image[k][1], image[k][2]) for k in act]) == 0)
        ent = []
        for k in act:
            s, tids, tp = sims[k].true_state(batch.slot(k).get_time(), False)
            ent.append((k, s, tids, tp))
        v, st = batch.compute_nees(ent)
        assert np.all(st == 0)
        nees[f, act] = v
        for k in act:
            sd = sims[k]
            while sd.next_measurement_type() == SimulationDataServer.IMU:
                batch.process_imu(k, sd.get_imu())
            image[k] = sd.get_vision() if sd.next_measurement_type() == SimulationDataServer.IMAGE else None
    return nees


def test_run_sim_is_the_python_loop():
    B, F = 8, 40
    fs, _ = sim_pair(0)
    mk = lambda: [SimulationDataServer(sim_pair(60 + k, duration=1.0 + 0.5 * k)[1], fs) for k in range(B)]  # noqa: E731 - runs of different lengths
    a = VIOFilterBatch(fs, B, 64).run_sim(mk(), F)
    b = python_main_sim(VIOFilterBatch(fs, B, 64), mk(), F)
    assert a.shape == b.shape and a.shape[0] == F
    assert np.array_equal(a, b, equal_nan=True)
    assert np.isnan(a[-1, 0]) and np.all(np.isfinite(a[:10]))  # slot 0's run (1 s, 21 frames) ended first


def test_trimmed_start_matches_the_untrimmed_oracle():
    B, F = 4, 3
    fs, _ = sim_pair(0)
    vals = VIOFilterBatch(fs, B, 64).run_sim([SimulationDataServer(sim_pair(80 + k, noise=1)[1], fs) for k in range(B)], F)
    for k in range(B):
        sd = SimulationDataServer(sim_pair(80 + k, noise=1)[1], fs)
        s0, tids, tp = sd.true_state(0.0, True)
        orc = OracleFilter(fs, s0, tids, tp, 0.0)
        out = []
        while len(out) < F:
            if sd.next_measurement_type() == SimulationDataServer.IMU:
                orc.process_imu(sd.get_imu())
                continue
            stamp, ids, y = sd.get_vision()
            _, t2, p2 = sd.true_state(stamp, True)
            orc.augment_landmark_states(ids, np.zeros(23), t2, p2)
            orc.process_vision(stamp, sd.cam, ids, y)
            s, t3, p3 = sd.true_state(orc.get_time(), False)
            out.append(orc.compute_nees(s, t3, p3))
        assert out[1] > 1e-6  # noisy start and measurements: frame 1 compares a real number, not rounding
        for f in range(F):
            assert abs(vals[f, k] - out[f]) <= TOL * abs(out[f]) + 1e-24, (k, f, vals[f, k], out[f])


def test_eqvio_sim_batch_prints_run_sim_means():
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    out = subprocess.run([exe, "--batch", "4", "--fastRiccati", "1", "--duration", "2", "--seed", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    printed = [float(m) for m in re.findall(r"run \d+ seed \d+: mean NEES (\S+)", out.stdout)]
    assert len(printed) == 4
    from eqvio_amd.capi import Settings

    fs = Settings.defaults()
    fs.fastRiccati = 1
    sims = []
    for k in range(4):
        ss = SimSettings.defaults(randomSeed=3 + k, duration=2.0)
        sims.append(SimulationDataServer(ss, fs))
    fs.cameraOffset[:] = sims[0].camera_offset()
    vals = VIOFilterBatch(fs, 4, int(ss.maxFeatures)).run_sim(sims, int(np.ceil(2.0 * ss.imageFreq)) + 2)
    for k in range(4):
        col = vals[:, k]
        assert rel(printed[k], float(np.mean(col[np.isfinite(col)]))) <= 1e-8, (k, printed[k])
