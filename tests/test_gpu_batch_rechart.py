"""Changing a slot's chart under landmarks on the GPU (eqf_batch_convert_chart, k_batch_rechart in eqvio_amd/csrc/eqf_batch.hpp): Sigma' against numpy's
T Sigma T^T with the T of tests/rechart_cases.py (built without the product's code; tests/test_rechart_cases.py shows on the CPU what it is), the rebuilt chart
constants through a whole frame in all three step modes, the converted slot's next frame against the oracle of the new chart, the invariance of the innovation
statistics, round trips, what a conversion leaves alone, the bridge to a context, the filter level and the tool.
The bar is the project's flat 1e-9 relative (1e-8 for the discrete mode, its existing bound).

Worst deviations seen on an MI355X (profiles/r24_batch_rechart_parity.txt): Sigma' against numpy's T Sigma T^T 3.1e-16; the next frame
against the oracle of the new chart 1.1e-12 fast and accurate, 5.1e-10 discrete; NIS 2.4e-14 and log det S 7.2e-16 between the twins; round trips 1.1e-15;
NEES 5.7e-13. Every test prints its figures."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_normal_cases as bn
import batch_scenarios as bs
import discrete_cases as dc
import rechart_cases as rcs
import riccati_cases as rc
from eqvio_amd.batch import RICCATI_ACCURATE, RICCATI_FAST, STATE_MATRIX_CONTINUOUS, STATE_MATRIX_DISCRETE, BatchCore, BatchError, VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, EqfCore
from oracle_binding import OracleFilter
from run_configs import parity
from test_gpu_batch_nees import plant as plant_nees
from test_gpu_batch_nees import spd, true_of
from util import rel_fro

pytestmark = pytest.mark.gpu
TOL = 1e-9
EQF_E_BAD_ARG = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.zeros(0, np.int32)
PAIR_IDS = [rcs.pair_name(p) for p in rcs.PAIRS]
MODES = {"fast": (RICCATI_FAST, STATE_MATRIX_CONTINUOUS), "accurate": (RICCATI_ACCURATE, STATE_MATRIX_CONTINUOUS), "discrete": (RICCATI_ACCURATE, STATE_MATRIX_DISCRETE)}
MODE_TOL = {"fast": 1e-9, "accurate": 1e-9, "discrete": 1e-8}


def base_settings(**kw):
    """what the batches here are created with: the shipped EuRoC settings under the Euclidean chart (a slot gets its chart from set_slot_chart)"""
    return bs.shipped_euroc(coordinateChoice=COORD_EUCLIDEAN, **kw)


def make_batch(charts, **kw):
    batch = VIOFilterBatch(base_settings(**kw), len(charts), 64)
    for k, c in enumerate(charts):
        batch.set_slot_chart(k, c)
    return batch


def set_mode(batch, k, mode):
    batch.set_slot_riccati(k, MODES[mode][0])
    batch.set_slot_state_matrix(k, MODES[mode][1])


def oracle_settings(chart, mode, **kw):
    s = bn.with_chart(base_settings(**kw), chart)
    return s if mode == "fast" else rc.oracle_settings(s) if mode == "accurate" else dc.oracle_settings(s)


def snap(batch, k):
    """everything the API shows of a slot's EqF state, as bytes"""
    return tuple(a.tobytes() for a in batch.slot(k).get_eqf()) + (batch.slot(k).get_sigma().tobytes(),)


def settings_but_chart(s):
    o = bn.with_chart(s, COORD_EUCLIDEAN)
    return bytes(o)


def bookkeeping(batch, k):
    """what a conversion must leave alone beside the state"""
    return (settings_but_chart(batch.get_slot_settings(k)), batch.slot_riccati(k), batch.slot_state_matrix(k), batch.innovation_totals(k), batch.last_result(k),
            batch.last_innovation(k), batch.nees_lu_fallbacks(k), batch.last_riccati(k), batch.slot(k).get_time(), batch.slot(k).is_initialised())


@pytest.fixture(scope="module")
def frame_case():
    """one planted frame with turnover (3 landmarks lost, 3 new) and two IMU samples at N = 21, near landmarks: tests/riccati_cases.py's generator, which every
    step mode runs at its bound"""
    return rc.make(base_settings(), "rechart_turnover", 9300, 21, *rc.evenly(2), lost=3, new=3)


def plant_frame(batch, k, sc, state=None, Sigma=None):
    batch.start_slot(k, sc.state[0], NONE, np.zeros((0, 3)), sc.t0)
    batch.slot(k).force_eqf(*(sc.state if state is None else state), sc.Sigma if Sigma is None else Sigma)


# ------------------------------------------------------------------------------------------------ 1. Sigma' = T Sigma T^T on the size grid
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_sigma_is_the_congruence(pair):
    a, b = pair
    batch = make_batch([a] * len(rcs.NS))
    before = []
    for k, N in enumerate(rcs.NS):
        state, S = rcs.case(N)
        batch.slot(k).force_eqf(*state, S)
        before.append((snap(batch, k), bookkeeping(batch, k)))
    assert batch.convert_chart([(k, b) for k in range(len(rcs.NS))]) == [0] * len(rcs.NS)
    worst = worst_part = 0.0
    for k, N in enumerate(rcs.NS):
        S1 = batch.slot(k).get_sigma()
        d = rel_fro(S1, rcs.expected(N, a, b))
        worst = max(worst, d)
        print(f"{rcs.pair_name(pair)} N {N}: Sigma' against numpy's T Sigma T^T {d:.2e}")
        assert d <= TOL, (N, d)
        if N > 0:  # under InvDepth the landmark rows are ~1e-3 of the sensor rows: each part of Sigma' on its own, so the small ones are not hidden
            E = rcs.expected(N, a, b)
            d_cross, d_lm = rel_fro(S1[21:, :21], E[21:, :21]), rel_fro(S1[21:, 21:], E[21:, 21:])
            worst_part = max(worst_part, d_cross, d_lm)
            assert d_cross <= TOL and d_lm <= TOL, (N, d_cross, d_lm)
        assert np.array_equal(S1, S1.T), N  # symmetric bit for bit
        assert snap(batch, k)[:5] == before[k][0][:5], N  # xi0, X, ids, q0, Q: bit for bit
        assert batch.slot_chart(k) == b and batch.get_slot_settings(k).coordinateChoice == b
        assert bookkeeping(batch, k) == before[k][1], N
        if COORD_NORMAL not in pair:  # the sensor block is copied bit for bit
            assert np.array_equal(S1[:21, :21], rcs.case(N)[1][:21, :21]), N
    print(f"{rcs.pair_name(pair)}: worst {worst:.2e}; sensor-landmark and landmark-landmark parts on their own {worst_part:.2e}")


# ------------------------------------------------------------------------------------------------ 2. the rebuilt chart constants: a fresh slot of the new chart
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_converted_slot_is_the_planted_one_through_a_frame(pair, frame_case):
    a, b = pair
    sc = frame_case
    for mode in MODES:
        batch = make_batch([a, b])
        for k in range(2):
            set_mode(batch, k, mode)
        plant_frame(batch, 0, sc)
        assert batch.convert_chart([(0, b)]) == [0]
        st, S1 = batch.slot(0).get_eqf(), batch.slot(0).get_sigma()
        plant_frame(batch, 1, sc, st, S1)
        assert snap(batch, 0) == snap(batch, 1)
        for u in sc.imus:
            batch.process_imu(0, u)
            batch.process_imu(1, u)
        status = batch.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k in range(2)])
        assert np.all(status == 0), status
        assert snap(batch, 0) == snap(batch, 1), (mode, "state or Sigma differ after the frame")
        assert batch.last_result(0) == batch.last_result(1) and batch.last_result(0)[0] & bs.UPDATED and batch.last_result(0)[0] & bs.ADDED
        assert batch.last_innovation(0) == batch.last_innovation(1) and batch.last_innovation(0)[0] > 0
        assert len(batch.slot(0).get_eqf()[2]) == 21  # three out, three in


# ------------------------------------------------------------------------------------------------ 3. the next frame against the oracle of the new chart
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_next_frame_follows_the_oracle_of_the_new_chart(pair, frame_case):
    a, b = pair
    sc = frame_case
    for mode in MODES:
        batch = make_batch([a])
        set_mode(batch, 0, mode)
        plant_frame(batch, 0, sc)
        assert batch.convert_chart([(0, b)]) == [0]
        orc = OracleFilter(oracle_settings(b, mode))
        orc.set_eqf(*batch.slot(0).get_eqf(), batch.slot(0).get_sigma(), time=sc.t0)
        for u in sc.imus:
            batch.process_imu(0, u)
            orc.process_imu(u)
        assert batch.process_vision([(0, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
        orc.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
        e = parity(batch.slot(0), orc)
        print(f"{rcs.pair_name(pair)} {mode}: next frame, parity state {e[0]:.2e} Sigma {e[1]:.2e}")
        assert max(e) <= MODE_TOL[mode], (mode, e)


# ------------------------------------------------------------------------------------------------ 4. the innovation statistics do not see the chart
def last_innovation(core, k):
    dof, nis, logdet = C.c_int(), C.c_double(), C.c_double()
    assert core.elib.eqf_batch_last_innovation(core.h, k, C.byref(dof), C.byref(nis), C.byref(logdet)) == 0
    return dof.value, nis.value, logdet.value


@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_innovation_statistics_are_invariant(pair):
    """twin slots, one converted, take the same frame without propagation (k = 0, dt = 0), without the equivariant output"""
    a, b = pair
    worst = [0.0, 0.0]
    for N in [n for n in rcs.NS if n > 0]:
        core = BatchCore(bs.reference_defaults(useEquivariantOutput=0), 2)
        state, S = rcs.case(N)
        for k in range(2):
            core.set_slot_chart(k, a)
            core.set_state(k, *state)
            core.set_sigma(k, S)
        assert core.convert_chart([(1, b)]) == [0]
        cam, mid, y = rcs.frame(N)
        status = core.step([(k, cam, np.zeros((0, 13)), np.zeros(0), mid, y, np.zeros(13), 0.0) for k in range(2)])
        assert np.all(status == 0), status
        (dof0, nis0, ld0), (dof1, nis1, ld1) = last_innovation(core, 0), last_innovation(core, 1)
        assert core.last_result(0)[0] == core.last_result(1)[0] == bs.UPDATED
        e_nis, e_ld = abs(nis1 - nis0) / abs(nis0), abs(ld1 - ld0) / max(1.0, abs(ld0))
        worst = [max(worst[0], e_nis), max(worst[1], e_ld)]
        print(f"{rcs.pair_name(pair)} N {N}: dof {dof0}, NIS {nis0:.6g} off by {e_nis:.2e}, log det S {ld0:.6g} off by {e_ld:.2e}")
        assert dof0 == dof1 == 2 * N
        assert e_nis <= 1e-9 and e_ld <= 1e-9, (N, e_nis, e_ld)
        core.close()
    print(f"{rcs.pair_name(pair)}: worst NIS {worst[0]:.2e}, log det S {worst[1]:.2e}")


# ------------------------------------------------------------------------------------------------ 5. round trips
@pytest.mark.parametrize("N", [5, 64])
def test_round_trips(N):
    state, S = rcs.case(N)
    worst_back = worst_via = 0.0
    for a, b in rcs.PAIRS:
        c = [x for x in rcs.CHARTS if x not in (a, b)][0]
        batch = make_batch([a, a, a])
        for k in range(3):
            batch.slot(k).force_eqf(*state, S)
        assert batch.convert_chart([(0, b), (1, b), (2, c)]) == [0, 0, 0]
        assert batch.convert_chart([(0, a), (1, c)]) == [0, 0]
        back, via, direct = batch.slot(0).get_sigma(), batch.slot(1).get_sigma(), batch.slot(2).get_sigma()
        d_back, d_via = rel_fro(back, S), rel_fro(via, direct)
        worst_back, worst_via = max(worst_back, d_back), max(worst_via, d_via)
        assert d_back <= TOL and d_via <= TOL, (rcs.pair_name((a, b)), d_back, d_via)
        assert [batch.slot_chart(k) for k in range(3)] == [a, c, c]
    print(f"N {N}: a -> b -> a against the original {worst_back:.2e}; a -> b -> c against a -> c {worst_via:.2e}")


# ------------------------------------------------------------------------------------------------ 6. - 8. what is not touched
def test_own_chart_touches_nothing():
    for a in rcs.CHARTS:
        batch = make_batch([a])
        state, S = rcs.case(21)
        batch.slot(0).force_eqf(*state, S)
        before = (snap(batch, 0), bookkeeping(batch, 0), bytes(batch.get_slot_settings(0)))
        assert batch.convert_chart([(0, a)]) == [0]
        assert (snap(batch, 0), bookkeeping(batch, 0), bytes(batch.get_slot_settings(0))) == before


def test_empty_slot_is_relabelled_like_set_slot_chart():
    """no landmark, neither chart Normal: exactly what eqf_batch_set_slot_chart gives; with Normal on one side the sensor block changes"""
    state, S = rcs.case(0)
    batch = make_batch([COORD_EUCLIDEAN, COORD_EUCLIDEAN, COORD_EUCLIDEAN])
    for k in range(3):
        batch.slot(k).force_eqf(*state, S)
    assert batch.convert_chart([(0, COORD_INVDEPTH), (2, COORD_NORMAL)]) == [0, 0]
    batch.set_slot_chart(1, COORD_INVDEPTH)
    assert snap(batch, 0) == snap(batch, 1) and bytes(batch.get_slot_settings(0)) == bytes(batch.get_slot_settings(1))
    assert batch.slot(0).get_sigma().tobytes() == np.asfortranarray(S).tobytes()
    assert rel_fro(batch.slot(2).get_sigma(), rcs.expected(0, COORD_EUCLIDEAN, COORD_NORMAL)) <= TOL and batch.slot_chart(2) == COORD_NORMAL


def test_same_bytes_in_any_call_and_batch():
    """one slot converted alone in a batch of 1, and as slot 5 of a batch of 300 among other entries with a refused entry in the middle"""
    s = base_settings()
    N = 64
    state, S = rcs.case(N)
    for a, b in rcs.PAIRS:
        one = BatchCore(s, 1)
        one.set_slot_chart(0, a)
        one.set_state(0, *state)
        one.set_sigma(0, S)
        assert one.convert_chart([(0, b)]) == [0]
        big = BatchCore(s, 300)
        for k, n in ((5, N), (299, 21), (0, 5), (17, 0)):
            big.set_slot_chart(k, a)
            big.set_state(k, *rcs.case(n)[0])
            big.set_sigma(k, rcs.case(n)[1])
        assert big.convert_chart([(299, b), (0, b), (300, b), (5, b), (17, b)]) == [0, 0, EQF_E_BAD_ARG, 0, 0]
        assert big.get_sigma(5).tobytes() == one.get_sigma(0).tobytes(), rcs.pair_name((a, b))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(big.get_state(5), one.get_state(0)))
        assert rel_fro(big.get_sigma(299), rcs.expected(21, a, b)) <= TOL
        one.close()
        big.close()


def test_unlisted_and_refused_slots_are_untouched():
    batch = make_batch([COORD_INVDEPTH] * 4)
    for k, N in enumerate((5, 21, 2, 64)):
        state, S = rcs.case(N)
        batch.slot(k).force_eqf(*state, S)
    before = [(snap(batch, k), bookkeeping(batch, k), bytes(batch.get_slot_settings(k))) for k in range(4)]
    # slot 1 done; slot 1 again: repeated; chart 3 and -1: outside the enum; slots 4 and -1: bad index; slot 0 after its refused entry: named already; slot 2 unlisted
    status = batch.convert_chart([(1, COORD_NORMAL), (1, COORD_EUCLIDEAN), (3, 3), (4, COORD_NORMAL), (-1, COORD_NORMAL), (0, -1), (0, COORD_NORMAL)])
    assert status == [0] + [EQF_E_BAD_ARG] * 6
    for k in (0, 2, 3):
        assert (snap(batch, k), bookkeeping(batch, k), bytes(batch.get_slot_settings(k))) == before[k], k
    assert batch.slot_chart(1) == COORD_NORMAL and rel_fro(batch.slot(1).get_sigma(), rcs.expected(21, COORD_INVDEPTH, COORD_NORMAL)) <= TOL
    assert batch.convert_chart([]) == []
    with pytest.raises(BatchError) as err:
        batch.slot(0).convert_chart(7)
    assert err.value.code == EQF_E_BAD_ARG and (snap(batch, 0), bookkeeping(batch, 0)) == before[0][:2]
    batch.slot(0).convert_chart(COORD_EUCLIDEAN)
    assert batch.slot(0).chart == COORD_EUCLIDEAN
    # the existing refusals stay: the chart of a slot that holds landmarks, by the settings calls and across a copy
    with pytest.raises(BatchError):
        batch.set_slot_chart(2, COORD_EUCLIDEAN)
    with pytest.raises(BatchError):
        batch.set_slot_settings(2, base_settings())
    assert batch.copy_slots([(2, 0)]) == [EQF_E_BAD_ARG]


# ------------------------------------------------------------------------------------------------ 9. what a conversion keeps
def test_conversion_keeps_settings_modes_totals_and_results(frame_case):
    sc = frame_case
    own = dict(measurementNoise=0.4, outlierThresholdAbs=9.0, outlierThresholdProb=5.0, initialPointVariance=0.07)
    batch = make_batch([COORD_INVDEPTH], **own)
    set_mode(batch, 0, "discrete")
    rng = np.random.default_rng(9400)
    st, V, lam = plant_nees(rng, 20, COORD_INVDEPTH)
    lam[3] = -1e-9  # a NEES that takes the partial-pivot fallback
    batch.slot(0).force_eqf(*st, spd(V, lam))
    orc = OracleFilter(bn.with_chart(base_settings(**own), COORD_INVDEPTH))
    orc.set_eqf(*st, spd(V, lam))
    assert batch.compute_nees([(0, *true_of(orc, rng))])[1][0] == 0 and batch.nees_lu_fallbacks(0) == 1
    plant_frame(batch, 0, sc)
    for u in sc.imus:
        batch.process_imu(0, u)
    assert batch.process_vision([(0, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    kept = bookkeeping(batch, 0)
    assert kept[3][0] == 1 and kept[4][0] & bs.UPDATED and kept[5][0] > 0 and kept[6] == 1 and kept[7][0] == 2 and kept[1:3] == MODES["discrete"]
    state = snap(batch, 0)[:5]
    for b in (COORD_NORMAL, COORD_EUCLIDEAN, COORD_INVDEPTH):
        assert batch.convert_chart([(0, b)]) == [0]
        assert bookkeeping(batch, 0) == kept and snap(batch, 0)[:5] == state, b
        got = batch.get_slot_settings(0)
        assert got.coordinateChoice == b and got.measurementNoise == 0.4 and got.initialPointVariance == 0.07


# ------------------------------------------------------------------------------------------------ 10. NEES of a converted slot
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_nees_of_a_converted_slot(pair):
    a, b = pair
    rng = np.random.default_rng(9500)
    batch = make_batch([a] * len(rcs.NS))
    for k, N in enumerate(rcs.NS):
        batch.slot(k).force_eqf(*rcs.case(N)[0], rcs.case(N)[1])
    assert batch.convert_chart([(k, b) for k in range(len(rcs.NS))]) == [0] * len(rcs.NS)
    entries, refs = [], []
    for k, N in enumerate(rcs.NS):
        orc = OracleFilter(bn.with_chart(base_settings(), b))
        orc.set_eqf(*rcs.case(N)[0], batch.slot(k).get_sigma())
        tr = true_of(orc, rng)
        entries.append((k, *tr))
        refs.append(orc.compute_nees(*tr))
    vals, status = batch.compute_nees(entries)
    assert np.all(status == 0)
    worst = max(abs(v - r) / abs(r) for v, r in zip(vals, refs))
    print(f"{rcs.pair_name(pair)}: NEES of the converted slots against the oracle of the new chart {worst:.2e}")
    assert worst <= TOL, (vals, refs)
    assert all(batch.nees_lu_fallbacks(k) == 0 for k in range(len(rcs.NS)))


# ------------------------------------------------------------------------------------------------ 11. a Normal slot reaches a Euclidean context
def test_normal_slot_is_stored_into_a_euclidean_context():
    N = 21
    state, S = rcs.case(N)
    batch = make_batch([COORD_NORMAL])
    batch.slot(0).force_eqf(*state, S)
    core = EqfCore(N, COORD_EUCLIDEAN)
    with pytest.raises(BatchError) as err:
        batch.slot(0).store_to(core)
    assert err.value.code == EQF_E_BAD_ARG  # the existing refusal stays
    batch.slot(0).convert_chart(COORD_EUCLIDEAN)
    batch.slot(0).store_to(core)
    assert core.get_sigma().tobytes() == batch.slot(0).get_sigma().tobytes()
    assert rel_fro(core.get_sigma(), rcs.expected(N, COORD_NORMAL, COORD_EUCLIDEAN)) <= TOL
    for x, y in zip(core.get_state(), batch.slot(0).get_eqf()):
        assert np.array_equal(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1))


# ------------------------------------------------------------------------------------------------ 12. the filter level: warm up once, branch into three charts
def test_branch_into_three_charts_in_one_step(frame_case):
    sc = frame_case
    modes = ["fast", "accurate", "discrete"]

    def branched():
        batch = make_batch([COORD_EUCLIDEAN] * 3)
        for k in range(3):
            set_mode(batch, k, modes[k])
        plant_frame(batch, 0, sc)
        for u in sc.imus:
            batch.process_imu(0, u)
        assert batch.copy_slots([(0, 1), (0, 2)]) == [0, 0]  # the IMU buffer and the time travel with the copy
        assert batch.convert_chart([(0, COORD_EUCLIDEAN), (1, COORD_INVDEPTH), (2, COORD_NORMAL)]) == [0, 0, 0]
        assert [batch.slot_chart(k) for k in range(3)] == rcs.CHARTS and [batch.slot_riccati(k) for k in range(3)] == [MODES[m][0] for m in modes]
        return batch

    together, alone = branched(), branched()
    assert np.all(together.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k in range(3)]) == 0)
    for k in (2, 0, 1):
        assert alone.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    for k in range(3):
        assert snap(together, k) == snap(alone, k), k
        assert together.last_result(k) == alone.last_result(k) and together.last_innovation(k) == alone.last_innovation(k)
        assert together.last_result(k)[0] & bs.UPDATED
    sig = [together.slot(k).get_sigma() for k in range(3)]
    assert rel_fro(sig[1], sig[0]) > 1e-3 and rel_fro(sig[2], sig[0]) > 1e-3  # three descriptions, not three copies


# ------------------------------------------------------------------------------------------------ 13. / 14. the tool
SLOT_LINE = r"slot (\d+)(?: chart (\S+))?: (frames updated (\d+)  failed (\d+)  mean NIS/dof (\S+)  log-likelihood (\S+))"


def test_eqvio_opt_rechart(tmp_path):
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([sim, "--duration", "2", "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    replay = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common, "--batch", "3",
              "--warmup", "10"]
    three = subprocess.run(replay + ["--rechart", "euclidean,invdepth,normal"], capture_output=True, text=True, timeout=120)
    same = subprocess.run(replay + ["--rechart", "invdepth"], capture_output=True, text=True, timeout=120)
    assert three.returncode == 0 and same.returncode == 0, (three.stderr[-2000:], same.stderr[-2000:])
    total = int(re.search(r"and (\d+) vision measurements in 3 slots", three.stdout).group(1))
    m = re.search(r"warm-up: 10 frames in slot 0, then copied into 2 slots; scores over the (\d+) frames after the warm-up", three.stdout)
    assert m and int(m.group(1)) == total - 10 > 20, three.stdout
    rows, rows_same = re.findall(SLOT_LINE, three.stdout), re.findall(SLOT_LINE, same.stdout)
    assert [(r[0], r[1]) for r in rows] == [("0", "euclidean"), ("1", "invdepth"), ("2", "normal")], three.stdout
    assert [(r[0], r[1]) for r in rows_same] == [("0", "invdepth"), ("1", "invdepth"), ("2", "invdepth")], same.stdout
    assert all(int(r[3]) > 20 and r[4] == "0" for r in rows), rows
    # the slot whose chart is the warm-up's chart scores what it scores when every slot keeps that chart
    assert len({r[2] for r in rows_same}) == 1 and rows[1][2] == rows_same[1][2], (rows, rows_same)
    assert rows[0][2] != rows[1][2] and rows[2][2] != rows[1][2], rows  # the other two are other filters from frame 10 on
    print("\n".join(f"slot {r[0]} chart {r[1]}: {r[2]}" for r in rows))
