"""Forking a context and changing its chart on the GPU (eqf_copy_ctx / eqf_convert_chart, k_ctx_copy / k_ctx_rechart in eqvio_amd/csrc/eqf_fork.hpp; VIOFilter
copy_from / convert_chart; `eqvio_opt --branchAt`): Sigma' against numpy's T Sigma T^T with the T of tests/rechart_cases.py at the sizes of tests/fork_cases.py,
independence of the capacity, the converted filter against a planted one of the new chart through a frame with turnover, its next frame against the oracle of
the new chart, round trips, the batch's conversion at N <= 64, the copy against the route through the host, the refusals, the filter level and the tool.
The bar is the project's flat 1e-9 relative (1e-8 for the discrete mode, its existing bound); comparisons are bit for bit unless a bound is named.

Worst deviations seen on an MI355X (profiles/r25_context_fork_parity.txt): Sigma' against numpy's T Sigma T^T 3.7e-16 (sensor-landmark and
landmark-landmark parts on their own 4.8e-16); the next frame against the oracle of the new chart 9.9e-13 fast, 9.9e-13 accurate, 2.1e-10 discrete; round trips
a -> b -> a 1.2e-15, a -> b -> c against a -> c 1.1e-15; against the batch's conversion 0 (bit-identical in all 36 cases run). Every test prints its figures."""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_normal_cases as bn
import batch_scenarios as bs
import discrete_cases as dc
import fork_cases as fc
import rechart_cases as rcs
import riccati_cases as rc
from eqvio_amd.batch import VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, OPT_EARLY_DOORBELL, OPT_INNOVATION_STATS, OPT_SIGMA_FP32, EqfCore, EqfError, VIOFilter
from oracle_binding import OracleFilter
from run_configs import parity
from test_gpu_batch_bridge import CtxFrames, ctx_arrays, planted_ctx
from test_gpu_batch_copy import no_outliers, same
from util import estimate_landmarks, random_spd, reasonable_state, rel_fro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
EQF_E_BAD_ARG, EQF_E_UNSUPPORTED = -3, -6
PAIR_IDS = [rcs.pair_name(p) for p in rcs.PAIRS]
MODE_TOL = {"fast": 1e-9, "accurate": 1e-9, "discrete": 1e-8}


def planted(N, chart, cap=None):
    """a context of capacity cap (default N) holding tests/rechart_cases.py's case(N) under `chart`"""
    state, S = rcs.case(N)
    core = EqfCore(max(N if cap is None else cap, 1), chart)
    core.set_state(*state)
    core.set_sigma(S)
    return core


def launches_expected(N, pair):
    return 1 if N > 0 or COORD_NORMAL in pair else 0


def settings(chart, mode="fast", **kw):
    s = bn.with_chart(bs.shipped_euroc(**kw), chart)
    return s if mode == "fast" else rc.oracle_settings(s) if mode == "accurate" else dc.oracle_settings(s)


def filter_arrays(f):
    return tuple(f.get_eqf()) + (f.get_sigma(),)


_frames = {}


def frame_case(N):
    """one planted frame with turnover (3 landmarks lost, 3 new) and two IMU samples, near landmarks: tests/riccati_cases.py's generator; built once per size"""
    if N not in _frames:
        _frames[N] = rc.make(settings(COORD_EUCLIDEAN), f"fork_turnover_{N}", 9400 + N, N, *rc.evenly(2), lost=3, new=3)
    return _frames[N]


def planted_filter(s, sc, state=None, Sigma=None):
    st = sc.state if state is None else state
    f = VIOFilter(s, max_landmarks=len(st[2]) + 8, sensor=sc.state[0], ids=st[2], p=np.ones((len(st[2]), 3)), time=sc.t0)
    f.force_eqf(*st, sc.Sigma if Sigma is None else Sigma)
    return f


def run_frame(filters, sc):
    for f in filters:
        for u in sc.imus:
            f.process_imu(u)
        f.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)


# ------------------------------------------------------------------------------------------------ 1. Sigma' = T Sigma T^T on the size grid
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_sigma_is_the_congruence(pair):
    a, b = pair
    worst = worst_part = 0.0
    for N in fc.SIZES:
        core = planted(N, a)
        before = ctx_arrays(core)
        assert core.chart == a and core.fork_stats() == (0, 0)
        core.convert_chart(b)
        after = ctx_arrays(core)
        S1, E = after[5], rcs.expected(N, a, b)
        d = rel_fro(S1, E)
        worst = max(worst, d)
        print(f"{rcs.pair_name(pair)} N {N}: Sigma' against numpy's T Sigma T^T {d:.2e}")
        assert d <= TOL, (N, d)
        if N > 0:  # under InvDepth the landmark rows are ~1e-3 of the sensor rows: each part of Sigma' on its own, so the small ones are not hidden
            d_cross, d_lm = rel_fro(S1[21:, :21], E[21:, :21]), rel_fro(S1[21:, 21:], E[21:, 21:])
            worst_part = max(worst_part, d_cross, d_lm)
            assert d_cross <= TOL and d_lm <= TOL, (N, d_cross, d_lm)
        assert np.array_equal(S1, S1.T), N  # symmetric bit for bit
        assert same(after[:5], before[:5]), N  # xi0, X, ids, q0, Q: bit for bit
        assert core.chart == b and core.fork_stats() == (0, launches_expected(N, pair))
        if COORD_NORMAL not in pair:  # the sensor block is copied bit for bit
            assert np.array_equal(S1[:21, :21], before[5][:21, :21]), N
        core.close()
    print(f"{rcs.pair_name(pair)}: worst {worst:.2e}; sensor-landmark and landmark-landmark parts on their own {worst_part:.2e}")


# ------------------------------------------------------------------------------------------------ 2. the capacity does not enter
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_result_does_not_depend_on_the_capacity(pair):
    a, b = pair
    for N in (5, 33, 200):
        tight, wide = planted(N, a), planted(N, a, cap=3 * N + 100)  # another leading dimension, another plane stride
        tight.convert_chart(b)
        wide.convert_chart(b)
        assert same(ctx_arrays(tight), ctx_arrays(wide)), N
        tight.close()
        wide.close()


# ------------------------------------------------------------------------------------------------ 3. the converted filter is the planted one of the new chart
@pytest.mark.parametrize("N", [21, 200])
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_converted_filter_is_the_planted_one_through_a_frame(pair, N):
    """N = 200: the look-ahead factorisation's route. Pins the chart constants the new chart reads and every cache the conversion must drop."""
    a, b = pair
    sc = frame_case(N)
    A = planted_filter(settings(a), sc)
    A.set_innovation_stats(True)
    A.convert_chart(b)
    st, S1 = A.get_eqf(), A.get_sigma()
    B = planted_filter(settings(b), sc, st, S1)
    B.set_innovation_stats(True)
    assert same(filter_arrays(A), filter_arrays(B))
    run_frame([A, B], sc)
    assert same(filter_arrays(A), filter_arrays(B)), "state or Sigma differ after the frame"
    assert A.last_innovation() == B.last_innovation() and A.last_innovation()[0] > 0
    assert A.innovation_totals() == B.innovation_totals()
    assert len(A.get_eqf()[2]) == N and not same(A.get_eqf()[2:3], st[2:3])  # three out, three in


# ------------------------------------------------------------------------------------------------ 4. the next frame against the oracle of the new chart
@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_next_frame_follows_the_oracle_of_the_new_chart(pair):
    a, b = pair
    sc = frame_case(21)
    for mode in MODE_TOL:
        flt = planted_filter(settings(a, mode), sc)
        flt.convert_chart(b)
        orc = OracleFilter(settings(b, mode))
        orc.set_eqf(*flt.get_eqf(), flt.get_sigma(), time=sc.t0)
        run_frame([flt, orc], sc)
        e = parity(flt, orc)
        print(f"{rcs.pair_name(pair)} {mode}: next frame, parity state {e[0]:.2e} Sigma {e[1]:.2e}")
        assert max(e) <= MODE_TOL[mode], (mode, e)


# ------------------------------------------------------------------------------------------------ 5. round trips
def test_round_trips():
    worst_back = worst_via = 0.0
    for N in (5, 65, 200):
        S = rcs.case(N)[1]
        for a in rcs.CHARTS:
            for b in rcs.CHARTS:
                if b == a:
                    continue
                core = planted(N, a)
                core.convert_chart(b)
                core.convert_chart(a)
                d = rel_fro(core.get_sigma(), S)
                worst_back = max(worst_back, d)
                assert d <= TOL and core.chart == a, (N, a, b, d)
                core.close()
                (c,) = [x for x in rcs.CHARTS if x not in (a, b)]
                via, direct = planted(N, a), planted(N, a)
                via.convert_chart(b)
                via.convert_chart(c)
                direct.convert_chart(c)
                d = rel_fro(via.get_sigma(), direct.get_sigma())
                worst_via = max(worst_via, d)
                assert d <= TOL and same(ctx_arrays(via)[:5], ctx_arrays(direct)[:5]), (N, a, b, c, d)
                via.close()
                direct.close()
    print(f"round trips: a -> b -> a against the original {worst_back:.2e}; a -> b -> c against a -> c {worst_via:.2e}")


def test_own_chart_and_empty_contexts():
    for a in rcs.CHARTS:  # a -> a: every byte stays, nothing is launched
        core = planted(21, a)
        before = ctx_arrays(core)
        core.convert_chart(a)
        assert same(ctx_arrays(core), before) and core.chart == a and core.fork_stats() == (0, 0)
        core.close()
    S = rcs.case(0)[1]
    for a, b in ((COORD_EUCLIDEAN, COORD_INVDEPTH), (COORD_INVDEPTH, COORD_EUCLIDEAN)):  # no landmark, neither chart Normal: relabelled, no launch
        core = planted(0, a)
        core.convert_chart(b)
        assert core.chart == b and np.array_equal(core.get_sigma(), S) and core.fork_stats() == (0, 0)
        core.close()
    for a in (COORD_EUCLIDEAN, COORD_INVDEPTH):  # ... to and from Normal: the sensor congruence
        core = planted(0, a)
        core.convert_chart(COORD_NORMAL)
        S1 = core.get_sigma()
        d = rel_fro(S1, rcs.expected(0, a, COORD_NORMAL))
        assert d <= TOL and rel_fro(S1, S) > 1e-3 and core.fork_stats() == (0, 1), d
        core.convert_chart(a)
        assert rel_fro(core.get_sigma(), S) <= TOL and core.fork_stats() == (0, 2)
        core.close()


# ------------------------------------------------------------------------------------------------ 6. the batch's conversion at N <= 64
def test_agrees_with_the_batchs_conversion():
    worst, identical, runs = 0.0, 0, 0
    for N in [n for n in fc.SIZES if 0 < n <= 64]:
        for a in (COORD_EUCLIDEAN, COORD_INVDEPTH):  # (the bridge refuses Normal-chart contexts)
            for b in [x for x in rcs.CHARTS if x != a]:
                core = planted(N, a, cap=64)
                batch = VIOFilterBatch(settings(COORD_EUCLIDEAN), 1, 64)
                batch.set_slot_chart(0, a)
                assert batch.load_core(core, [0]) == [0]
                assert batch.convert_chart([(0, b)]) == [0]
                core.convert_chart(b)
                Sc, Sb = core.get_sigma(), batch.slot(0).get_sigma()
                d = rel_fro(Sc, Sb)
                worst, identical, runs = max(worst, d), identical + int(np.array_equal(Sc, Sb)), runs + 1
                assert d <= TOL, (N, a, b, d)
                core.close()
    print(f"context against batch conversion: worst {worst:.2e}; bit-identical in {identical} of {runs} cases")


# ------------------------------------------------------------------------------------------------ 7. copy
#        N, source capacity, destination capacity, destination N before
COPIES = [(40, 40, 8, 5), (40, 48, 40, 40), (40, 40, 300, 0), (200, 200, 16, 9), (0, 8, 40, 17), (1, 8, 8, 3), (65, 80, 64, 64)]


@pytest.mark.parametrize("N,cap_s,cap_d,Nd", COPIES)
def test_copy_equals_the_host_route(N, cap_s, cap_d, Nd):
    src = planted(N, COORD_INVDEPTH, cap=cap_s)
    dst, twin = planted_ctx(cap_d, Nd, 31000 + Nd), planted_ctx(cap_d, Nd, 31000 + Nd)
    ref = ctx_arrays(src)
    dst.copy_from(src)  # the device
    twin.set_state(*ref[:5])  # the host route
    twin.set_sigma(ref[5])
    assert same(ctx_arrays(dst), ref) and same(ctx_arrays(twin), ref) and same(ctx_arrays(src), ref)
    assert dst.N == N and dst.fork_stats() == (1, 0) and src.fork_stats() == (0, 0)
    if N >= 4:  # a frame with turnover on both: two landmarks leave, two come
        fr = CtxFrames(no_outliers(), 31100 + N)
        for c in (dst, twin):
            c.remove_landmarks([0, N // 2])
            c.add_landmarks(np.array([7000, 7001], np.int32), np.array([[0.4, -0.3, 6.0], [-0.5, 0.2, 7.0]]), 0.3)
        now = ctx_arrays(dst)
        assert same(ctx_arrays(twin), now) and len(now[2]) == N
        f = fr.make(now[2], estimate_landmarks(now[3], now[4]))
        for c in (dst, twin):
            fr.run(c, f)
        assert same(ctx_arrays(dst), ctx_arrays(twin))
    for c in (src, dst, twin):
        c.close()


@pytest.mark.parametrize("busy", ["update", "reshape", "held"])
def test_copy_from_a_context_with_work_in_flight(busy):
    """tests/test_gpu_batch_bridge.py's three states of a context that is not at rest: read as eqf_get_state reads it, and going on as its twin that was not read"""
    s = no_outliers()
    N = 40
    rng = np.random.default_rng(32000)
    st = reasonable_state(rng, N)
    S = random_spd(rng, 21 + 3 * N)
    read, twin = EqfCore(N + 8, COORD_INVDEPTH), EqfCore(N + 8, COORD_INVDEPTH)
    for c in (read, twin):
        c.set_state(*st)
        c.set_sigma(S)
    ids, p = st[2], estimate_landmarks(st[3], st[4])
    fr = CtxFrames(s, 32001)
    new_ids, new_p = np.array([500, 501], np.int32), np.array([[0.4, -0.3, 6.0], [-0.5, 0.2, 7.0]])
    first = fr.make(ids, p)
    dst = planted_ctx(16, 5, 32002)  # before the contexts get busy: creating a context allocates, which waits for the device
    for c in (twin, read):
        if busy == "update":  # an update that may have been taken from the early doorbell: the lift's results are then not in yet
            fr.run(c, first)
        elif busy == "reshape":  # recorded, not applied
            c.remove_landmarks([0, 5])
            c.add_landmarks(new_ids, new_p, 0.3)
        else:
            held = c.add_landmarks_held(new_ids, new_p, 0.3)
    unsettled = read.lib.eqf_update_unsettled(read.h)  # (reads a flag of the handle: no device work)
    dst.copy_from(read)  # directly behind, no call in between
    print(f"{busy}: the update was unsettled at the copy: {unsettled}")
    ref = ctx_arrays(read)
    assert same(ctx_arrays(dst), ref)
    if busy == "reshape":
        assert list(ref[2]) == [int(i) for i in ids if i not in (ids[0], ids[5])] + [500, 501]
    if busy == "held":
        assert list(ref[2][-2:]) == ([500, 501] if held else [int(ids[-2]), int(ids[-1])])
    now_ids = ref[2]
    known = {int(i): q for i, q in zip(ids, p)}
    known.update({500: new_p[0], 501: new_p[1]})
    nxt = fr.make(now_ids, [known[int(i)] for i in now_ids])
    for c in (read, twin):  # the source goes on as its twin, which was not read
        fr.run(c, nxt)
    assert same(ctx_arrays(read), ctx_arrays(twin))


def test_destination_keeps_its_options_and_totals_and_a_self_copy_does_nothing():
    s = no_outliers()
    dst = planted_ctx(40, 20, 33000)
    dst.set_option(OPT_INNOVATION_STATS, 1)
    dst.set_option(OPT_EARLY_DOORBELL, 0)
    got = ctx_arrays(dst)
    fr = CtxFrames(s, 33001)
    fr.run(dst, fr.make(got[2], estimate_landmarks(got[3], got[4])))
    totals = dst.innovation_totals()
    assert totals[0] == 1 and totals[1] == 40
    src = planted_ctx(64, 33, 33002)
    dst.copy_from(src)
    assert same(ctx_arrays(dst), ctx_arrays(src))
    assert dst.get_option(OPT_INNOVATION_STATS) == 1 and dst.get_option(OPT_EARLY_DOORBELL) == 0 and dst.innovation_totals() == totals
    assert src.get_option(OPT_INNOVATION_STATS) == 0 and src.get_option(OPT_EARLY_DOORBELL) == 1 and dst.fork_stats() == (1, 0)
    ref = ctx_arrays(dst)
    dst.copy_from(dst)  # dst == src: nothing
    assert same(ctx_arrays(dst), ref) and dst.fork_stats() == (1, 0) and dst.innovation_totals() == totals
    assert dst.fork_stats(reset=True) == (1, 0) and dst.fork_stats() == (0, 0)


# ------------------------------------------------------------------------------------------------ 8. refusals
def code_of(call, *args):
    with pytest.raises(EqfError) as err:
        call(*args)
    return err.value.code


def test_refusals_leave_everything_untouched():
    inv, euc, nrm = planted(5, COORD_INVDEPTH, cap=16), planted(5, COORD_EUCLIDEAN, cap=16), planted(5, COORD_NORMAL, cap=16)
    kept = [ctx_arrays(c) for c in (inv, euc, nrm)]

    def untouched():
        return all(same(ctx_arrays(c), k) for c, k in zip((inv, euc, nrm), kept)) and (inv.chart, euc.chart, nrm.chart) == (COORD_INVDEPTH, COORD_EUCLIDEAN, COORD_NORMAL)

    # a chart mismatch with landmarks
    for d, s in ((inv, euc), (euc, inv), (nrm, inv), (inv, nrm)):
        assert code_of(d.copy_from, s) == EQF_E_BAD_ARG and untouched()
    # without landmarks: Euclidean and InvDepth take each other's, Normal does not mix
    e0, i0, n0 = planted(0, COORD_EUCLIDEAN, cap=8), planted(0, COORD_INVDEPTH, cap=8), planted(0, COORD_NORMAL, cap=8)
    assert code_of(inv.copy_from, n0) == EQF_E_BAD_ARG and code_of(nrm.copy_from, e0) == EQF_E_BAD_ARG and untouched()
    spare = planted(5, COORD_INVDEPTH, cap=16)
    spare.copy_from(e0)
    assert spare.N == 0 and spare.chart == COORD_INVDEPTH and same(ctx_arrays(spare), ctx_arrays(e0))
    spare_n = planted(3, COORD_NORMAL, cap=16)
    spare_n.copy_from(n0)
    assert spare_n.N == 0 and same(ctx_arrays(spare_n), ctx_arrays(n0))
    # a chart outside the enum
    for bad in (-1, 3, 7):
        assert code_of(inv.convert_chart, bad) == EQF_E_BAD_ARG and untouched()
    # the float store, on either side and for both calls
    f32 = planted(5, COORD_INVDEPTH, cap=16)
    f32.set_option(OPT_SIGMA_FP32, 2)
    kept32 = ctx_arrays(f32)
    assert code_of(f32.copy_from, inv) == EQF_E_UNSUPPORTED and code_of(inv.copy_from, f32) == EQF_E_UNSUPPORTED
    assert code_of(f32.convert_chart, COORD_EUCLIDEAN) == EQF_E_UNSUPPORTED
    assert untouched() and same(ctx_arrays(f32), kept32) and f32.chart == COORD_INVDEPTH and f32.fork_stats() == (0, 0) and inv.fork_stats() == (0, 0)


def test_rounding_model_rounds_as_set_sigma_does():
    """EQF_OPT_SIGMA_FP32 = 1: Sigma is rounded to float behind the copy and behind the conversion, as behind eqf_set_sigma"""
    N = 21
    state, S = rcs.case(N)
    src = planted(N, COORD_INVDEPTH)
    dst, twin = EqfCore(32, COORD_INVDEPTH), EqfCore(32, COORD_INVDEPTH)
    for c in (dst, twin):
        c.set_option(OPT_SIGMA_FP32, 1)
    dst.copy_from(src)
    twin.set_state(*state)
    twin.set_sigma(S)
    S32 = twin.get_sigma()
    assert same(ctx_arrays(dst), ctx_arrays(twin)) and np.array_equal(S32, S32.astype(np.float32).astype(np.float64)) and not np.array_equal(S32, S)
    # the conversion of the rounded Sigma in fp64, then set through eqf_set_sigma of a rounding context: what the rounding context's own conversion leaves
    plain = EqfCore(32, COORD_INVDEPTH)
    plain.set_state(*state)
    plain.set_sigma(S32)
    plain.convert_chart(COORD_NORMAL)
    dst.convert_chart(COORD_NORMAL)
    want = EqfCore(32, COORD_NORMAL)
    want.set_option(OPT_SIGMA_FP32, 1)
    want.set_state(*state)
    want.set_sigma(plain.get_sigma())
    assert same(ctx_arrays(dst), ctx_arrays(want)) and not np.array_equal(dst.get_sigma(), plain.get_sigma())
    assert dst.get_option(OPT_SIGMA_FP32) == 1 and dst.chart == COORD_NORMAL


# ------------------------------------------------------------------------------------------------ 9. the filter level and the tool
def test_filter_copy_carries_the_host_half():
    """a frame with turnover: the source F and its twin U that is not read; the copy D and a filter H built the host way from what F shows"""
    sc = frame_case(21)
    s = settings(COORD_INVDEPTH)
    F, U = planted_filter(s, sc), planted_filter(s, sc)
    for u in sc.imus:
        F.process_imu(u)
        U.process_imu(u)
    D = VIOFilter(s, max_landmarks=8)  # fresh: not initialised, no landmark, capacity below the source's 21
    assert not D.is_initialised()
    D.copy_from(F)
    assert D.is_initialised() and D.get_time() == F.get_time() == sc.t0
    held = filter_arrays(F)
    assert same(filter_arrays(D), held)
    H = planted_filter(s, sc, held[:5], held[5])
    for u in sc.imus:
        H.process_imu(u)
    for f in (F, U, D, H):
        f.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)  # D has the IMU samples only if the copy carried the buffer
    ref = filter_arrays(H)
    assert len(ref[2]) == 21 and not same(ref[2:3], held[2:3])
    for f in (F, U, D):
        assert same(filter_arrays(f), ref) and f.get_time() == sc.stamp
    assert np.array_equal(D.state_estimate()[1], H.state_estimate()[1])
    # convert_chart at the filter level: the core reports the chart, the next frame is the oracle's under the new chart's settings (test 4 runs on it)
    D.convert_chart(COORD_EUCLIDEAN)
    from eqvio_amd.capi import load_eqf_lib

    assert load_eqf_lib().eqf_chart(D.core_handle()) == COORD_EUCLIDEAN and load_eqf_lib().eqf_chart(F.core_handle()) == COORD_INVDEPTH
    with pytest.raises(RuntimeError):
        D.copy_from(F)  # F's landmarks are in InvDepth coordinates
    assert same(filter_arrays(F), ref)


BRANCH_LINE = r"branch (\d+) chart (\S+): (frames updated (\d+)  mean NIS/dof (\S+)  log-likelihood (\S+))"
FINAL_LINE = r"branch (\d+) chart (\S+): (final time \S+  position \S+ \S+ \S+  landmarks \d+)"


def test_eqvio_opt_branches_into_three_charts(tmp_path):
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([sim, "--duration", "2", "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    replay = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", "--nis", *common]
    mixed = subprocess.run(replay + ["--branchAt", "10", "--branchCharts", "euclidean,invdepth,normal"], capture_output=True, text=True, timeout=120)
    alike = subprocess.run(replay + ["--branchAt", "10", "--branchCharts", "invdepth,invdepth,invdepth"], capture_output=True, text=True, timeout=120)
    assert mixed.returncode == 0 and alike.returncode == 0, (mixed.stderr[-2000:], alike.stderr[-2000:])
    total = int(re.search(r"and (\d+) vision measurements", mixed.stdout).group(1))
    m = re.search(r"branch: 10 frames on a single filter \(chart invdepth\), then copied into 3 filters and converted; scores over the (\d+) frames after the branch", mixed.stdout)
    assert m and int(m.group(1)) == total - 10 > 20, mixed.stdout
    rows, rows0 = re.findall(BRANCH_LINE, mixed.stdout), re.findall(BRANCH_LINE, alike.stdout)
    fin, fin0 = re.findall(FINAL_LINE, mixed.stdout), re.findall(FINAL_LINE, alike.stdout)
    assert [(r[0], r[1]) for r in rows] == [("0", "euclidean"), ("1", "invdepth"), ("2", "normal")] == [(r[0], r[1]) for r in fin], mixed.stdout
    assert [(r[0], r[1]) for r in rows0] == [(str(k), "invdepth") for k in range(3)], alike.stdout
    assert len({r[2] for r in rows}) == 3, rows  # three charts, three different scores
    assert 20 < int(rows[1][3]) <= total - 10  # no warm-up frame is scored
    assert len({r[2] for r in rows0}) == 1 and len({r[2] for r in fin0}) == 1, rows0  # one filter three times over: the same text
    assert rows[1][2] == rows0[1][2] and fin[1][2] == fin0[1][2]  # the branch in the warm-up's own chart is that filter
    print("\n".join(f"branch {r[0]} chart {r[1]}: {r[2]}" for r in rows))
