"""The bridge between a context and the slots of the filter batch on the GPU (eqf_batch_load_ctx / _store_ctx / k_batch_bridge, eqvio_batch_load_filter /
_store_filter): a slot loaded through the bridge is the slot the route through the host makes, bit for bit, now and in later frames, whatever the context's
capacity and whatever the slot held before; a context that has work in flight is read as eqf_get_state reads it and goes on as if it had not been read; one
context into many slots; the way back into a context, with growth; parity with the oracle on both sides; the refusals; what a destination keeps; the filter
level with its host half; `eqvio_opt --warmupOnFilter`. Comparisons are bit for bit unless TOL is named."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import slot_settings_cases as ssc
from eqvio_amd.batch import BatchError, VIOFilterBatch
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, OPT_SIGMA_FP32, EqfCore, VIOFilter
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from run_configs import parity
from test_gpu_batch_copy import SLOT_LINE, nees_bits, no_outliers, plant, prepare, same, shared_frame, snap
from util import estimate_landmarks, imu_selection, project, random_spd, reasonable_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG, EQF_E_CAPACITY, EQF_E_UNSUPPORTED = -3, -4, -6
TOL = 1e-9  # the project's flat parity bound
NONE_I, NONE_P = np.zeros(0, np.int32), np.zeros((0, 3))


def ctx_arrays(core):
    """everything of a context eqf_get_state / eqf_get_sigma show: xi0, X, ids, q0, Q, Sigma"""
    return tuple(core.get_state()) + (core.get_sigma(),)


def planted_ctx(cap, N, seed, chart=COORD_INVDEPTH, id_offset=0):
    rng = np.random.default_rng(seed)
    st = reasonable_state(rng, N, id_offset=id_offset)
    core = EqfCore(cap, chart)
    core.set_state(*st)
    core.set_sigma(random_spd(rng, 21 + 3 * N))
    return core


# ------------------------------------------------------------------------------------------------ 1. load equals the host route
#        context capacity, its N, destination N before, destination pair
LOADS = [(8, 0, 5, 0), (8, 1, 64, 1), (8, 7, 0, 0), (40, 0, 64, 0), (40, 1, 5, 1), (40, 7, 64, 1), (100, 63, 5, 0), (100, 63, 64, 1), (100, 64, 0, 0), (100, 64, 5, 1),
         (100, 64, 64, 0)]


@pytest.mark.parametrize("cap,N,Nd,dcur", LOADS)
def test_load_equals_the_host_route(cap, N, Nd, dcur):
    batch = VIOFilterBatch(no_outliers(), 2, 64)
    for k in (0, 1):  # both destinations alike: the same former state in the same pair
        prepare(batch, k, Nd, dcur, 21000 + Nd)
    core = planted_ctx(cap, N, 21100 + 7 * cap + N)
    ref = ctx_arrays(core)
    assert len(ref[2]) == N and ref[5].shape == (21 + 3 * N,) * 2
    assert batch.load_core(core, [0]) == [0]  # A: the bridge
    batch.slot(1).force_eqf(*ref)             # B: get_state / get_sigma -> set_state / set_sigma
    a, b = bs.slot_arrays(batch.slot(0)), bs.slot_arrays(batch.slot(1))
    assert same(a, ref) and same(b, ref)
    assert same(ctx_arrays(core), ref)  # the context shows what it showed
    rng = np.random.default_rng(21200 + N)
    if N:
        bits = nees_bits(batch, [0, 1], rng)
        assert bits[0] == bits[1]
    # three frames for both: up to capacity (first and last landmark leave), five leave and five come, all measured
    n = N
    for drop, add in (([0, n - 1] if n >= 3 else [], None), ([1, 20, 33, 50, 63], 5), ([], 0)):
        add = 64 - (n - len(drop)) if add is None else add
        shared_frame(batch, [0, 1], rng, drop, add)
        a, b = snap(batch, 0), snap(batch, 1)
        n = len(a[2])
        assert n == 64, n
        assert same(a, b)
        assert batch.last_innovation(0) == batch.last_innovation(1) and batch.last_result(0) == batch.last_result(1)
        assert batch.last_innovation(0)[0] > 0
        bits = nees_bits(batch, [0, 1], rng)
        assert bits[0] == bits[1]


# ------------------------------------------------------------------------------------------------ 2. a context that is not at rest
class CtxFrames:
    """frames for contexts that hold the same filter, through the entry points the filter level uses: stage, propagate, statistics + update"""

    def __init__(self, settings, seed):
        self.s, self.rng, self.t = settings, np.random.default_rng(seed), 0.0
        self.Qd, self.Pd, self.var = settings.input_gain_diag12(), settings.state_gain_diag8(), settings.measurementNoise**2

    def make(self, ids, p):
        """a frame that measures the landmarks ids at (about) the camera-frame points p"""
        stamp = self.t + bs.FRAME_DT
        imus = bs.frame_imus(self.rng, self.t, stamp, 2)
        dts, mean, total = imu_selection(imus, self.t, stamp)
        order = np.argsort(ids)
        y = (project(bs.PINHOLE, np.asarray(p)) + self.rng.normal(size=(len(ids), 2)) * 0.5)[order].reshape(-1)
        self.t = stamp
        return mean, total, imus, dts, np.asarray(ids, np.int32)[order], y

    def run(self, core, fr, orc=None):
        mean, total, imus, dts, mid, y = fr
        core.stage_measurement(mid, y)
        core.propagate_fast(mean, total, self.Qd, self.Pd, imus, dts, bool(self.s.useDiscreteVelocityLift))
        upd = core.stats_then_update(bs.PINHOLE, mid, y, 1e8, 1e8, self.var, bool(self.s.useEquivariantOutput), bool(self.s.useDiscreteInnovationLift))[0]
        assert upd == 1, upd
        if orc is not None:
            orc.integrate_riccati_fast(mean, total)
            for u, dt in zip(imus, dts):
                orc.integrate_observer(u, dt, bool(self.s.useDiscreteVelocityLift))
            orc.vision_update(bs.PINHOLE, mid, y)


@pytest.mark.parametrize("busy", ["update", "reshape", "held"])
def test_load_from_a_context_with_work_in_flight(busy):
    s = no_outliers()
    N = 40
    rng = np.random.default_rng(22000)
    st = reasonable_state(rng, N)
    S = random_spd(rng, 21 + 3 * N)
    read, twin = EqfCore(N + 8, COORD_INVDEPTH), EqfCore(N + 8, COORD_INVDEPTH)
    for c in (read, twin):
        c.set_state(*st)
        c.set_sigma(S)
    ids, p = st[2], estimate_landmarks(st[3], st[4])
    fr = CtxFrames(s, 22001)
    new_ids, new_p = np.array([500, 501], np.int32), np.array([[0.4, -0.3, 6.0], [-0.5, 0.2, 7.0]])
    first = fr.make(ids, p)
    batch = VIOFilterBatch(s, 2, 64)  # before the contexts get busy: creating a batch allocates, which waits for the device
    for c in (twin, read):
        if busy == "update":  # an update that may have been taken from the early doorbell: the lift's results are then not in yet
            fr.run(c, first)
        elif busy == "reshape":  # recorded, not applied
            c.remove_landmarks([0, 5])
            c.add_landmarks(new_ids, new_p, 0.3)
        else:
            held = c.add_landmarks_held(new_ids, new_p, 0.3)
    unsettled = read.lib.eqf_update_unsettled(read.h)  # (reads a flag of the handle: no device work)
    assert batch.load_core(read, [1]) == [0]  # directly behind, no call in between
    print(f"{busy}: the update was unsettled at the load: {unsettled}")
    ref = ctx_arrays(read)
    assert same(bs.slot_arrays(batch.slot(1)), ref)
    if busy == "reshape":
        assert list(ref[2]) == [int(i) for i in ids if i not in (ids[0], ids[5])] + [500, 501]
    if busy == "held":
        assert list(ref[2][-2:]) == ([500, 501] if held else [int(ids[-2]), int(ids[-1])])
    # the context goes on as its twin, which was not read
    now_ids = ref[2]
    known = {int(i): q for i, q in zip(ids, p)}
    known.update({500: new_p[0], 501: new_p[1]})
    nxt = fr.make(now_ids, [known[int(i)] for i in now_ids])
    for c in (read, twin):
        fr.run(c, nxt)
    assert same(ctx_arrays(read), ctx_arrays(twin))


# ------------------------------------------------------------------------------------------------ 3. fan-out
def test_fan_out_into_a_large_batch_and_a_batch_of_one():
    s = bs.shipped_euroc()
    B = 300
    batch = VIOFilterBatch(s, B, 64)
    rng = np.random.default_rng(23000)
    for k, n in ((1, 9), (3, 64), (B - 2, 17), (B - 1, 33)):  # some slots hold filters of their own
        xi0, Xs, ids, q0, Q = reasonable_state(rng, n, id_offset=1000 * k)
        batch.start_slot(k, xi0, NONE_I, NONE_P, 1.0 + k)
        batch.slot(k).force_eqf(xi0, Xs, ids, q0, Q, random_spd(rng, 21 + 3 * n))
    core = planted_ctx(40, 40, 23001)
    ref = ctx_arrays(core)
    before = [snap(batch, k) for k in range(B)]
    listed = [0, 3, B - 1]
    assert batch.load_core(core, listed) == [0, 0, 0]
    after = [snap(batch, k) for k in range(B)]
    for k in range(B):
        if k in listed:
            assert same(after[k][:6], ref), k
            assert after[k][6:] == before[k][6:]  # the device level does not know the host half
        else:
            assert same(before[k], after[k]), k
    rec, _, st = batch.state_estimates(listed)
    assert np.all(st == 0)
    assert bytes(rec[0]) == bytes(rec[1]) == bytes(rec[2]) and rec[0].N == 40
    one = VIOFilterBatch(s, 1, 64)
    assert one.load_core(core, [0]) == [0]
    assert same(bs.slot_arrays(one.slot(0)), ref)
    rec1, _, _ = one.state_estimates([0])
    assert bytes(rec1[0]) == bytes(rec[0])
    assert batch.load_core(core, []) == []


# ------------------------------------------------------------------------------------------------ 4. store
#         slot N, its pair, context capacity, context N before
STORES = [(40, 0, 8, 5), (3, 1, 64, 64), (0, 0, 16, 9), (64, 1, 100, 0), (7, 0, 40, 40)]


@pytest.mark.parametrize("N,cur,cap,Nc", STORES)
def test_store_equals_set_state_and_set_sigma(N, cur, cap, Nc):
    s = no_outliers()
    batch = VIOFilterBatch(s, 2, 64)
    prepare(batch, 1, N, cur, 24000 + N)
    slot = snap(batch, 1)
    assert len(slot[2]) == N
    X, Y = planted_ctx(cap, Nc, 24100 + Nc), planted_ctx(cap, Nc, 24100 + Nc)
    batch.slot(1).store_to(X)  # the bridge
    Y.set_state(*slot[:5])     # the host route
    Y.set_sigma(slot[5])
    x, y = ctx_arrays(X), ctx_arrays(Y)
    assert same(x, slot[:6]) and same(y, slot[:6])
    assert X.N == N and same(snap(batch, 1), slot)  # the slot is unchanged
    if N == 0:
        return
    fr = CtxFrames(s, 24200 + N)
    ids, p = x[2], estimate_landmarks(x[3], x[4])
    for _ in range(2):
        f = fr.make(ids, p)
        for c in (X, Y):
            fr.run(c, f)
        assert same(ctx_arrays(X), ctx_arrays(Y))


# ------------------------------------------------------------------------------------------------ 5. round trip
def test_round_trip_context_slot_context():
    first = planted_ctx(100, 64, 25000)
    batch = VIOFilterBatch(bs.shipped_euroc(), 3, 64)
    assert batch.load_core(first, [2]) == [0]
    second = planted_ctx(8, 3, 25001)
    batch.slot(2).store_to(second)
    assert same(ctx_arrays(first), ctx_arrays(second)) and second.N == 64


# ------------------------------------------------------------------------------------------------ 6. parity with the oracle on both sides
def test_parity_after_a_load_and_after_a_store():
    s = no_outliers()
    sc = bs.make(s, "bridge40", 26000, 40)
    core = EqfCore(40, COORD_INVDEPTH)
    core.set_state(*sc.state)
    core.set_sigma(sc.Sigma)
    batch = VIOFilterBatch(s, 2, 64)
    batch.start_slot(1, sc.state[0], NONE_I, NONE_P, sc.t0)
    assert batch.load_core(core, [1]) == [0]
    orc = OracleFilter(s)
    orc.set_eqf(*ctx_arrays(core), time=sc.t0)
    for u in sc.imus:
        batch.process_imu(1, u)
        orc.process_imu(u)
    assert batch.process_vision([(1, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    orc.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
    e = parity(batch.slot(1), orc)
    print(f"slot's next frame after a load, against the oracle started from the context: state {e[0]:.2e} Sigma {e[1]:.2e}")
    assert max(e) < TOL, e
    # and back: the context's next frame after a store of that slot
    other = planted_ctx(16, 5, 26001)
    batch.slot(1).store_to(other)
    got = ctx_arrays(other)
    orc2 = OracleFilter(s)
    orc2.set_eqf(*got, time=0.0)
    fr = CtxFrames(s, 26002)
    fr.run(other, fr.make(got[2], estimate_landmarks(got[3], got[4])), orc2)
    e = parity(other, orc2)
    print(f"context's next frame after a store, against the oracle started from the slot: state {e[0]:.2e} Sigma {e[1]:.2e}")
    assert max(e) < TOL, e


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_slots_untouched():
    base = bs.shipped_euroc()  # InvDepth
    batch = VIOFilterBatch(base, 4, 40)
    batch.set_slot_settings(1, ssc.clone(base, coordinateChoice=COORD_EUCLIDEAN))  # while it is empty
    rng = np.random.default_rng(27000)
    for k, n in enumerate((6, 4, 3, 0)):
        xi0, Xs, ids, q0, Q = reasonable_state(rng, n, id_offset=100 * k)
        batch.start_slot(k, xi0, NONE_I, NONE_P, 1.0 + k)
        batch.slot(k).force_eqf(xi0, Xs, ids, q0, Q, random_spd(rng, 21 + 3 * n))
    before = [snap(batch, k) for k in range(4)]
    elib, core_h = batch.elib, batch.core_handle()
    all4, st = (C.c_int * 4)(0, 1, 2, 3), (C.c_int * 4)(7, 7, 7, 7)

    def untouched():
        return all(same(before[k], snap(batch, k)) for k in range(4)) and list(st) == [7, 7, 7, 7]

    # of the whole call
    normal = planted_ctx(16, 5, 27001, chart=COORD_NORMAL)
    assert elib.eqf_batch_load_ctx(core_h, normal.h, 4, all4, st) == EQF_E_UNSUPPORTED and untouched()
    assert elib.eqf_batch_store_ctx(core_h, 0, normal.h) == EQF_E_UNSUPPORTED and same(ctx_arrays(normal), ctx_arrays(planted_ctx(16, 5, 27001, chart=COORD_NORMAL)))
    f32 = planted_ctx(16, 5, 27002)
    f32.set_option(OPT_SIGMA_FP32, 2)
    kept = ctx_arrays(f32)
    assert elib.eqf_batch_load_ctx(core_h, f32.h, 4, all4, st) == EQF_E_UNSUPPORTED and untouched()
    assert elib.eqf_batch_store_ctx(core_h, 0, f32.h) == EQF_E_UNSUPPORTED and same(ctx_arrays(f32), kept)
    big = planted_ctx(64, 41, 27003)
    assert elib.eqf_batch_load_ctx(core_h, big.h, 4, all4, st) == EQF_E_CAPACITY and untouched()
    with pytest.raises(BatchError) as err:
        batch.load_core(big, [0])
    assert err.value.code == EQF_E_CAPACITY and untouched()
    # per entry: a slot listed twice, bad indices, the Euclidean slot of an InvDepth context with landmarks; the other entries are done
    src = planted_ctx(16, 5, 27004)
    ref = ctx_arrays(src)
    assert batch.load_core(src, [2, 2, -1, 4, 1, 3]) == [0, EQF_E_BAD_ARG, EQF_E_BAD_ARG, EQF_E_BAD_ARG, EQF_E_BAD_ARG, 0]
    after = [snap(batch, k) for k in range(4)]
    assert same(before[0], after[0]) and same(before[1], after[1])
    assert same(after[2][:6], ref) and same(after[3][:6], ref) and not same(before[2], after[2])
    assert batch.get_slot_settings(1).coordinateChoice == COORD_EUCLIDEAN
    # the same mismatch without landmarks is accepted, in both directions
    empty = planted_ctx(16, 0, 27005)
    assert batch.load_core(empty, [1]) == [0] and same(bs.slot_arrays(batch.slot(1)), ctx_arrays(empty))
    euclid = planted_ctx(16, 4, 27006, chart=COORD_EUCLIDEAN)
    batch.slot(1).store_to(euclid)  # an empty Euclidean-chart slot... into a Euclidean context
    assert euclid.N == 0
    # store: a slot with landmarks into a context of the other chart, a bad slot
    kept = ctx_arrays(euclid)
    with pytest.raises(BatchError) as err:
        batch.slot(2).store_to(euclid)
    assert err.value.code == EQF_E_BAD_ARG and same(ctx_arrays(euclid), kept)
    assert elib.eqf_batch_store_ctx(core_h, 4, src.h) == EQF_E_BAD_ARG and elib.eqf_batch_store_ctx(core_h, -1, src.h) == EQF_E_BAD_ARG
    assert same(ctx_arrays(src), ref)


# ------------------------------------------------------------------------------------------------ 8. what the destination keeps
def test_destination_keeps_its_settings_totals_and_fallback_count():
    from test_gpu_batch_nees import plant as plant_nees, spd, true_of

    base = bs.shipped_euroc()
    own = ssc.clone(base, measurementNoise=0.4, outlierThresholdAbs=9.0, outlierThresholdProb=5.0)
    batch = VIOFilterBatch(base, 2, 64)
    batch.set_slot_settings(1, own)
    rng = np.random.default_rng(28000)
    st, V, lam = plant_nees(rng, 20, base.coordinateChoice)
    lam[3] = -1e-9
    batch.slot(1).force_eqf(*st, spd(V, lam))
    orc = OracleFilter(base)
    orc.set_eqf(*st, spd(V, lam))
    assert batch.compute_nees([(1, *true_of(orc, rng))])[1][0] == 0 and batch.nees_lu_fallbacks(1) == 1
    sc = bs.make(own, "first", 28001, 9, sigma_edit=ssc.tracking)
    plant(batch, 1, sc)
    assert batch.process_vision([(1, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    totals, last = batch.innovation_totals(1), batch.last_innovation(1)
    assert totals[0] == 1 and last[0] > 0 and batch.last_result(1)[0] != 0
    core = planted_ctx(40, 14, 28002)
    assert batch.load_core(core, [1]) == [0]
    assert same(bs.slot_arrays(batch.slot(1)), ctx_arrays(core))
    assert ssc.same_bytes(batch.get_slot_settings(1), own) and ssc.same_bytes(batch.get_slot_settings(0), base)
    assert batch.innovation_totals(1) == totals and batch.nees_lu_fallbacks(1) == 1
    assert batch.last_innovation(1) == (0, 0.0, 0.0) and batch.last_result(1) == (0, 0.0)


# ------------------------------------------------------------------------------------------------ 9. the filter level
def test_filter_level_moves_the_host_half_too():
    s = bs.shipped_euroc()
    w = SimWorld(seed=300, num_points=1500, max_features=40, trajectory="wave", noise_px=2.5)
    sensor, _, _ = w.true_state(0.0, NONE_I)
    frames = list(w.frames(13))
    flt = VIOFilter(s, max_landmarks=48, sensor=sensor, ids=NONE_I, p=NONE_P, time=0.0)
    for imus, stamp, mid, y in frames[:10]:
        for u in imus:
            flt.process_imu(u)
        flt.process_vision(stamp, w.cam, mid, y)
    held = tuple(flt.get_eqf()) + (flt.get_sigma(),)
    assert len(held[2]) > 10
    batch = VIOFilterBatch(s, 5, 64)
    assert batch.load_filter(flt, [0, 2, 4]) == [0, 0, 0]
    assert same(tuple(flt.get_eqf()) + (flt.get_sigma(),), held) and flt.get_time() == frames[9][1]
    # the reference: a slot forced to the filter's EqF state, at its time, with the sample the filter's buffer still holds
    batch.start_slot(3, sensor, NONE_I, NONE_P, flt.get_time())
    batch.slot(3).force_eqf(*held)
    batch.process_imu(3, frames[9][0][-1])
    for k in (0, 2, 4):
        assert same(snap(batch, k), snap(batch, 3)), k
        assert batch.slot(k).get_time() == flt.get_time() and batch.slot(k).is_initialised()
    assert not batch.slot(1).is_initialised()
    imus, stamp, mid, y = frames[10]
    for k in (0, 2, 3, 4):
        for u in imus:
            batch.process_imu(k, u)
    assert np.all(batch.process_vision([(k, stamp, w.cam, mid, y) for k in (0, 2, 3, 4)]) == 0)
    for k in (0, 2, 4):
        assert same(snap(batch, k), snap(batch, 3)), k
    assert batch.last_innovation(0)[0] > 0
    # and back: slot 2 into a second filter X; Y is a filter built the host way - the slot's ids, time and EqF state, and the sample the slot's buffer holds
    slot = snap(batch, 2)
    X = VIOFilter(s, max_landmarks=64, sensor=sensor, ids=NONE_I, p=NONE_P, time=0.0)
    batch.slot(2).store_to(X)
    Y = VIOFilter(s, max_landmarks=64, sensor=sensor, ids=slot[2], p=np.ones((len(slot[2]), 3)), time=float(slot[6]))
    Y.force_eqf(*slot[:6])
    Y.process_imu(frames[10][0][-1])
    assert same(snap(batch, 2), slot)
    for f in (X, Y):
        assert same(tuple(f.get_eqf()) + (f.get_sigma(),), slot[:6]) and f.get_time() == stamp and f.is_initialised()
    orc = OracleFilter(s)
    orc.set_eqf(*slot[:6], time=float(slot[6]))
    orc.process_imu(frames[10][0][-1])
    imus, stamp2, mid, y = frames[11]
    for f in (X, Y, orc):
        for u in imus:
            f.process_imu(u)
        f.process_vision(stamp2, w.cam, mid, y)
    assert same(tuple(X.get_eqf()) + (X.get_sigma(),), tuple(Y.get_eqf()) + (Y.get_sigma(),)) and X.get_time() == stamp2 == Y.get_time()
    assert np.array_equal(X.state_estimate()[1], Y.state_estimate()[1]) and len(X.get_eqf()[2]) > 10
    e = parity(X, orc)
    print(f"filter's next frame after a store, against the oracle started from the slot: state {e[0]:.2e} Sigma {e[1]:.2e}")
    assert max(e) < TOL, e
    # a filter of capacity 8 grows when it receives the slot
    Z = VIOFilter(s, max_landmarks=8, sensor=sensor, ids=NONE_I, p=NONE_P, time=0.0)
    batch.slot(2).store_to(Z)
    assert same(tuple(Z.get_eqf()) + (Z.get_sigma(),), slot[:6]) and Z.get_time() == stamp


# ------------------------------------------------------------------------------------------------ 10. the tool
def test_eqvio_opt_warmup_on_filter(tmp_path):
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([sim, "--duration", "2", "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    replay = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common]
    v = "1.0"
    sweep = ["--batch", "4", "--measurementNoise", v, "--sweep", "measurementNoise=" + ",".join([v] * 4), "--warmup", "10"]
    onf = subprocess.run(replay + sweep + ["--warmupOnFilter"], capture_output=True, text=True, timeout=120)
    old = subprocess.run(replay + sweep, capture_output=True, text=True, timeout=120)
    assert onf.returncode == 0 and old.returncode == 0, (onf.stderr[-2000:], old.stderr[-2000:])
    total = int(re.search(r"and (\d+) vision measurements in 4 slots", onf.stdout).group(1))
    assert total == int(re.search(r"and (\d+) vision measurements in 4 slots", old.stdout).group(1)) > 30
    m = re.search(r"warm-up: 10 frames on a single filter, then loaded into 4 slots; scores over the (\d+) frames after the warm-up", onf.stdout)
    assert m and int(m.group(1)) == total - 10, onf.stdout
    assert "in slot 0" not in onf.stdout
    assert re.search(r"warm-up: 10 frames in slot 0, then copied into 3 slots; scores over the (\d+) frames after the warm-up", old.stdout), old.stdout
    assert "single filter" not in old.stdout
    rows, rows0 = re.findall(SLOT_LINE, onf.stdout), re.findall(SLOT_LINE, old.stdout)
    assert [r[0] for r in rows] == ["0", "1", "2", "3"] and len(rows0) == 4, onf.stdout
    assert len({r[3] for r in rows}) == 1, rows  # four loads of one filter, one tuning: the same text
    assert 20 < int(rows[0][4]) <= total - 10 and rows[0][5] == "0", rows[0]  # no warm-up frame is scored
