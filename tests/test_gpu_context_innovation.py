"""Innovation statistics of the single-filter context path on the GPU (EQF_OPT_INNOVATION_STATS, eqf_last_innovation / eqf_innovation_totals, include/eqf_hip.h):
dof, NIS = yTilde^T S^-1 yTilde and log det S of a context's vision update against the CPU oracle (tests/context_innovation_cases.py;
tests/test_context_innovation_cases.py shows on the CPU that the frames are well conditioned and their references exact) on every route an update takes and at
the sizes where the factorisation changes form; that the option changes nothing else; bit reproducibility; what cancelled, failed and option-off updates leave;
capacity growth; the Python VIOFilter on a teacher-forced simulated sequence; a context against the batch slot it was loaded into."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import context_innovation_cases as cic
import context_scenarios as cs
from eqvio_amd.capi import OPT_INNOVATION_STATS, EqfCore, EqfError, VIOFilter
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from slot_settings_cases import tracking
from util import teacher_force

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = cic.TOL
EQF_E_NOT_SPD, EQF_E_UNSUPPORTED = -2, -6


def hold(name, got, ref, scale=1.0):
    """(dof, nis, logdet) of the device against the oracle's: the bounds of tests/test_gpu_batch_innovation.py, with the frame's own reference gap"""
    dof, nis, logdet = got
    _, gap_ld = cic.exact_gap(ref)
    e_nis, e_ld = abs(nis - ref.nis) / ref.nis, abs(logdet - ref.logdet)
    print(f"{name}: dof {dof} (oracle {ref.dof})  NIS {nis!r} rel err {e_nis:.2e}  log det S {logdet!r} abs err {e_ld:.2e} (reference gap {gap_ld:.2e})")
    assert dof == ref.dof, (name, dof, ref.dof)
    assert e_nis <= scale * TOL, (name, nis, ref.nis)
    assert e_ld <= scale * max(TOL * max(1.0, abs(ref.logdet)), 10 * gap_ld), (name, logdet, ref.logdet)


def bits(x):
    return np.float64(x).tobytes()


def same_bits(a, b):
    return a[0] == b[0] and bits(a[1]) == bits(b[1]) and bits(a[2]) == bits(b[2])


_device = {}


def device_run(name, stats=True):
    """cic.run_device of the frame, once per process"""
    if (name, stats) not in _device:
        sc, opts = cic.FRAME_BY_NAME[name]
        _device[(name, stats)] = cic.run_device(sc, cic.oracle_run(sc)[0], opts, stats=stats)
    return _device[(name, stats)]


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", [sc.name for sc, _ in cic.FRAMES])
def test_parity_with_the_oracle(name):
    sc, _ = cic.FRAME_BY_NAME[name]
    run, refs = cic.oracle_run(sc)
    dev = device_run(name)
    assert [r[0] for r in dev["results"]] == [1] * sc.frames  # every frame updated
    exp = sc.expected()
    forced_chain = any(o == cic.OPT_LOOKAHEAD for o, _ in cic.FRAME_BY_NAME[name][1])
    assert dev["counters"]["la"] == (0 if forced_chain else exp["la"]) and dev["counters"]["sel"] == exp["sel"], dev["counters"]  # the form the frame is here for
    for k, ref in enumerate(refs):
        hold(f"{name}[{k}]", dev["innovation"][k], ref)
    n, dof, nis, logdet = dev["totals"]
    sums = [0, 0.0, 0.0]
    for d, a, b in dev["innovation"]:
        sums = [sums[0] + d, sums[1] + a, sums[2] + b]
    assert (n, dof) == (sc.frames, sums[0]) and bits(nis) == bits(sums[1]) and bits(logdet) == bits(sums[2])
    # and the update itself is the oracle's (the context-size tests' bound), so the statistics describe the update that was applied
    assert np.linalg.norm(dev["after"][-1][2] - run.after[-1][2]) / np.linalg.norm(run.after[-1][2]) < 1e-7


# ------------------------------------------------------------------------------------------------ the option changes nothing else
def identical(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(identical(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["inn_staged_N40", "select_inv_N200_M190", "inn_update_N257"])
def test_the_option_changes_nothing_else(name):
    on, off = device_run(name), device_run(name, stats=False)
    assert identical(on["after"], off["after"])  # state, estimate, Sigma of every frame
    assert identical([list(r) for r in on["results"]], [list(r) for r in off["results"]])  # updated, the statistics, the removed indices
    assert on["counters"] == off["counters"], (on["counters"], off["counters"])
    assert off["totals"] == (0, 0, 0.0, 0.0)


def test_the_same_frame_gives_the_same_bits_in_two_fresh_contexts():
    for name in ("inn_update_N200", "select_inv_N513_M257", "inn_staged_N129", "inn_chain_N40"):
        sc, opts = cic.FRAME_BY_NAME[name]
        again = cic.run_device(sc, cic.oracle_run(sc)[0], opts)
        first = device_run(name)
        assert all(same_bits(a, b) for a, b in zip(first["innovation"], again["innovation"])), (name, first["innovation"], again["innovation"])
        assert first["totals"] == again["totals"]


# ------------------------------------------------------------------------------------------------ status rules
def fresh(sc, run, stats=True, cap=None):
    core = EqfCore(sc.N if cap is None else cap, cs.CHART_NAMES[sc.chart])
    core.set_option(OPT_INNOVATION_STATS, 1 if stats else 0)
    core.set_state(*run.state0)
    core.set_sigma(run.Sigma0)
    return core


def test_a_cancelled_tail_leaves_the_last_result_and_the_totals():
    sc, _ = cic.FRAME_BY_NAME["inn_staged_N40"]
    run, refs = cic.oracle_run(sc)
    core = fresh(sc, run)
    try:
        assert core.last_innovation() == (0, 0.0, 0.0) and core.innovation_totals() == (0, 0, 0.0, 0.0)  # never updated
        assert cic.drive_frame(core, sc, run.frames[0])[0] == 1
        last, totals = core.last_innovation(), core.innovation_totals()
        hold("frame 0", last, refs[0])
        assert totals == (1, last[0], last[1], last[2])
        # frame 1 with one planted outlier under the shipped absolute threshold: the statistics kernel cancels the speculative tail, nothing is applied
        fr = run.frames[1]
        y = fr.y.copy()
        y[2 * 7] += 30.0
        s = sc.settings()
        core.stage_measurement(fr.mid, y)
        core.propagate_fast(fr.mean, fr.total, s.input_gain_diag12(), s.state_gain_diag8(), fr.imus, fr.dts, bool(sc.vel_lift))
        before = cs.read_counters(core)
        upd, absE, _, _ = core.stats_then_update(cs.CAMERAS[sc.cam], fr.mid, y, 6.0, 1e9, s.measurementNoise**2, bool(sc.star), bool(sc.lift))
        after = cs.read_counters(core)
        assert upd == 0 and absE.max() > 6.0
        assert (after["queued"], after["cancelled"]) == (before["queued"] + 1, before["cancelled"] + 1)  # a tail was queued, and cancelled on the device
        assert same_bits(core.last_innovation(), last) and core.innovation_totals() == totals
        # an update call that applies nothing for want of landmarks (*updated == -1) leaves them as well
        upd2 = core.stats_then_update(cs.CAMERAS[sc.cam], np.array([10 ** 6], np.int32), np.array([100.0, 100.0]), 6.0, 1e9, s.measurementNoise**2, True, False)[0]
        assert upd2 == -1 and same_bits(core.last_innovation(), last) and core.innovation_totals() == totals
    finally:
        core.close()


def test_a_failed_factorisation_reports_nan_and_adds_nothing():
    sc = cic.NOT_SPD
    run, refs = cic.oracle_run(sc)
    core = fresh(sc, run)
    try:
        assert cic.drive_frame(core, sc, run.frames[0])[0] == 1  # a good update first: there is a last result and a total to keep
        good, totals = core.last_innovation(), core.innovation_totals()
        hold("good", good, refs[0])
        core.set_state(*run.state0)
        core.set_sigma(cic.not_spd_sigma(sc))
        assert core.innovation_totals() == totals  # eqf_set_state / eqf_set_sigma leave them
        with pytest.raises(EqfError) as e:
            cic.drive_frame(core, sc, run.frames[0])
        assert e.value.code == EQF_E_NOT_SPD
        dof, nis, logdet = core.last_innovation()
        assert dof == 16 and math.isnan(nis) and math.isnan(logdet)
        assert core.innovation_totals() == totals
    finally:
        core.close()


def test_option_off_is_unsupported_reset_clears_only_the_totals_and_growth_keeps_everything():
    sc, _ = cic.FRAME_BY_NAME["inn_update_N40"]
    run, refs = cic.oracle_run(sc)
    core = fresh(sc, run, cap=40)
    try:
        cic.drive_frame(core, sc, run.frames[0])
        last, totals = core.last_innovation(), core.innovation_totals()
        assert totals == (1, 80, last[1], last[2])
        # capacity growth forced by eqf_add_landmarks: option, totals and last result survive
        ids = run.state0[2]
        core.add_landmarks(np.arange(50, dtype=np.int32) + int(ids.max()) + 1, np.tile([0.3, -0.2, 4.0], (50, 1)), 0.5)
        assert core.N == 90 and core.get_option(OPT_INNOVATION_STATS) == 1
        assert same_bits(core.last_innovation(), last) and core.innovation_totals() == totals
        # ... and the grown context goes on counting: the same frame from the same state gives the same bits (the new buffers, the chain's per-panel tiles included)
        core.set_state(*run.state0)
        core.set_sigma(run.Sigma0)
        cic.drive_frame(core, sc, run.frames[0])
        assert same_bits(core.last_innovation(), last)
        assert core.innovation_totals() == (2, 160, last[1] + last[1], last[2] + last[2])
        # the reset clears only the totals
        core.reset_innovation_totals()
        assert core.innovation_totals() == (0, 0, 0.0, 0.0) and same_bits(core.last_innovation(), last)
        # an update with the option off: the getter refuses and writes nothing; the totals stand still
        core.set_option(OPT_INNOVATION_STATS, 0)
        core.set_state(*run.state0)
        core.set_sigma(run.Sigma0)
        cic.drive_frame(core, sc, run.frames[0])
        import ctypes as C

        dof, nis, logdet = C.c_int(-7), C.c_double(-7.5), C.c_double(-8.5)
        assert core.lib.eqf_last_innovation(core.h, C.byref(dof), C.byref(nis), C.byref(logdet)) == EQF_E_UNSUPPORTED
        assert (dof.value, nis.value, logdet.value) == (-7, -7.5, -8.5)
        assert core.innovation_totals() == (0, 0, 0.0, 0.0)
        # null outputs are skipped
        core.set_option(OPT_INNOVATION_STATS, 1)
        core.set_state(*run.state0)
        core.set_sigma(run.Sigma0)
        cic.drive_frame(core, sc, run.frames[0])
        assert core.lib.eqf_last_innovation(core.h, None, C.byref(nis), None) == 0 and bits(nis.value) == bits(last[1])
        assert core.lib.eqf_innovation_totals(core.h, None, None, None, C.byref(logdet)) == 0 and bits(logdet.value) == bits(last[2])
    finally:
        core.close()


def test_the_kernel_has_its_own_timing_slot():
    from eqvio_amd.capi import OPT_TIMING

    sc, _ = cic.FRAME_BY_NAME["inn_update_N40"]
    run, _ = cic.oracle_run(sc)
    core = fresh(sc, run)
    try:
        core.set_option(OPT_TIMING, 1)
        cic.drive_frame(core, sc, run.frames[0])
        times = dict(core.kernel_times())
        assert "k_innovation_stats" in times and 0 < times["k_innovation_stats"] < 1000.0, times
    finally:
        core.close()


# ------------------------------------------------------------------------------------------------ filter level
def test_filter_level_on_a_teacher_forced_sequence():
    """A simulated sequence at maxFeatures 40 through the Python VIOFilter with the shipped thresholds (frames with and without discarded landmarks), teacher forced
    against the oracle's filter: every frame's values against the oracle's, the totals the host's own running sums bit for bit. The first frame creates every
    landmark on its measurement's bearing - yTilde is rounding noise there (NIS ~ 1e-31) and has no relative bound; its dof and log det S are held - so 31 frames run."""
    s = bs.shipped_euroc()
    F = 31
    w = SimWorld(seed=100, num_points=1500, max_features=40, trajectory="wave", noise_px=2.5)
    sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
    none_i, none_p = np.zeros(0, np.int32), np.zeros((0, 3))
    flt = VIOFilter(s, max_landmarks=64, sensor=sensor, ids=none_i, p=none_p, time=0.0)
    orc = OracleFilter(s, sensor, none_i, none_p, 0.0)
    flt.set_innovation_stats(True)
    assert flt.last_innovation() == (0, 0.0, 0.0)
    sums, held, partial = [0, 0, 0.0, 0.0], 0, 0
    for f, (imus, stamp, mid, y) in enumerate(w.frames(F)):
        for u in imus:
            flt.process_imu(u)
            orc.process_imu(u)
        ref, _, _ = cic.sequence_reference(s, orc, imus, stamp, w.cam, mid, y)
        flt.process_vision(stamp, w.cam, mid, y)
        orc.process_vision(stamp, w.cam, mid, y)
        got = flt.last_innovation()
        if f == 0:
            assert got[0] == ref.dof == 2 * len(mid) and got[1] < 1e-15 and abs(got[2] - ref.logdet) <= TOL * abs(ref.logdet)
        else:
            hold(f"frame {f}", got, ref)
            held += 1
            partial += ref.dof < 2 * len(mid)
        sums = [sums[0] + 1, sums[1] + got[0], sums[2] + got[1], sums[3] + got[2]]
        teacher_force(flt, orc)  # eqf_set_state / eqf_set_sigma: the totals survive it
    assert held == 30 and partial >= 5  # frames whose outlier decision discarded landmarks are among them
    n, dof, nis, logdet = flt.innovation_totals()
    print(f"updates {n} dof {dof} mean NIS/dof {nis / dof:.4f}")
    assert (n, dof) == (sums[0], sums[1]) and bits(nis) == bits(sums[2]) and bits(logdet) == bits(sums[3])
    flt.reset_innovation_totals()
    assert flt.innovation_totals() == (0, 0, 0.0, 0.0) and flt.last_innovation()[0] > 0
    flt.close()


def test_a_context_against_the_slot_it_was_loaded_into():
    """A planted filter at N = 40 loaded into a batch slot (load_filter), the same frame stepped on both: each side is within the bounds of the same oracle, so the
    two agree within twice the bounds."""
    from eqvio_amd.batch import VIOFilterBatch

    s = bs.shipped_euroc()
    sc = bs.make(s, "ctx_slot40", 7500, 40, sigma_edit=tracking)
    flt = VIOFilter(s, max_landmarks=64, sensor=sc.state[0], ids=sc.state[2], p=np.ones((40, 3)), time=sc.t0)
    flt.force_eqf(*sc.state, sc.Sigma)
    flt.set_innovation_stats(True)
    batch = VIOFilterBatch(s, 2, 64)
    assert batch.load_filter(flt, [1]) == [0]
    for u in sc.imus:
        flt.process_imu(u)
        batch.process_imu(1, u)
    flt.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
    assert batch.process_vision([(1, sc.stamp, sc.cam, sc.mid, sc.y)])[0] == 0
    a, b = flt.last_innovation(), batch.last_innovation(1)
    import innovation_cases as ic

    ref = ic.reference(s, sc)
    print(f"context {a}  slot {b}  oracle ({ref.dof}, {ref.nis!r}, {ref.logdet!r})")
    assert a[0] == b[0] == ref.dof > 0
    assert abs(a[1] - b[1]) / ref.nis <= 2 * TOL
    assert abs(a[2] - b[2]) <= 2 * max(TOL * max(1.0, abs(ref.logdet)), 10 * cic.exact_gap(ref)[1])
    hold("context", a, ref)
    flt.close()


# ------------------------------------------------------------------------------------------------ the command lines
def test_the_tools_print_the_single_filter_score(tmp_path):
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([sim, "--duration", "2", "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--nis", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    m = re.search(r"^innovation: updates (\d+)  mean NIS/dof (\S+)  log-likelihood (\S+)$", out.stdout, re.M)
    assert m and int(m.group(1)) > 30 and math.isfinite(float(m.group(2))) and float(m.group(2)) > 0 and math.isfinite(float(m.group(3))), out.stdout[-600:]
    replay = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common]
    one = subprocess.run(replay + ["--nis"], capture_output=True, text=True, timeout=120)
    assert one.returncode == 0, one.stderr[-2000:]
    m1 = re.search(r"^single filter: frames updated (\d+)  mean NIS/dof (\S+)  log-likelihood (\S+)$", one.stdout, re.M)
    assert m1 and int(m1.group(1)) > 30, one.stdout[-600:]
    # the same replay as a one-slot batch scores the same tuning: the two lines agree to the bounds the two paths are held to (both are the oracle's to 1e-9 per frame)
    b = subprocess.run(replay + ["--batch", "1"], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-2000:]
    mb = re.search(r"^slot 0: frames updated (\d+)  failed 0  mean NIS/dof (\S+)  log-likelihood (\S+)$", b.stdout, re.M)
    assert mb, b.stdout[-600:]
    print(one.stdout.splitlines()[-1], "|", mb.group(0))
    plain = subprocess.run(replay, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "NIS" not in plain.stdout
