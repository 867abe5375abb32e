"""Innovation statistics of the filter batch on the GPU (eqf_batch_last_innovation / _innovation_totals, include/eqf_batch.h): dof, NIS = yTilde^T S^-1 yTilde
and log det S of every slot's update against the slot's own CPU oracle (tests/innovation_cases.py; tests/test_batch_innovation_api.py shows on the CPU that the
frames are well conditioned and their references exact) over the sizes at which the two reductions of k_batch_frame can go wrong; dof on frames whose matched
measurement is not the measurement; what empty, failed and refused steps leave; bit identity across batches and against the calls themselves; the totals on a
teacher-forced simulated run; per-slot tunings; the two command lines."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import innovation_cases as ic
from batch_scenarios import EMPTY, UPDATED
from eqvio_amd.batch import VIOFilterBatch
from eqvio_amd.simworld import SimWorld
from oracle_binding import OracleFilter
from util import teacher_force

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
# 10 x the largest gap between the float64 reference and its 50-digit evaluation, as tests/test_batch_innovation_api.py::
# test_every_frame_is_well_conditioned_and_its_reference_exact prints it (log det S: 2.274e-13 absolute, on rank64_cap)
LOGDET_GAP = 10 * 2.274e-13


def plant(batch, k, sc):
    batch.start_slot(k, sc.state[0], np.zeros(0, np.int32), np.zeros((0, 3)), sc.t0)
    batch.slot(k).force_eqf(*sc.state, sc.Sigma)
    for u in sc.imus:
        batch.process_imu(k, u)


def step(batch, scs, slots=None):
    slots = list(range(len(scs))) if slots is None else slots
    return batch.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k, sc in zip(slots, scs)])


def hold(name, got, ref):
    """one slot's (dof, nis, logdet) against its oracle's"""
    dof, nis, logdet = got
    e_nis, e_ld = abs(nis - ref.nis) / ref.nis, abs(logdet - ref.logdet)
    print(f"{name}: dof {dof} (oracle {ref.dof})  NIS {nis!r} rel err {e_nis:.2e}  log det S {logdet!r} abs err {e_ld:.2e}")
    assert dof == ref.dof, (name, dof, ref.dof)
    assert e_nis <= TOL, (name, nis, ref.nis)
    assert e_ld <= max(TOL * max(1.0, abs(ref.logdet)), LOGDET_GAP), (name, logdet, ref.logdet)


def bits(x):
    return np.float64(x).tobytes()


def grid_step(call):
    """the size grid in one batch, one step; call: whether the new entry points are used around it"""
    s, scs = ic.grid()
    batch = VIOFilterBatch(s, len(scs), 64)
    if call:
        batch.reset_innovation_totals()
    for k, sc in enumerate(scs):
        plant(batch, k, sc)
        if call:
            assert batch.last_innovation(k) == (0, 0.0, 0.0) and batch.innovation_totals(k) == (0, 0, 0.0, 0.0)  # never stepped
    status = step(batch, scs)
    inn = [batch.last_innovation(k) for k in range(len(scs))] if call else None
    return batch, status, inn, [bs.slot_arrays(batch.slot(k)) for k in range(len(scs))], [batch.last_result(k) for k in range(len(scs))]


@pytest.fixture(scope="module")
def grid():
    return grid_step(True)


def test_size_grid_against_the_oracle(grid):
    batch, status, inn, _, results = grid
    s, scs = ic.grid()
    assert [2 * len(sc.mid) for sc in scs] == [2, 16, 62, 64, 66, 126, 128]
    for k, sc in enumerate(scs):
        assert status[k] == 0 and results[k][0] & UPDATED, (sc.name, status[k], results[k])
        hold(sc.name, inn[k], ic.reference(s, sc))
        assert batch.innovation_totals(k) == (1,) + inn[k]  # one updated step: the totals are its values, to the bit


def test_the_calls_do_not_touch_the_step(grid):
    """state, Sigma, flags and depth of every slot of the grid, bit for bit, with and without the new entry points around the step"""
    _, status, _, arrays, results = grid
    _, status0, _, arrays0, results0 = grid_step(False)
    assert np.array_equal(status, status0) and results == results0
    for k, (a, b) in enumerate(zip(arrays, arrays0)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), k


def test_both_charts_and_outputs_at_33():
    frames = ic.variants33()
    batch = VIOFilterBatch(bs.shipped_euroc(), len(frames), 64)
    for k, (s, sc) in enumerate(frames):
        batch.set_slot_settings(k, s)
        plant(batch, k, sc)
    assert np.all(step(batch, [sc for _, sc in frames]) == 0)
    got = [batch.last_innovation(k) for k in range(len(frames))]
    for k, (s, sc) in enumerate(frames):
        hold(sc.name, got[k], ic.reference(s, sc))
    assert len({g[1] for g in got}) == 4 and len({g[2] for g in got}) == 4  # chart and output both show in the score


def test_dof_follows_the_matched_measurement():
    frames = ic.dof_frames()
    batch = VIOFilterBatch(bs.shipped_euroc(), len(frames), 64)
    for k, (name, s, sc) in enumerate(frames):
        batch.set_slot_settings(k, s)
        plant(batch, k, sc)
    assert np.all(step(batch, [sc for _, _, sc in frames]) == 0)
    got = {name: batch.last_innovation(k) for k, (name, _, _) in enumerate(frames)}
    for name, s, sc in frames:
        hold(name, got[name], ic.reference(s, sc))
    assert got["rank64_cap"][0] == 2 * (64 - ic.RANK_CAP)  # 64 measured, the capped discards do not count
    assert got["turnover16"][0] == 128                     # 48 kept + 16 new features
    assert got["keep_lost_8of64"][0] == 16                 # 64 landmarks in the state, 8 measured


def test_status_table():
    """empty: 0, 0, 0; a failed update: m, NaN, NaN; neither adds to the totals; a refusal before the launch leaves the last values"""
    s, fails = bs.build_group("failures")
    good_a, not_spd, good_b, nonfinite, _ = fails
    empty = bs.make(s, "empty", 11400, 8, measured=[])
    over = bs.make(s, "over_capacity", 3200, 64, new=1, oracle="none")
    first = bs.make(s, "first", 11401, 8, sigma_edit=ic.tracking)
    second = [good_a, not_spd, good_b, nonfinite, empty, over]
    batch = VIOFilterBatch(s, len(second), 64)
    for k in range(len(second)):
        plant(batch, k, first)
    assert np.all(step(batch, [first] * len(second)) == 0)
    ref = ic.reference(s, first)
    before = [batch.last_innovation(k) for k in range(len(second))]
    for k in range(len(second)):
        hold(f"first[{k}]", before[k], ref)
        assert bits(before[k][1]) == bits(before[0][1]) and bits(before[k][2]) == bits(before[0][2])  # the same frame in every slot: the same bits
        assert batch.innovation_totals(k) == (1,) + before[k]
    for k, sc in enumerate(second):
        plant(batch, k, sc)
        assert batch.innovation_totals(k) == (1,) + before[k] and batch.last_innovation(k) == before[k]  # planting a state clears nothing
    status = step(batch, second)
    assert status.tolist() == [0, bs.EQF_E_NOT_SPD, 0, bs.EQF_E_NONFINITE, 0, bs.EQF_E_CAPACITY], status
    for k in (0, 2):
        got = batch.last_innovation(k)
        assert got[0] == 2 * len(second[k].mid) and math.isfinite(got[1]) and math.isfinite(got[2]) and batch.last_result(k)[0] & UPDATED
        n, dof, nis, logdet = batch.innovation_totals(k)
        assert (n, dof) == (2, before[k][0] + got[0]) and bits(nis) == bits(before[k][1] + got[1]) and bits(logdet) == bits(before[k][2] + got[2])
    for k in (1, 3):
        dof, nis, logdet = batch.last_innovation(k)
        assert dof == 2 * len(second[k].mid) == 128 and math.isnan(nis) and math.isnan(logdet), (k, dof, nis, logdet)
        assert not batch.last_result(k)[0] & UPDATED
        assert batch.innovation_totals(k) == (1,) + before[k]
    assert batch.last_result(4)[0] & EMPTY and batch.last_innovation(4) == (0, 0.0, 0.0)
    assert batch.innovation_totals(4) == (1,) + before[4]
    assert batch.last_innovation(5) == before[5] and batch.innovation_totals(5) == (1,) + before[5]


def test_a_slot_gives_the_same_bits_alone_and_in_a_batch_of_300():
    s, scs = ic.grid()
    sc = scs[4]  # N = 33: m = 66, both waves' second-entry lanes in use
    one = VIOFilterBatch(s, 1, 64)
    plant(one, 0, sc)
    assert step(one, [sc])[0] == 0
    alone = one.last_innovation(0)
    big = VIOFilterBatch(s, 300, 64)
    frames = [sc if k == 5 else scs[k % len(scs)] for k in range(300)]
    for k, f in enumerate(frames):
        plant(big, k, f)
    assert np.all(step(big, frames) == 0)
    got = big.last_innovation(5)
    assert got[0] == alone[0] == 66 and bits(got[1]) == bits(alone[1]) and bits(got[2]) == bits(alone[2]), (got, alone)
    first = {}
    for k, f in enumerate(frames):  # and so does every other slot against the first slot that holds the same frame
        j = first.setdefault(f.name, k)
        a, b = big.last_innovation(k), big.last_innovation(j)
        assert a[0] == b[0] and bits(a[1]) == bits(b[1]) and bits(a[2]) == bits(b[2]), (k, j)


def test_totals_are_the_sum_of_the_frames_in_order():
    """eight simulated slots, 30 frames, teacher forced: the totals are the per-frame values added in frame order, exactly; force_eqf leaves them; reset clears
    one slot and leaves its neighbours"""
    s = bs.shipped_euroc()
    B, F = 8, 30
    ws = [SimWorld(seed=100 + k, num_points=1500, max_features=40, trajectory=("wave" if k % 2 == 0 else "hover"), noise_px=2.5) for k in range(B)]
    batch = VIOFilterBatch(s, B, 64)
    orcs = {}
    for k, w in enumerate(ws):
        sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
        batch.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        orcs[k] = OracleFilter(s, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    batch.reset_innovation_totals()
    sums = [[0, 0, 0.0, 0.0] for _ in range(B)]
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
            dof, nis, logdet = batch.last_innovation(k)
            if batch.last_result(k)[0] & UPDATED:
                assert dof > 0 and dof % 2 == 0 and dof <= 2 * len(mid) and nis > 0 and math.isfinite(logdet)
                sums[k] = [sums[k][0] + 1, sums[k][1] + dof, sums[k][2] + nis, sums[k][3] + logdet]
            teacher_force(batch.slot(k), orcs[k])  # force_eqf: the totals survive it
    for k in range(B):
        n, dof, nis, logdet = batch.innovation_totals(k)
        print(f"slot {k}: updates {n} dof {dof} mean NIS/dof {nis / dof:.4f} log-likelihood {ic.log_likelihood(dof, nis, logdet):.6g}")
        assert n >= 20 and (n, dof) == (sums[k][0], sums[k][1]) and bits(nis) == bits(sums[k][2]) and bits(logdet) == bits(sums[k][3]), (k, n, dof, nis, logdet, sums[k])
    batch.reset_innovation_totals(3)
    assert batch.innovation_totals(3) == (0, 0, 0.0, 0.0)
    assert batch.last_innovation(3)[0] > 0  # the last step's values are not totals
    for k in (2, 4):
        assert batch.innovation_totals(k) == (sums[k][0], sums[k][1], sums[k][2], sums[k][3])
    batch.reset_innovation_totals()
    assert all(batch.innovation_totals(k) == (0, 0, 0.0, 0.0) for k in range(B))


def test_four_tunings_of_one_frame_in_one_step():
    base, frames = ic.noise_frames()
    batch = VIOFilterBatch(base, len(frames), 64)
    for k, (s, sc) in enumerate(frames):
        batch.set_slot_settings(k, s)
        plant(batch, k, sc)
    assert np.all(step(batch, [sc for _, sc in frames]) == 0)
    got = [batch.last_innovation(k) for k in range(len(frames))]
    for k, (s, sc) in enumerate(frames):
        hold(f"measurementNoise {s.measurementNoise}", got[k], ic.reference(s, sc))
    assert len({g[0] for g in got}) == 1 and len({g[1] for g in got}) == 4 and len({g[2] for g in got}) == 4


SLOT_LINE = r"slot (\d+)(?: (\S+)=(\S+))?: frames updated (\d+)  failed (\d+)  mean NIS/dof (\S+)  log-likelihood (\S+)"


def test_eqvio_opt_sweep_prints_one_slot_batches(tmp_path):
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    run, ds = str(tmp_path / "run"), str(tmp_path / "ds")
    common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
    out = subprocess.run([sim, "--duration", "2", "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds, *common],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    replay = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common]
    values = ["0.3", "1.0", "3.0"]
    out = subprocess.run(replay + ["--batch", "3", "--sweep", "measurementNoise=" + ",".join(values)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(SLOT_LINE, out.stdout)
    assert [r[0] for r in rows] == ["0", "1", "2"] and {r[1] for r in rows} == {"measurementNoise"} and [r[2] for r in rows] == values, out.stdout
    assert all(int(r[3]) > 30 and r[4] == "0" and math.isfinite(float(r[5])) and math.isfinite(float(r[6])) for r in rows), rows
    assert len({r[5] for r in rows}) == 3 and len({r[6] for r in rows}) == 3
    for k, v in enumerate(values):  # slot k is the one-slot batch with that value, to the printed precision
        one = subprocess.run(replay + ["--batch", "1", "--sweep", "measurementNoise=" + v], capture_output=True, text=True, timeout=120)
        assert one.returncode == 0, one.stderr[-2000:]
        r = re.findall(SLOT_LINE, one.stdout)
        assert len(r) == 1 and r[0][2:] == rows[k][2:], (k, r, rows[k])


def test_eqvio_sim_innovation_adds_its_lines_and_changes_nothing_else():
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    cmd = [exe, "--batch", "4", "--fastRiccati", "1", "--duration", "2", "--seed", "3"]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    inn = subprocess.run(cmd + ["--innovation"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and inn.returncode == 0, (plain.stderr[-1000:], inn.stderr[-1000:])
    rate = lambda t: re.sub(r"runs x frames/s \S+", "runs x frames/s *", t)  # the one number of the output that is a timing
    lines = rate(inn.stdout).splitlines()
    assert "innovation" not in plain.stdout
    assert lines[:-4] == rate(plain.stdout).splitlines()  # the new lines come behind the existing ones
    rows = [re.fullmatch(r"innovation run (\d+): updates (\d+)  mean NIS/dof (\S+)  log-likelihood (\S+)", l) for l in lines[-4:]]
    assert all(rows), lines[-4:]
    assert [r.group(1) for r in rows] == ["0", "1", "2", "3"]
    assert all(int(r.group(2)) > 30 and math.isfinite(float(r.group(3))) and float(r.group(3)) > 0 and math.isfinite(float(r.group(4))) for r in rows)
