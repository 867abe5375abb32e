"""The reference's initial-distribution and true-input checks (test/test_FilterStatistics.cpp:90-118) for a whole filter batch at once: nine slots - the
three charts times the three Riccati modes (fast, accurate, discrete state matrix) - are planted with FilterStatisticsTest's filter at N landmarks
(tests/ensemble_cases.py's StatFixture: its variances, 0 x inputGain and 0 x stateGain as the true-input check sets them, removeLostLandmarks off), ONE
eqf_bens_sample_seeded call draws P particles from every slot's Sigma, and every frame is one propagation-only step per mode (no measurement) with the true
input, ONE eqf_bens_integrate call with the same sample and ONE eqf_bens_nees call. Prints every slot's mean NEES per frame (frame 0: the initial check, band
0.1 of 1; frames 1 .. 5: the true-input check, band 1.0 of 1) and one JSON line with the worst distance from 1 per Riccati mode. The reference runs its true-input
check with the discrete state matrix; the fast and the accurate mode linearise a 0.2 s step of free fall and are reported for what they are.

--checks output runs the reference's fourth check instead (outputDistribution, :140-168; the knobs of scripts/ensemble_consistency.py --deviceOutput): after
sampling, every slot gets a measurement of its xi0's first --measured landmarks with pixel noise of variance --measVar (numpy), then ONE eqf_bens_likelihood
call, ONE eqf_bens_resample_weighted_seeded call, ONE vision step of the batch with that measurement (no IMU sample) and ONE eqf_bens_nees call. Prints ess, the
distinct particles and the mean NEES per slot (band 0.5 of 1) and one JSON line.

--checks turnover lets the clouds follow their slots' landmark turnover (eqvio_amd/csrc/eqf_batch_ensemble_follow.h): after sampling, for --rounds rounds, ONE
eqf_batch_augment call makes the oldest landmark of every slot leave and one or two new ones arrive with provided points, ONE eqf_bens_follow call brings every
cloud back in step and ONE eqf_bens_nees call judges it (band 0.1 of 1: the followed cloud is a draw from the slot's belief). A last round runs the output
check on the changed landmark set: likelihood, resample_weighted_seeded, a vision step, follow, nees (band 0.5 of 1). Prints the mean NEES per round and slot and
one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from ensemble_cases import CHART_NAMES, PINHOLE, STAT_BANDS, StatFixture  # noqa: E402
from eqvio_amd.batch import BatchCore  # noqa: E402
from eqvio_amd.batch_ensemble import BatchEnsemble  # noqa: E402
from eqvio_amd.capi import Camera  # noqa: E402

MODES = ("fast", "accurate", "discrete")


def output_check(a, f, core, ens, cam, slots, label):
    """the reference's outputDistribution for every slot: likelihood, weightedResample, the filter's vision update, mean NEES"""
    from eqvio_ref import Camera as RCam  # noqa: E402
    from ensemble_cases import R  # noqa: E402

    M = a.landmarks if a.measured is None else min(a.measured, a.landmarks)
    var = f.settings.measurementNoise**2
    rng = np.random.default_rng([a.seed, 77])
    y0 = R.measure(f.xi0, RCam(0, *PINHOLE))
    mids = np.ascontiguousarray(f.ids[:M])
    meas = [np.array([y0[int(i)] for i in mids], float).reshape(M, 2) + np.sqrt(var) * rng.normal(size=(M, 2)) for _ in slots]
    _, mean0, status = ens.nees(slots)
    assert not any(status), status
    _, w, _, ess, status = ens.likelihood([(k, cam, mids, meas[k], var) for k in slots])
    assert not any(status), status
    src, status = ens.resample_weighted_seeded([(k, a.particles, a.seed, 100 + k) for k in slots])
    assert not any(status), status
    none13, none = np.zeros((0, 13)), np.zeros(0)
    assert not any(core.step_accurate([(k, cam, none13, none, mids, meas[k]) for k in slots]))  # no IMU sample: the vision update alone, whatever the slot's Riccati mode
    _, mean, status = ens.nees(slots)
    assert not any(status), status
    distinct = [len(set(src[k, :a.particles].tolist())) for k in slots]
    for k in slots:
        print(f"{label[k]}: ess {ess[k]:.1f} distinct {distinct[k]} mean NEES before {mean0[k]:.4f} after {mean[k]:.4f}", flush=True)
    print(json.dumps({"metric": "batch_ensemble_output_consistency", "N": a.landmarks, "P": a.particles, "measured": M, "meas_var": var, "slots": label,
                      "ess": [float(v) for v in ess], "distinct": distinct, "mean_nees": [float(v) for v in mean], "worst": float(np.max(np.abs(mean - 1.0))),
                      "band": STAT_BANDS["output"], "launches_factorisations": ens.stats()}))


def turnover_check(a, f, core, ens, cam, slots, label):
    """clouds that follow their slots' landmark turnover (eqvio_amd/csrc/eqf_batch_ensemble_follow.h): every round the oldest landmark leaves every slot and one or two
    new ones arrive, then follow, then nees; the last round is an output check on the landmark set the turnover has left"""
    rng = np.random.default_rng([a.seed, 78])
    var = f.settings.measurementNoise**2
    next_id = 1000
    rows = []

    def judge(what):
        _, mean, status = ens.nees(slots)
        assert not any(status), status
        rows.append([float(v) for v in mean])
        print(f"{what}: " + "  ".join(f"{label[k]} {mean[k]:.4f}" for k in slots), flush=True)

    judge("round 0 (sampled)")
    for r in range(1, a.rounds + 1):
        entries = []
        for k in slots:
            ids = core.get_state(k)[2]
            n_new = min(1 + (r + k) % 2, 64 - max(len(ids) - 1, 0))
            new = np.arange(next_id, next_id + n_new, dtype=np.int32)
            next_id += n_new
            pts = rng.uniform(-1, 1, (n_new, 3)) * 10.0 + np.array([0, 0, 20.0])
            entries.append((k, np.concatenate([ids[1:], new]), new, pts))
        assert not any(core.augment(entries))
        assert ens.nees(slots)[2] == [-3] * len(slots)  # what every call answered before follow existed: a filter id the cloud does not hold
        dropped, added, status = ens.follow([(k, a.seed, 200 + 16 * r + k) for k in slots])
        assert not any(status), status
        sizes = [ens.size(k)[1] for k in slots]
        judge(f"round {r} (dropped {int(dropped.min())} .. {int(dropped.max())}, added {int(added.min())} .. {int(added.max())}, N = {min(sizes)} .. {max(sizes)})")
    # the output check on the changed landmark set: a measurement of every landmark the slot now holds (X is the identity: the estimate is q0)
    meas = []
    for k in slots:
        _, _, ids, q0, _ = core.get_state(k)
        y = np.stack([PINHOLE[0] * q0[:, 0] / q0[:, 2] + PINHOLE[2], PINHOLE[1] * q0[:, 1] / q0[:, 2] + PINHOLE[3]], axis=1) + np.sqrt(var) * rng.normal(size=(len(ids), 2))
        meas.append((ids, y))
    _, _, _, ess, status = ens.likelihood([(k, cam, meas[k][0], meas[k][1], var) for k in slots])
    assert not any(status), status
    src, status = ens.resample_weighted_seeded([(k, a.particles, a.seed, 100 + k) for k in slots])
    assert not any(status), status
    none13, none = np.zeros((0, 13)), np.zeros(0)
    assert not any(core.step_accurate([(k, cam, none13, none, meas[k][0], meas[k][1]) for k in slots]))
    dropped, added, status = ens.follow([(k, a.seed, 900 + k) for k in slots])
    assert not any(status), status
    _, mean, status = ens.nees(slots)
    assert not any(status), status
    distinct = [len(set(src[k, :a.particles].tolist())) for k in slots]
    for k in slots:
        print(f"{label[k]}: output round on N = {ens.size(k)[1]}: ess {ess[k]:.1f} distinct {distinct[k]} follow -{int(dropped[k])} +{int(added[k])} mean NEES {mean[k]:.4f}", flush=True)
    arr = np.array(rows)
    print(json.dumps({"metric": "batch_ensemble_turnover_consistency", "N": a.landmarks, "P": a.particles, "rounds": a.rounds, "slots": label,
                      "turnover_worst": float(np.max(np.abs(arr - 1.0))), "turnover_band": STAT_BANDS["initial"], "output_mean_nees": [float(v) for v in mean],
                      "output_worst": float(np.max(np.abs(mean - 1.0))), "output_band": STAT_BANDS["output"], "ess": [float(v) for v in ess],
                      "launches_factorisations": ens.stats()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=2)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--dt", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--checks", choices=("propagation", "output", "turnover"), default="propagation")
    ap.add_argument("--rounds", type=int, default=5, help="--checks turnover: rounds of augment, follow, nees")
    ap.add_argument("--measured", type=int, default=None, help="--checks output: measured landmarks (default: all)")
    ap.add_argument("--measVar", type=float, default=None, help="--checks output: measurement variance in px^2 (default: measurementNoise^2)")
    a = ap.parse_args()
    f = StatFixture(a.landmarks, a.particles, 1)
    s = f.settings
    if a.checks == "output" and a.measVar is not None:
        s.measurementNoise = float(np.sqrt(a.measVar))  # the filter's update and the likelihood weigh the measurement alike
    s.fastRiccati, s.removeLostLandmarks = 1, 0
    B = 9
    core = BatchCore(s, B)
    label = []
    for k in range(B):
        chart, mode = k // 3, MODES[k % 3]
        core.set_slot_chart(k, chart)
        core.set_state(k, f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
        core.set_sigma(k, f.sigma0)
        label.append(f"{CHART_NAMES[chart]}/{mode}")
    ens = BatchEnsemble(core, a.particles)
    slots = list(range(B))
    assert not any(ens.sample_seeded([(k, a.particles, a.seed, k) for k in slots]))
    cam = Camera.pinhole(*PINHOLE, 752, 480)
    vel, none_i, none_d = f.true_vel, np.zeros(0, np.int32), np.zeros(0)
    rows = []

    def judge(frame):
        _, mean, status = ens.nees(slots)
        assert not any(status), status
        rows.append([float(v) for v in mean])
        print(f"frame {frame}: " + "  ".join(f"{label[k]} {mean[k]:.4f}" for k in slots), flush=True)

    if a.checks == "output":
        output_check(a, f, core, ens, cam, slots, label)
        return
    if a.checks == "turnover":
        turnover_check(a, f, core, ens, cam, slots, label)
        return
    judge(0)
    for frame in range(1, a.frames + 1):
        for mode, step in zip(MODES, (core.step, core.step_accurate, core.step_discrete)):
            entries = [(k, cam, vel[None, :], np.array([a.dt]), none_i, none_d, vel, a.dt) for k in slots if MODES[k % 3] == mode]
            assert not any(step(entries))
        assert not any(ens.integrate([(k, vel, a.dt) for k in slots]))
        judge(frame)
    arr = np.array(rows)
    print(json.dumps({"metric": "batch_ensemble_consistency", "N": a.landmarks, "P": a.particles, "slots": label, "initial_worst": float(np.max(np.abs(arr[0] - 1.0))),
                      "initial_band": STAT_BANDS["initial"], "true_input_worst": {m: float(np.max(np.abs(arr[1:, i::3] - 1.0))) for i, m in enumerate(MODES)}, "true_input_band": STAT_BANDS["true_input"],
                      "launches_factorisations": ens.stats()}))


if __name__ == "__main__":
    main()
