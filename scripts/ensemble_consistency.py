"""The reference's statistical suite (test/test_FilterStatistics.cpp:98-168) at any size, entirely through the particle ensemble:
a planted filter (xi0 random, X = identity, Sigma0 = the fixture's initial covariance) of --landmarks N in --chart c, --particles P particles sampled by
eqf_ensemble_sample from numpy's normals, and the four checks - initial distribution, true input (5 steps of 0.2 s at zero velocity), random input (5 steps of
0.05 s) and output (measurement likelihood and weightedResample on the host from eqf_ensemble_get, eqf_ensemble_resample, one vision update) - each judged by the
mean of ONE eqf_ensemble_nees call. --deviceOutput runs the output check through include/eqf_ensemble_output.h instead (eqf_ensemble_likelihood in the log
domain, eqf_ensemble_resample_weighted from numpy's uniforms: no particle leaves the device); --measured M measures the first M landmarks only, on both sides
(the filter's update takes the same ids), and --measVar v sets the measurement variance of both sides: the two knobs eqf_vision_update already has. With one of
the three flags the output check also prints ess, the distinct particles, the mean NEES after resampling and the weighted mean sum_k w_k NEES_k before it.
The filter's side is the device's discrete Riccati step with zero gains, the observer step and the vision update, as in
tests/test_gpu_reference_tests.py. --deviceRandom SEED draws every per-particle random number on the device through include/eqf_ensemble_random.h, one stream
per draw, numbered from 0 in the order the script draws: the particles (eqf_ensemble_sample_seeded), the resampling uniforms (eqf_ensemble_resample_weighted_seeded;
the flag implies --deviceOutput) and, in the random-input check, an input disturbance per particle and step (eqf_ensemble_integrate_seeded with the standard
deviations sqrt(inputGain / dt) of gyr and acc - the noisy input the reference samples at :129 - against a filter whose Riccati step then carries that input gain
instead of zero). numpy keeps drawing the planted filter and the measurement noise. Prints one JSON line per check with every mean NEES seen and the reference's band (0.1 / 1.0 / 0.1 / 0.5 at N = 2, P = 1000)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from eqvio_amd.capi import Camera, EqfCore, Settings  # noqa: E402
from eqvio_amd.ensemble import ParticleEnsemble  # noqa: E402

CHARTS = {"euclid": 0, "invdepth": 1, "normal": 2}
BANDS = {"initial": 0.1, "true_input": 1.0, "random_input": 0.1, "output": 0.5}
FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375


def planted(N, chart, seed):
    rng = np.random.default_rng([seed, N, chart])
    s = Settings.defaults()
    s.coordinateChoice = chart
    s.initialPointVariance = s.initialPointDepthVariance = 0.01**2
    s.initialBiasOmegaVariance = s.initialBiasAccelVariance = 0.01**2
    s.initialVelocityVariance = 0.1**2
    s.initialPositionVariance = 0.001**2
    xi0 = np.zeros(23)
    xi0[0:6] = rng.uniform(-1, 1, 6)
    for lo in (6, 16):
        q = rng.normal(size=4)
        xi0[lo:lo + 4] = q / np.linalg.norm(q)
    xi0[10:13], xi0[13:16], xi0[20:23] = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    q0 = rng.uniform(-1, 1, (N, 3)) * 10.0
    q0[:, 2] += 20.0
    ident = np.zeros(23)
    ident[6] = ident[16] = 1.0
    core = EqfCore(max(N, 1), chart)
    core.set_state(xi0, ident, np.arange(N, dtype=np.int32), q0, np.tile(np.array([1.0, 0, 0, 0, 1.0]), (N, 1)))
    core.set_sigma(np.diag(s.initial_cov_diag(N)))
    return rng, s, core, q0


def pixels(p):
    return np.stack([FX * p[..., 0] / p[..., 2] + CX, FY * p[..., 1] / p[..., 2] + CY], axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=2)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--chart", choices=sorted(CHARTS), default="invdepth")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--checks", default="initial,true_input,random_input,output", help="which of the four checks to run")
    ap.add_argument("--deviceOutput", action="store_true", help="the output check through eqf_ensemble_likelihood / eqf_ensemble_resample_weighted")
    ap.add_argument("--deviceRandom", type=int, default=None, metavar="SEED", help="draw particles, input disturbances and resampling uniforms on the device from this seed")
    ap.add_argument("--measured", type=int, default=None, help="measure the first M landmarks only (both sides)")
    ap.add_argument("--measVar", type=float, default=None, help="measurement variance of both sides (default measurementNoise^2)")
    a = ap.parse_args()
    N, P, chart = a.landmarks, a.particles, CHARTS[a.chart]
    seeded = a.deviceRandom is not None
    a.deviceOutput = a.deviceOutput or seeded
    streams = iter(range(1 << 30))  # one stream per draw, in the order of the draws
    extended = a.deviceOutput or a.measured is not None or a.measVar is not None
    M = N if a.measured is None else max(0, min(N, a.measured))
    n = 21 + 3 * N
    for check in [c for c in ("initial", "true_input", "random_input", "output") if c in a.checks.split(",")]:
        rng, s, core, q0 = planted(N, chart, a.seed)
        ens = ParticleEnsemble(core, P, N)
        t0 = time.perf_counter()
        if seeded:
            ens.sample_seeded(P, a.deviceRandom, next(streams))
        else:
            ens.sample(rng.normal(size=(n, P)))
        means = []
        if check == "initial":
            means.append(ens.nees()[1])
        elif check in ("true_input", "random_input"):
            vel, dt = np.zeros(13), 0.2
            if check == "random_input":
                vel[1:7], dt = rng.uniform(-1, 1, 6), 0.05
            gain = np.zeros(12)  # 0 * inputGain, 0 * stateGain (:110-111, :133-134)
            if seeded and check == "random_input":
                gain[0:6] = s.input_gain_diag12()[0:6]  # the gyr and acc noise the particles are driven with; no bias walk
            for _ in range(5):
                if seeded and check == "random_input":
                    ens.integrate_seeded(vel, dt, np.sqrt(gain[0:6] / dt), a.deviceRandom, next(streams))
                else:
                    ens.integrate(vel, dt)
                core.integrate_riccati_discrete(vel, dt, gain, np.zeros(8))
                core.integrate_observer(vel[None, :], np.array([dt]), True)
                means.append(ens.nees()[1])
        elif extended:
            noise_var = s.measurementNoise**2  # the measurement is drawn as before; --measVar is what both sides believe
            var = noise_var if a.measVar is None else a.measVar
            ids = np.arange(M, dtype=np.int32)
            cam = Camera.pinhole(FX, FY, CX, CY, 752, 480)
            y = (pixels(q0) + np.sqrt(noise_var) * rng.normal(size=(N, 2)))[:M]
            u = None if seeded else rng.uniform(size=P)
            nees_before = ens.nees()[0]
            if a.deviceOutput:
                logw, w, lse, ess = ens.likelihood(cam, ids, y, var)
                idx = ens.resample_weighted_seeded(P, a.deviceRandom, next(streams)) if seeded else ens.resample_weighted(u)
            else:
                _, _, p = ens.get()
                err = (y[None, :, :] - pixels(p[:, :M])).reshape(P, -1)
                logw = -0.5 * np.einsum("ki,ki->k", err, err) / var
                w = np.exp(logw - logw.max())
                w /= w.sum()
                ess = 1.0 / np.sum(w * w)
                idx = np.minimum(np.searchsorted(np.cumsum(w), (u + np.arange(P)) / P, side="left"), P - 1).astype(np.int32)
                ens.resample(idx)
            if M > 0:
                core.vision_update(cam, ids, y.reshape(-1), var, True, False)
            means.append(ens.nees()[1])
            print(json.dumps({"check": check, "route": ("device, seeded" if seeded else "device") if a.deviceOutput else "host", "measured": M, "meas_var": var, "ess": round(float(ess), 3),
                              "distinct_particles_after_resampling": int(len(set(idx.tolist()))), "mean_nees_after_resampling": round(float(means[-1]), 6),
                              "weighted_mean_nees_before_resampling": round(float(np.sum(w * nees_before)), 6)}), flush=True)
        else:
            var = s.measurementNoise**2
            ids = np.arange(N, dtype=np.int32)
            y = pixels(q0) + np.sqrt(var) * rng.normal(size=(N, 2))  # X = identity: the estimate's points are q0
            _, _, p = ens.get()
            err = (y[None, :, :] - pixels(p)).reshape(P, -1)
            logw = -0.5 * np.einsum("ki,ki->k", err, err) / var
            w = np.exp(logw - logw.max())
            w /= w.sum()
            idx, j, total = np.zeros(P, np.int32), 0, w[0]  # weightedResample (test/testing_utilities.h:55-74)
            for k in range(P):
                thr = (rng.uniform() + k) / P
                while total < thr and j + 1 < P:
                    j += 1
                    total += w[j]
                idx[k] = j
            ens.resample(idx)
            if N > 0:
                core.vision_update(Camera.pinhole(FX, FY, CX, CY, 752, 480), ids, y.reshape(-1), var, True, False)
            means.append(ens.nees()[1])
            print(json.dumps({"check": check, "distinct_particles_after_resampling": int(len(set(idx.tolist())))}), flush=True)
        launches, facts = ens.stats()
        print(json.dumps({"check": check, "chart": a.chart, "N": N, "n": n, "P": P, "mean_nees": [round(float(m), 6) for m in means], "reference_band": BANDS[check],
                          "inside": bool(all(abs(m - 1.0) <= BANDS[check] for m in means)), "seconds": round(time.perf_counter() - t0, 3), "launches": launches,
                          "factorisations": facts}), flush=True)
        ens.close()
        core.close()


if __name__ == "__main__":
    main()
