"""One eqf_ensemble_nees call for P particles against P calls of eqf_compute_nees on the same context: InvDepth contexts of N landmarks with a planted Sigma
(tests/ensemble_cases.py's), P particles sampled by the ensemble from the caller's normals. Both routes in one process, --reps repetitions (default five),
medians with min and max; host clock around the call (every call ends synchronised). One JSON line per size; it also says how far the two routes' values are
apart, and times sample, integrate, errors and covariance on their own. --profile makes the ensemble calls alone, for a kernel trace of its own."""
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

from ensemble_cases import planted_sigma  # noqa: E402
from eqvio_amd.capi import COORD_INVDEPTH, EqfCore  # noqa: E402
from eqvio_amd.ensemble import ParticleEnsemble  # noqa: E402
from util import random_imu, reasonable_state  # noqa: E402


def ms(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(call, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,40,200")
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    P = a.particles
    for N in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        n = 21 + 3 * N
        core = EqfCore(N, COORD_INVDEPTH)
        core.set_state(*reasonable_state(rng, N))
        core.set_sigma(planted_sigma(rng, COORD_INVDEPTH, N))
        xi, imu = rng.normal(size=(n, P)), random_imu(rng)
        ens = ParticleEnsemble(core, P, N)
        ens.sample(xi)  # warm-up
        ens.nees()
        if a.profile:
            for _ in range(a.reps):
                ens.sample(xi)
                ens.nees()
                ens.covariance()
                ens.integrate(imu, 0.01)
            continue
        t_sample = timed(lambda: ens.sample(xi), a.reps)
        ids, sens, p = ens.get()
        core.compute_nees(sens[0], ids, p[0])  # warm-up (its buffers are allocated on first use)
        t_one, t_many, apart = [], [], 0.0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            vals, _ = ens.nees()
            t_one.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            single = np.array([core.compute_nees(sens[k], ids, p[k]) for k in range(P)])
            t_many.append(1e3 * (time.perf_counter() - t0))
            apart = max(apart, float(np.max(np.abs(vals - single) / single)))
        ens.stats(reset=True)
        ens.nees()
        launches, facts = ens.stats()
        t_err = timed(ens.errors, a.reps)
        t_cov = timed(ens.covariance, a.reps)
        t_int = timed(lambda: ens.integrate(imu, 0.01), a.reps)
        print(json.dumps({"metric": "ensemble_nees", "N": N, "n": n, "P": P, "reps": a.reps, "ensemble_nees_ms": ms(t_one), "P_compute_nees_calls_ms": ms(t_many),
                          "speedup": round(float(np.median(t_many) / np.median(t_one)), 1), "routes_apart_rel": apart, "launches_per_call": launches,
                          "factorisations_per_call": facts, "sample_ms": ms(t_sample), "errors_ms": ms(t_err), "covariance_ms": ms(t_cov), "integrate_ms": ms(t_int)}), flush=True)
        ens.close()
        core.close()


if __name__ == "__main__":
    main()
