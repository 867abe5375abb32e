"""What the host's random numbers cost an ensemble, and what the device generator (include/eqf_ensemble_random.h) costs instead: eqf_ensemble_sample from numpy's
normals against eqf_ensemble_sample_seeded, and eqf_ensemble_resample_weighted from numpy's uniforms against eqf_ensemble_resample_weighted_seeded (the caller's
weights on both sides), on InvDepth contexts of N landmarks with a planted Sigma (tests/ensemble_cases.py's). One ensemble per size, created for --maxParticles
particles and timed at --particles (default 1000) and at that largest P. The two routes alternate in one process, --reps repetitions (default five), medians
with min and max of the host clock around the calls (every call ends synchronised). sample's host route is reported twice: with numpy's generation of the n x P
normals inside the clock and without it. One JSON line per (N, P). --profile makes the seeded calls alone, for a kernel trace of its own."""
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
from util import reasonable_state  # noqa: E402


def ms(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,40,200")
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--maxParticles", type=int, default=4000, help="the capacity every ensemble is created with; timed too")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    Pmax = max(a.maxParticles, a.particles)
    for N in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        n = 21 + 3 * N
        core = EqfCore(N, COORD_INVDEPTH)
        core.set_state(*reasonable_state(rng, N))
        core.set_sigma(planted_sigma(rng, COORD_INVDEPTH, N))
        ens = ParticleEnsemble(core, Pmax, N)
        for P in sorted({a.particles, Pmax}):
            gen = np.random.default_rng([N, P])
            w = gen.uniform(0.5, 1.5, P)
            stream = iter(range(1 << 30))
            for _ in range(2):  # warm-up of both routes
                ens.sample(np.asfortranarray(gen.normal(size=(n, P))))
                ens.resample_weighted(gen.uniform(size=P), w)
                ens.sample_seeded(P, a.seed, next(stream))
                ens.resample_weighted_seeded(P, a.seed, next(stream), w)
            if a.profile:
                for _ in range(a.reps):
                    ens.sample_seeded(P, a.seed, next(stream))
                    ens.resample_weighted_seeded(P, a.seed, next(stream), w)
                continue
            t_gen, t_host, t_seeded, t_rgen, t_rhost, t_rseeded = [], [], [], [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                xi = np.asfortranarray(gen.normal(size=(n, P)))
                t1 = time.perf_counter()
                ens.sample(xi)
                t2 = time.perf_counter()
                t_gen.append(1e3 * (t1 - t0))
                t_host.append(1e3 * (t2 - t1))
                t0 = time.perf_counter()
                u = gen.uniform(size=P)
                t1 = time.perf_counter()
                ens.resample_weighted(u, w)
                t2 = time.perf_counter()
                t_rgen.append(1e3 * (t1 - t0))
                t_rhost.append(1e3 * (t2 - t1))
                t0 = time.perf_counter()
                ens.sample_seeded(P, a.seed, next(stream))
                t_seeded.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                ens.resample_weighted_seeded(P, a.seed, next(stream), w)
                t_rseeded.append(1e3 * (time.perf_counter() - t0))
            ens.stats(reset=True)
            ens.sample(xi)
            plain = ens.stats(reset=True)
            ens.sample_seeded(P, a.seed, next(stream))
            seeded = ens.stats(reset=True)
            both = [g + h for g, h in zip(t_gen, t_host)]
            rboth = [g + h for g, h in zip(t_rgen, t_rhost)]
            print(json.dumps({"metric": "ensemble_random", "N": N, "n": n, "P": P, "reps": a.reps, "xi_megabytes": round(8e-6 * n * P, 2),
                              "sample_ms": ms(t_host), "numpy_normals_ms": ms(t_gen), "sample_with_numpy_normals_ms": ms(both), "sample_seeded_ms": ms(t_seeded),
                              "seeded_over_sample": round(float(np.median(t_seeded) / np.median(t_host)), 3),
                              "seeded_over_sample_with_generation": round(float(np.median(t_seeded) / np.median(both)), 3),
                              "resample_weighted_ms": ms(t_rhost), "numpy_uniforms_ms": ms(t_rgen), "resample_weighted_seeded_ms": ms(t_rseeded),
                              "seeded_over_resample_weighted": round(float(np.median(t_rseeded) / np.median(t_rhost)), 3),
                              "seeded_over_resample_weighted_with_generation": round(float(np.median(t_rseeded) / np.median(rboth)), 3),
                              "launches_factorisations_sample": plain, "launches_factorisations_sample_seeded": seeded}), flush=True)
        ens.close()
        core.close()


if __name__ == "__main__":
    main()
