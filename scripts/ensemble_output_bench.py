"""One eqf_ensemble_likelihood + eqf_ensemble_resample_weighted against the host route of the same process (eqf_ensemble_get, the projections, the log-domain
weights and weightedResample's indices in numpy, eqf_ensemble_resample): P particles scattered 0.25 m around N landmarks 4 - 12 m in front of a pinhole camera,
M = N landmarks measured, measurement variance 4 px^2. --reps repetitions (default five) of each route, alternating, every repetition on freshly set particles
(the setting is outside the clock); medians with min and max of the host clock around the calls (every call ends synchronised). One JSON line per size, which
also says whether the two routes chose the same indices. --profile makes the device calls alone, for a kernel trace of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from eqvio_amd.capi import Camera  # noqa: E402
from eqvio_amd.ensemble import ParticleEnsemble  # noqa: E402

FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375


def ms(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def pixels(p):
    return np.stack([FX * p[..., 0] / p[..., 2] + CX, FY * p[..., 1] / p[..., 2] + CY], axis=-1)


def host_route(ens, y, var, u):
    P = len(u)
    _, _, p = ens.get()
    err = (y[None, :, :] - pixels(p)).reshape(P, -1)
    logw = -0.5 * np.einsum("ki,ki->k", err, err) / var
    w = np.exp(logw - logw.max())
    w /= w.sum()
    idx = np.minimum(np.searchsorted(np.cumsum(w), (u + np.arange(P)) / P, side="left"), P - 1).astype(np.int32)
    ens.resample(idx)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,40,200")
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    P, var = a.particles, 4.0
    cam = Camera.pinhole(FX, FY, CX, CY, 752, 480)
    for N in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        ids = np.arange(N, dtype=np.int32)
        q = np.column_stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(4, 12, N)])
        p = q[None, :, :] + 0.25 * rng.normal(size=(P, N, 3))
        sens = rng.normal(size=(P, 23))
        y = pixels(q) + np.sqrt(var) * rng.normal(size=(N, 2))
        u = rng.uniform(size=P)
        ens = ParticleEnsemble(None, P, N)
        for _ in range(2):  # warm-up of both routes
            ens.set(ids, sens, p)
            ens.likelihood(cam, ids, y, var)
            ens.resample_weighted(u)
            ens.set(ids, sens, p)
            host_route(ens, y, var, u)
        if a.profile:
            for _ in range(a.reps):
                ens.set(ids, sens, p)
                ens.likelihood(cam, ids, y, var)
                ens.resample_weighted(u)
            continue
        t_dev, t_lik, t_host, same, ess = [], [], [], True, 0.0
        for _ in range(a.reps):
            ens.set(ids, sens, p)
            t0 = time.perf_counter()
            _, _, _, ess = ens.likelihood(cam, ids, y, var)
            t1 = time.perf_counter()
            src = ens.resample_weighted(u)
            t2 = time.perf_counter()
            t_lik.append(1e3 * (t1 - t0))
            t_dev.append(1e3 * (t2 - t0))
            ens.set(ids, sens, p)
            t0 = time.perf_counter()
            idx = host_route(ens, y, var, u)
            t_host.append(1e3 * (time.perf_counter() - t0))
            same = same and bool(np.array_equal(src, idx))
        print(json.dumps({"metric": "ensemble_output", "N": N, "M": N, "P": P, "reps": a.reps, "device_route_ms": ms(t_dev), "of_which_likelihood_ms": ms(t_lik),
                          "host_route_ms": ms(t_host), "speedup": round(float(np.median(t_host) / np.median(t_dev)), 1), "same_indices": same, "ess": round(float(ess), 3)}),
              flush=True)
        ens.close()


if __name__ == "__main__":
    main()
