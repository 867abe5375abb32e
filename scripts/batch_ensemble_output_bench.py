"""What weighing and resampling every slot's cloud of a filter batch costs: ONE eqf_bens_likelihood call and ONE eqf_bens_resample_weighted_seeded call over
all B slots (include/eqf_batch_ensemble_output.h) against the route a batch user had before them, slot by slot - eqf_bens_get the cloud over the bus,
ParticleEnsemble.set, .likelihood, .resample_weighted_seeded, .get, eqf_bens_set - in the same process, alternating which route goes first. Before each route
the clouds are drawn anew by eqf_bens_sample_seeded with the same seed and stream, so both routes see the same bytes; the script checks that they choose the same
indices and leave the same clouds. Every slot has N landmarks, a planted Sigma (tests/ensemble_cases.py's) and a measurement of all N: the pinhole projection of
its cloud's first particle plus pixel noise. Medians of --reps repetitions (default five) with min and max of the host clock around the calls; every call ends
synchronised. One JSON line per (B, P). --profile makes the new calls alone, for a kernel trace of its own."""
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

from ensemble_cases import PINHOLE, planted_sigma  # noqa: E402
from eqvio_amd.batch import BatchCore  # noqa: E402
from eqvio_amd.batch_ensemble import BatchEnsemble  # noqa: E402
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, Camera, Settings  # noqa: E402
from eqvio_amd.ensemble import ParticleEnsemble  # noqa: E402
from util import reasonable_state  # noqa: E402


def ms(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="16,256")
    ap.add_argument("--particles", default="256,1000")
    ap.add_argument("--landmarks", type=int, default=40)
    ap.add_argument("--measVar", type=float, default=1e4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    N = a.landmarks
    s = Settings.defaults()
    s.fastRiccati = 1
    cam = Camera.pinhole(*PINHOLE, 752, 480)
    fx, fy, cx, cy = PINHOLE
    for B in [int(v) for v in a.slots.split(",")]:
        core = BatchCore(s, B)
        rng = np.random.default_rng(B)
        for k in range(B):
            chart = (COORD_EUCLIDEAN, COORD_INVDEPTH)[k % 2]
            core.set_slot_chart(k, chart)
            core.set_state(k, *reasonable_state(rng, N))
            core.set_sigma(k, planted_sigma(rng, chart, N))
        slots = list(range(B))
        for P in [int(v) for v in a.particles.split(",")]:
            ens = BatchEnsemble(core, P)
            single = ParticleEnsemble(None, P, N)

            def sample(st):
                assert not any(ens.sample_seeded([(k, P, a.seed, st) for k in slots]))

            sample(0)
            meas = []
            for k in slots:  # one measurement per slot, fixed over the repetitions
                ids, _, p = ens.get(k)
                y = np.column_stack([fx * p[0, :, 0] / p[0, :, 2] + cx, fy * p[0, :, 1] / p[0, :, 2] + cy]) + np.sqrt(a.measVar) * rng.normal(size=(N, 2))
                meas.append((ids, y))

            def new_route(st):
                _, _, _, ess, status = ens.likelihood([(k, cam, meas[k][0], meas[k][1], a.measVar) for k in slots])
                assert not any(status), status
                src, status = ens.resample_weighted_seeded([(k, P, a.seed, 1000 + st) for k in slots])
                assert not any(status), status
                return src, ess

            def old_route(st):
                out = np.zeros((B, P), np.int32)
                for k in slots:
                    single.set(*ens.get(k))
                    single.likelihood(cam, meas[k][0], meas[k][1], a.measVar)
                    out[k] = single.resample_weighted_seeded(P, a.seed, 1000 + st)
                    ens.set(k, *single.get())
                return out

            for st in (0, 1):
                sample(st)
                new_route(st)
            if a.profile:
                for st in range(a.reps):
                    sample(st)
                    new_route(st)
                ens.close()  # before its batch goes: the batch must outlive the ensemble
                continue
            sample(0)
            old_route(0)
            t_new, t_old, same_src, same_cloud = [], [], True, True
            for rep in range(a.reps):
                res = {}
                for route in (("new", "old") if rep % 2 == 0 else ("old", "new")):
                    sample(rep)
                    t0 = time.perf_counter()
                    src = new_route(rep)[0] if route == "new" else old_route(rep)
                    (t_new if route == "new" else t_old).append(1e3 * (time.perf_counter() - t0))
                    res[route] = (np.array(src[:, :P]), [ens.get(k) for k in (0, B - 1)])
                same_src = same_src and np.array_equal(res["new"][0], res["old"][0])
                same_cloud = same_cloud and all(x.tobytes() == y.tobytes() for ca, cb in zip(res["new"][1], res["old"][1]) for x, y in zip(ca, cb))
            sample(0)
            ens.stats(reset=True)
            _, ess = new_route(0)
            launches = ens.stats(reset=True)[0]
            single.set(*ens.get(0))
            single.stats(reset=True)
            single.likelihood(cam, meas[0][0], meas[0][1], a.measVar)
            single.resample_weighted_seeded(P, a.seed, 7)
            old_launches = single.stats(reset=True)[0]
            print(json.dumps({"metric": "batch_ensemble_output", "B": B, "N": N, "P": P, "meas_var": a.measVar, "reps": a.reps, "likelihood_resample_ms": ms(t_new),
                              "slot_by_slot_get_set_likelihood_resample_get_set_ms": ms(t_old), "old_over_new": round(float(np.median(t_old) / np.median(t_new)), 2),
                              "launches_new": launches, "launches_old_route": old_launches * B, "cloud_MB_per_slot": round(8e-6 * (23 + 3 * N) * P, 3),
                              "median_ess": round(float(np.median(ess)), 1), "same_indices": bool(same_src), "same_clouds_first_and_last_slot": bool(same_cloud)}), flush=True)
            assert same_src and same_cloud
            ens.close()
            single.close()
        core.close()


if __name__ == "__main__":
    main()
