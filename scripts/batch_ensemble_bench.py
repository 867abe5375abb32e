"""What judging every slot of a filter batch against a cloud of particles costs: ONE eqf_bens_nees call and ONE eqf_bens_sample_seeded call over all B slots
(include/eqf_batch_ensemble.h) against today's route, slot by slot - the slot stored into a context (eqf_batch_store_ctx), the particles set into a
ParticleEnsemble against that context and its nees(), the particles on the host at the start as that route has them - in the same process. The slots alternate
between the Euclidean and the InvDepth chart (the old route cannot take a Normal-chart slot at all), N landmarks each, a planted Sigma
(tests/ensemble_cases.py's). Medians of --reps repetitions (default five) with min and max of the host clock around the calls; every call ends synchronised.
One JSON line per (B, P). --profile makes the new calls alone, for a kernel trace of its own."""
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
from eqvio_amd.batch import BatchCore, load_batch_protos  # noqa: E402
from eqvio_amd.batch_ensemble import BatchEnsemble  # noqa: E402
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, EqfCore, Settings  # noqa: E402
from eqvio_amd.ensemble import ParticleEnsemble  # noqa: E402
from util import reasonable_state  # noqa: E402


def ms(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="16,256")
    ap.add_argument("--particles", default="256,1000")
    ap.add_argument("--landmarks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    N = a.landmarks
    elib, _ = load_batch_protos()
    s = Settings.defaults()
    s.fastRiccati = 1
    for B in [int(v) for v in a.slots.split(",")]:
        core = BatchCore(s, B)
        rng = np.random.default_rng(B)
        charts = [(COORD_EUCLIDEAN, COORD_INVDEPTH)[k % 2] for k in range(B)]
        for k in range(B):
            core.set_slot_chart(k, charts[k])
            core.set_state(k, *reasonable_state(rng, N))
            core.set_sigma(k, planted_sigma(rng, charts[k], N))
        ctx = {c: EqfCore(N, c) for c in (COORD_EUCLIDEAN, COORD_INVDEPTH)}
        for P in [int(v) for v in a.particles.split(",")]:
            ens = BatchEnsemble(core, P)
            single = {c: ParticleEnsemble(ctx[c], P, N) for c in ctx}
            slots = list(range(B))
            stream = iter(range(1 << 30))

            def sample():
                st = next(stream)
                assert not any(ens.sample_seeded([(k, P, a.seed, st) for k in slots]))

            def nees():
                vals, mean, status = ens.nees(slots)
                assert not any(status)
                return vals, mean

            def old_route(clouds):
                out = np.zeros((B, P))
                for k in slots:
                    assert elib.eqf_batch_store_ctx(core.h, k, ctx[charts[k]].h) == 0
                    single[charts[k]].set(*clouds[k])
                    out[k], _ = single[charts[k]].nees()
                return out

            for _ in range(2):
                sample()
                nees()
            if a.profile:
                for _ in range(a.reps):
                    sample()
                    nees()
                ens.close()  # before its batch goes: the batch must outlive the ensemble
                continue
            clouds = [ens.get(k) for k in slots]
            old_route(clouds)
            t_sample, t_nees, t_old = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                sample()
                t1 = time.perf_counter()
                vals, _ = nees()
                t2 = time.perf_counter()
                t_sample.append(1e3 * (t1 - t0))
                t_nees.append(1e3 * (t2 - t1))
                clouds = [ens.get(k) for k in slots]
                t0 = time.perf_counter()
                old = old_route(clouds)
                t_old.append(1e3 * (time.perf_counter() - t0))
            agree = float(np.max(np.abs(vals[:, :P] - old) / np.abs(old)))
            ens.stats(reset=True)
            sample()
            smp = ens.stats(reset=True)
            nees()
            nee = ens.stats(reset=True)
            single[COORD_INVDEPTH].stats(reset=True)
            single[COORD_INVDEPTH].nees()
            old_launches = single[COORD_INVDEPTH].stats(reset=True)[0] + 1  # ... and the store's launch
            print(json.dumps({"metric": "batch_ensemble", "B": B, "N": N, "P": P, "reps": a.reps, "nees_ms": ms(t_nees), "sample_seeded_ms": ms(t_sample),
                              "slot_by_slot_store_set_nees_ms": ms(t_old), "old_over_new_nees": round(float(np.median(t_old) / np.median(t_nees)), 2),
                              "launches_factorisations_nees": nee, "launches_factorisations_sample_seeded": smp, "launches_old_route": old_launches * B,
                              "nees_max_rel_difference_between_routes": agree}), flush=True)
            ens.close()
            for c in single:
                single[c].close()
        core.close()


if __name__ == "__main__":
    main()
