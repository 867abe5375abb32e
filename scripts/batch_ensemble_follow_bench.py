"""What bringing every slot's cloud of a filter batch back in step with its slot costs after a landmark turnover: ONE eqf_bens_follow call over all B slots
(eqvio_amd/csrc/eqf_batch_ensemble_follow.h) against the route a batch user had before it, slot by slot - eqf_bens_get the cloud over the bus, the conditional draw in
numpy, eqf_bens_set - in the same process, alternating which route goes first. Every slot holds N landmarks in the Euclidean chart with a planted Sigma
(tests/ensemble_cases.py's); before each route the slots are planted anew, the clouds drawn anew by eqf_bens_sample_seeded and ONE eqf_batch_augment call makes
the oldest landmark of every slot leave and two new ones arrive, so both routes see the same bytes.

The numpy route is the cheapest correct one for this turnover, not the general one: eqf_batch_augment leaves Sigma_AK = 0, so the draw needs no eps_K and no
solve - eps_A = chol(Sigma_AA) Xi_A around q0 with Q = identity, p = q0 + eps_A. Its normals are the rows of normals(seed, stream, n, P) the call itself uses
(tests/ensemble_random_cases.py), computed BEFORE the clock starts; the script checks that both routes leave the same ids and kept bytes and added points
within 1e-9 in the first and the last slot. Medians of --reps repetitions (default five) with min and max of the host clock around the calls; every call ends
synchronised. One JSON line per (B, P). --profile makes the new call alone, for a kernel trace of its own."""
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
from ensemble_random_cases import philox4x64_10, unit  # noqa: E402
from eqvio_amd.batch import BatchCore  # noqa: E402
from eqvio_amd.batch_ensemble import BatchEnsemble  # noqa: E402
from eqvio_amd.capi import COORD_EUCLIDEAN, Settings  # noqa: E402
from util import reasonable_state  # noqa: E402


def ms(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def normal_rows(seed, stream, lo, hi, P):
    """rows lo .. hi - 1 of normals(seed, stream, n, P): the row blocks of four that hold them, include/eqf_ensemble_random.h's counter map"""
    j0, j1 = lo // 4, (hi + 3) // 4
    j, k = np.meshgrid(np.arange(j0, j1, dtype=np.uint64), np.arange(P, dtype=np.uint64), indexing="ij")
    x = philox4x64_10(seed, stream, j, k, np.uint64(0), np.uint64(0))
    out = np.zeros((4 * (j1 - j0), P))
    for h in (0, 1):
        r, ang = np.sqrt(-2.0 * np.log(unit(x[2 * h]))), 2.0 * np.pi * unit(x[2 * h + 1])
        out[2 * h::4], out[2 * h + 1::4] = r * np.cos(ang), r * np.sin(ang)
    return out[lo - 4 * j0:hi - 4 * j0]


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
    assert 1 <= N <= 62
    s = Settings.defaults()
    s.fastRiccati = 1
    nK, n = 21 + 3 * (N - 1), 21 + 3 * (N + 1)
    for B in [int(v) for v in a.slots.split(",")]:
        core = BatchCore(s, B)
        rng = np.random.default_rng(B)
        planted = [(reasonable_state(rng, N), planted_sigma(rng, COORD_EUCLIDEAN, N)) for _ in range(B)]
        new_p = rng.uniform(-1, 1, (B, 2, 3)) * 5.0 + np.array([0, 0, 15.0])
        slots = list(range(B))
        for P in [int(v) for v in a.particles.split(",")]:
            ens = BatchEnsemble(core, P)
            xi = [normal_rows(a.seed, 500 + k, nK, n, P) for k in slots]  # the old route's normals, outside the clock

            def turnover(st):
                """the slots planted, the clouds drawn, the oldest landmark of every slot gone and two new ones there"""
                for k, (state, Sigma) in enumerate(planted):
                    core.set_slot_chart(k, COORD_EUCLIDEAN)
                    core.set_state(k, *state)
                    core.set_sigma(k, Sigma)
                assert not any(ens.sample_seeded([(k, P, a.seed, st) for k in slots]))
                ids = [planted[k][0][2] for k in slots]
                new = np.array([900001, 900002], np.int32)
                assert not any(core.augment([(k, np.concatenate([ids[k][1:], new]), new, new_p[k]) for k in slots]))

            def new_route():
                dropped, added, status = ens.follow([(k, a.seed, 500 + k) for k in slots])
                assert not any(status) and np.all(dropped == 1) and np.all(added == 2), status

            def old_route():
                for k in slots:
                    ids, sens, p = ens.get(k)
                    _, _, fids, q0, _ = core.get_state(k)
                    S = core.get_sigma(k)
                    eps = np.linalg.cholesky(S[nK:, nK:]) @ xi[k]  # Sigma_AK = 0 behind eqf_batch_augment: no eps_K, no solve
                    where = {int(g): j for j, g in enumerate(ids)}
                    out = np.empty((P, N + 1, 3))
                    for i, fid in enumerate(fids[:N - 1]):
                        out[:, i] = p[:, where[int(fid)]]
                    out[:, N - 1:] = q0[N - 1:][None] + eps.T.reshape(P, 2, 3)
                    ens.set(k, fids, sens, out)

            for st in (0, 1):
                turnover(st)
                new_route()
            if a.profile:
                for st in range(a.reps):
                    turnover(st)
                    new_route()
                ens.close()  # before its batch goes: the batch must outlive the ensemble
                continue
            turnover(0)
            old_route()
            t_new, t_old, worst, same = [], [], 0.0, True
            for rep in range(a.reps):
                res = {}
                for route in (("new", "old") if rep % 2 == 0 else ("old", "new")):
                    turnover(rep)
                    t0 = time.perf_counter()
                    new_route() if route == "new" else old_route()
                    (t_new if route == "new" else t_old).append(1e3 * (time.perf_counter() - t0))
                    res[route] = [ens.get(k) for k in (0, B - 1)]
                for (ia, sa, pa), (ib, sb, pb) in zip(res["new"], res["old"]):
                    same = same and np.array_equal(ia, ib) and sa.tobytes() == sb.tobytes() and np.ascontiguousarray(pa[:, :N - 1]).tobytes() == np.ascontiguousarray(pb[:, :N - 1]).tobytes()
                    worst = max(worst, float(np.max(np.abs(pa[:, N - 1:] - pb[:, N - 1:]) / np.maximum(1.0, np.abs(pb[:, N - 1:])))))
            turnover(0)
            ens.stats(reset=True)
            new_route()
            launches, facts = ens.stats(reset=True)
            print(json.dumps({"metric": "batch_ensemble_follow", "B": B, "N": N, "dropped": 1, "added": 2, "P": P, "reps": a.reps, "follow_ms": ms(t_new),
                              "slot_by_slot_get_numpy_set_ms": ms(t_old), "old_over_new": round(float(np.median(t_old) / np.median(t_new)), 2), "launches_new": launches,
                              "factorisations_new": facts, "cloud_MB_per_slot": round(8e-6 * (23 + 3 * N) * P, 3), "same_ids_sensor_and_kept_bytes": bool(same),
                              "added_points_worst_rel": worst}), flush=True)
            assert same and worst <= 1e-9
            ens.close()
        core.close()


if __name__ == "__main__":
    main()
