"""Forking a context and changing its chart: eqf_copy_ctx (one launch of k_ctx_copy) and eqf_convert_chart (one launch of k_ctx_rechart), nothing of Sigma over
the bus, against the only routes there were - eqf_get_state + eqf_get_sigma then eqf_set_state + eqf_set_sigma into the other context, and for the chart the
same with T Sigma T^T in numpy in between, into a fresh context of the new chart. InvDepth contexts of N landmarks (capacity N), converted to Normal (the
dearest direction: a 3 x 3 product per landmark and the dense sensor rows); the routes alternate in one process, --reps repetitions (default seven), medians
with min and max; host clock around the call (every call ends synchronised). One JSON line per size and call; it also says how far the two routes' Sigma are
apart. The numpy route's T is scripts/batch_rechart_bench.py's. --profile makes the device calls alone, for a kernel trace of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from batch_rechart_bench import T_invdepth_to_normal  # noqa: E402
from eqvio_amd.capi import COORD_INVDEPTH, COORD_NORMAL, EqfCore  # noqa: E402
from util import random_spd, reasonable_state  # noqa: E402


def ms(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40,200,500")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    for N in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        state = reasonable_state(rng, N)
        S = random_spd(rng, 21 + 3 * N)
        src, dev_dst, host_dst, host_nrm = EqfCore(N, COORD_INVDEPTH), EqfCore(N, COORD_INVDEPTH), EqfCore(N, COORD_INVDEPTH), EqfCore(N, COORD_NORMAL)
        src.set_state(*state)
        src.set_sigma(S)
        dev_dst.copy_from(src)  # warm-up
        if a.profile:
            for _ in range(a.reps):
                dev_dst.copy_from(src)
                dev_dst.convert_chart(COORD_NORMAL)
                dev_dst.convert_chart(COORD_INVDEPTH)
            continue
        t_copy, t_copy_host, t_conv, t_conv_host, apart = [], [], [], [], 0.0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            st = src.get_state()
            host_dst.set_state(*st)
            host_dst.set_sigma(src.get_sigma())
            t_copy_host.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            dev_dst.copy_from(src)
            t_copy.append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(dev_dst.get_sigma(), host_dst.get_sigma())
            t0 = time.perf_counter()
            st = src.get_state()
            T = T_invdepth_to_normal(st[0], st[3])
            S1 = T @ src.get_sigma() @ T.T
            host_nrm.set_state(*st)
            host_nrm.set_sigma(0.5 * (S1 + S1.T))
            t_conv_host.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            dev_dst.convert_chart(COORD_NORMAL)
            t_conv.append(1e3 * (time.perf_counter() - t0))
            Sd, Sh = dev_dst.get_sigma(), host_nrm.get_sigma()
            apart = max(apart, float(np.linalg.norm(Sd - Sh) / np.linalg.norm(Sh)))
            dev_dst.convert_chart(COORD_INVDEPTH)  # untimed: back to where a copy is accepted
        n = 21 + 3 * N
        print(json.dumps({"metric": "context_copy", "N": N, "n": n, "reps": a.reps, "copy_ctx_ms": ms(t_copy), "host_route_ms": ms(t_copy_host),
                          "speedup": round(float(np.median(t_copy_host) / np.median(t_copy)), 1), "sigma_bytes": 8 * n * n}), flush=True)
        print(json.dumps({"metric": "context_convert_invdepth_to_normal", "N": N, "n": n, "reps": a.reps, "convert_chart_ms": ms(t_conv), "host_route_ms": ms(t_conv_host),
                          "speedup": round(float(np.median(t_conv_host) / np.median(t_conv)), 1), "routes_apart_rel_fro": apart}), flush=True)
        for c in (src, dev_dst, host_dst, host_nrm):
            c.close()


if __name__ == "__main__":
    main()
