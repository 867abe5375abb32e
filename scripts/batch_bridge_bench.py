"""What moving a filter between a context and the slots of a filter batch costs on the device (eqf_batch_load_ctx / eqf_batch_store_ctx, include/eqf_batch.h)
against the route through the host it replaces. One JSON line per measurement, host clock around calls that end synchronised, median of --reps calls after a
warm-up call of every route:
  load      a context of N landmarks into 1, 16 and 255 slots of a 256-slot batch: ONE eqf_batch_load_ctx call, against eqf_get_state + eqf_get_sigma once and
            eqf_batch_set_state + eqf_batch_set_sigma per slot
  store     one slot into a context: eqf_batch_store_ctx against eqf_batch_get_state + _get_sigma and eqf_set_state + eqf_set_sigma
  warmup    (--tool) wall time of `eqvio_opt --batch B --sweep ... --warmup F` with and without --warmupOnFilter on one simulated dataset
  step      (--throughput, with --parent-libs DIR for the build to compare against) scripts/batch_throughput.py at B = 256, maxFeatures 40, three
            alternating runs of each build
--profile runs the bridge calls alone, a fixed number of times, for a kernel trace."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from batch_throughput import shipped_euroc  # noqa: E402
from eqvio_amd.batch import VIOFilterBatch  # noqa: E402
from eqvio_amd.capi import COORD_INVDEPTH, EqfCore  # noqa: E402
from util import random_spd, reasonable_state  # noqa: E402


def stats_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median": round(float(np.median(ts)), 4), "min": round(float(min(ts)), 4), "max": round(float(max(ts)), 4)}


def bridge(a, out):
    B = a.slots
    for N in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        b = VIOFilterBatch(shipped_euroc(), B, 64)
        st = reasonable_state(rng, N)
        core, back = EqfCore(N, COORD_INVDEPTH), EqfCore(N, COORD_INVDEPTH)
        core.set_state(*st)
        core.set_sigma(random_spd(rng, 21 + 3 * N))
        bh, elib = b.core_handle(), b.elib
        for count in (1, 16, B - 1):
            slots, status = (C.c_int * count)(*range(1, count + 1)), (C.c_int * count)()

            def device():
                assert elib.eqf_batch_load_ctx(bh, core.h, count, slots, status) == 0

            def host():
                eqf, S = core.get_state(), core.get_sigma()
                for k in range(1, count + 1):
                    b.slot(k).force_eqf(*eqf, S)

            device()
            assert not any(status)
            if a.profile:
                for _ in range(a.reps):
                    device()
                continue
            host()
            d, h = stats_ms(device, a.reps), stats_ms(host, a.reps)
            out({"metric": "load_ctx_into_slots", "N": N, "n": 21 + 3 * N, "slots": count, "reps": a.reps, "load_ctx_ms": d, "host_route_ms": h,
                 "speedup": round(h["median"] / d["median"], 1)})

        def store():
            assert elib.eqf_batch_store_ctx(bh, 1, back.h) == 0

        def store_host():
            s1 = b.slot(1)
            eqf, S = s1.get_eqf(), s1.get_sigma()
            back.set_state(*eqf)
            back.set_sigma(S)

        store()
        if a.profile:
            for _ in range(a.reps):
                store()
            # k_batch_copy at the same size beside it: slot 1 into the 255 others
            src, dst, st2 = (C.c_int * (B - 1))(*([1] * (B - 1))), (C.c_int * (B - 1))(*([0] + list(range(2, B)))), (C.c_int * (B - 1))()
            for _ in range(a.reps):
                assert elib.eqf_batch_copy_slots(bh, B - 1, src, dst, st2) == 0
            out({"metric": "profile_run", "N": N, "calls_each": a.reps})
            continue
        store_host()
        d, h = stats_ms(store, a.reps), stats_ms(store_host, a.reps)
        out({"metric": "store_ctx_from_slot", "N": N, "n": 21 + 3 * N, "reps": a.reps, "store_ctx_ms": d, "host_route_ms": h, "speedup": round(h["median"] / d["median"], 1)})
        b.close()


def tool(a, out):
    sim, opt = (os.path.join(ROOT, "eqvio_amd", "lib", n) for n in ("eqvio_sim", "eqvio_opt"))
    with tempfile.TemporaryDirectory() as td:
        run, ds = os.path.join(td, "run"), os.path.join(td, "ds")
        common = ["--coordinateChoice", "InvDepth", "--fastRiccati", "1", "--initialPointVariance", "1.0", "--useMedianDepth", "0", "--initialSceneDepth", "3.0"]
        r = subprocess.run([sim, "--duration", str(a.duration), "--maxFeatures", "40", "--numWalls", "4", "--seed", "2", "--quiet", "--output", run, "--writeDataset", ds,
                            *common], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        values = ",".join(["1.0"] * a.toolB)
        cmd = [opt, "--imu", ds + "/imu.csv", "--features", run + "/features.csv", "--cameraOffset", "0.5", "-0.5", "0.5", "-0.5", "0", "0", "0", *common, "--batch",
               str(a.toolB), "--measurementNoise", "1.0", "--sweep", "measurementNoise=" + values, "--warmup", str(a.toolWarmup)]
        for rep in range(3):
            for name, extra in (("in_slot_0", []), ("on_filter", ["--warmupOnFilter"])):
                t0 = time.perf_counter()
                r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
                wall = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-2000:]
                frames = int(re.search(r"and (\d+) vision measurements", r.stdout).group(1))
                loop = float(re.search(r"Time taken: (\S+) seconds", r.stdout).group(1))
                out({"metric": "eqvio_opt_warmup", "warmup": name, "rep": rep, "B": a.toolB, "warmup_frames": a.toolWarmup, "frames": frames, "loop_seconds": round(loop, 4),
                     "process_seconds": round(wall, 3)})


def throughput(a, out):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "batch_throughput.py"), "--sizes", "40", "--batches", "256"]
    builds = [("this", None)] + ([("parent", a.parent_libs)] if a.parent_libs else [])
    for rep in range(3):
        for name, libs in builds:
            env = dict(os.environ)
            if libs:
                env["EQVIO_AMD_LIB_DIR"] = os.path.abspath(libs)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    out({"build": name, "rep": rep, **json.loads(line)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40,64")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--tool", action="store_true")
    ap.add_argument("--duration", type=float, default=12.0, help="seconds of the simulated dataset (20 frames per second)")
    ap.add_argument("--toolB", type=int, default=16)
    ap.add_argument("--toolWarmup", type=int, default=100)
    ap.add_argument("--throughput", action="store_true")
    ap.add_argument("--parent-libs", default=None)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def out(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    bridge(a, out)
    if a.tool and not a.profile:
        tool(a, out)
    if a.throughput and not a.profile:
        throughput(a, out)


if __name__ == "__main__":
    main()
