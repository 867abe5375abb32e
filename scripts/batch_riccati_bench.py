"""What the accurate Riccati mode of the filter batch and its discrete-state-matrix form cost (eqf_batch_step_accurate, eqf_batch_step_discrete,
eqvio_batch_set_slot_riccati / _set_slot_state_matrix) at B = 256, maxFeatures 40 and the shipped EuRoC settings. One JSON line per measurement; host clock around eqvio_batch_run_prepared, ending in a device synchronise, after a warm-up:
  modes     aggregate vision updates/s of a batch whose slots are all fast, all accurate, all discrete, and half fast and half accurate, in the same process,
            three runs each
  parent    (--parent-libs DIR: the libraries of the build to compare against) the fast figure of scripts/batch_throughput.py, three times in the order this, parent,
            parent, this
  nees      (--nees) one batch of 3 S slots: slots 0 .. S-1 fast, S .. 2S-1 accurate and 2S .. 3S-1 discrete over the SAME S simulator seeds
            (eqvio_batch_run_sim), the mean NEES of every run in the three columns
--profile runs the steps of one mode alone (--profile-mode accurate | discrete), a fixed number of times, for a kernel trace of its own."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from batch_throughput import prepared, shipped_euroc  # noqa: E402
from eqvio_amd.batch import RICCATI_ACCURATE, RICCATI_FAST, STATE_MATRIX_CONTINUOUS, STATE_MATRIX_DISCRETE, VIOFilterBatch  # noqa: E402
from eqvio_amd.capi import SimSettings, SimulationDataServer  # noqa: E402
from eqvio_amd.simworld import SimWorld  # noqa: E402


def set_mode(b, k, word):
    """slot k's two choices for one word: fast, accurate, or discrete (accurate with the discrete state matrix)"""
    b.set_slot_riccati(k, RICCATI_FAST if word == "fast" else RICCATI_ACCURATE)
    b.set_slot_state_matrix(k, STATE_MATRIX_DISCRETE if word == "discrete" else STATE_MATRIX_CONTINUOUS)


def modes(a, out):
    B, N = a.slots, a.maxFeatures
    s = shipped_euroc()
    ws = [SimWorld(seed=1000 + k, num_points=1500, max_features=N, trajectory="wave" if k % 2 == 0 else "hover", noise_px=0.5) for k in range(B)]
    seqs = [prepared(w, a.warmup + a.frames) for w in ws]
    layouts = {a.profile_mode: [a.profile_mode] * B} if a.profile else {"fast": ["fast"] * B, "accurate": ["accurate"] * B, "discrete": ["discrete"] * B,
                                                                        "half": ["fast" if k < B // 2 else "accurate" for k in range(B)]}
    for rep in range(1 if a.profile else 3):
        for name, layout in layouts.items():
            b = VIOFilterBatch(s, B, 64)
            for k, w in enumerate(ws):
                b.start_slot(k, w.true_state(0.0, np.zeros(0, np.int32))[0], np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
                set_mode(b, k, layout[k])
            b.run_prepared(seqs, 0, a.warmup)
            b.synchronize()
            t0 = time.perf_counter()
            b.run_prepared(seqs, a.warmup, a.frames)
            b.synchronize()
            dt = time.perf_counter() - t0
            samples = [b.last_riccati(k)[0] for k in range(B)]
            out({"metric": "batch_riccati_updates_per_s", "slots": name, "rep": rep, "maxFeatures": N, "B": B, "frames": a.frames, "seconds": round(dt, 4),
                 "updates_per_s": round(B * a.frames / dt, 1), "step_ms": round(1e3 * dt / a.frames, 3), "riccati_samples_last_frame": int(max(samples))})
            b.close()


def parent(a, out):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "batch_throughput.py"), "--sizes", str(a.maxFeatures), "--batches", str(a.slots)]
    for rep in range(3):
        for name, libs in (("this", None), ("parent", a.parent_libs), ("parent", a.parent_libs), ("this", None)):  # A B B A: neither build always runs first
            env = dict(os.environ)
            if libs:
                env["EQVIO_AMD_LIB_DIR"] = os.path.abspath(libs)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    out({"build": name, "rep": rep, **json.loads(line)})


def nees(a, out):
    S = a.seeds
    fs = shipped_euroc()
    sims = [SimulationDataServer(SimSettings.defaults(numPoints=1000, maxFeatures=a.maxFeatures, randomSeed=a.seed + k % S, duration=a.duration, trajectory="wave",
                                                      initialNoise=1, inputNoise=1, outputNoise=1), fs) for k in range(3 * S)]
    b = VIOFilterBatch(fs, 3 * S, 64)
    for k in range(S, 3 * S):
        set_mode(b, k, "accurate" if k < 2 * S else "discrete")
    vals = b.run_sim(sims, int(np.ceil(a.duration * 20.0)) + 2)
    mean = np.nanmean(vals, axis=0)
    for k in range(S):
        out({"metric": "mean_nees", "seed": a.seed + k, "frames": int(np.sum(~np.isnan(vals[:, k]))), "fast": round(float(mean[k]), 6), "accurate": round(float(mean[S + k]), 6),
             "discrete": round(float(mean[2 * S + k]), 6)})
    out({"metric": "mean_nees_over_seeds", "seeds": S, "duration": a.duration, "fast": round(float(np.mean(mean[:S])), 6), "accurate": round(float(np.mean(mean[S:2 * S])), 6),
         "discrete": round(float(np.mean(mean[2 * S:])), 6)})
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--maxFeatures", type=int, default=40)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-mode", choices=["accurate", "discrete"], default="accurate")
    ap.add_argument("--parent-libs", default=None)
    ap.add_argument("--nees", action="store_true")
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--duration", type=float, default=5.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def out(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.nees:
        return nees(a, out)
    modes(a, out)
    if a.parent_libs and not a.profile:
        parent(a, out)


if __name__ == "__main__":
    main()
