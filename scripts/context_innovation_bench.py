#!/usr/bin/env python3
"""What EQF_OPT_INNOVATION_STATS costs a single filter's frame: frame rate with the option on against off in the SAME process and filter,
alternating chunks of frames, medians of the chunks; at 40, 200 and 500 landmarks; on quiet frames (bench.py's headline workload: hover world, outlier thresholds off,
every frame the speculative one-round-trip path) and on frames with the shipped EuRoC thresholds (bench.py's frame_mix: wave world, landmark turnover, the
device-side outlier decision). Then the new kernel's own time from eqf_last_kernel_times (option 100 = 1: event pairs around every launch).
usage: python scripts/context_innovation_bench.py [--out profiles/context_innovation_bench.json] [--chunk 200] [--runs 6]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (first: its HIP runtime, see __graft_entry__.build)

import bench
from eqvio_amd.capi import OPT_INNOVATION_STATS, OPT_TIMING, PreparedFrames, VIOFilter, load_eqf_lib
from eqvio_amd.simworld import SimWorld

WARM = 100


def workload(kind, N, n_frames):
    s = bench.eurocish_settings()
    if kind == "quiet":
        world, frames = bench.build_workload(seed=100, n_frames=n_frames, N=N)
        cap = N
    else:  # bench.frame_mix's second workload
        s.outlierThresholdAbs, s.outlierThresholdProb, s.featureRetention, s.initialPointVariance = 4.852186665580312, 0.03229809583062128, 0.18594708334486176, 129.90415638150924
        world = SimWorld(seed=321, num_points=max(2500, 6 * N), max_features=N, trajectory="wave", noise_px=0.5)
        frames = list(world.frames(n_frames))
        cap = N + 120
    ids0 = frames[0][2]
    sensor, ids, p = world.true_state(0.0, ids0)
    p = p * (1.0 + 0.05 * np.random.default_rng(7).normal(size=(len(ids), 1)))
    return world, frames, VIOFilter(s, max_landmarks=cap, device=0, sensor=sensor, ids=ids, p=p, time=0.0)


def measure(kind, N, chunk, runs, lib):
    n_frames = WARM + 2 * runs * chunk + 40
    world, frames, flt = workload(kind, N, n_frames)
    core = flt.core_handle()
    prepared = PreparedFrames(world.cam, *bench.flatten_frames(frames))
    flt.run_prepared(prepared, 0, WARM)
    lib.eqf_synchronize(core)
    rates = {0: [], 1: []}
    pos = WARM
    for r in range(runs):
        for val in ((0, 1) if r % 2 == 0 else (1, 0)):  # alternating, and the order within a pair alternates too
            lib.eqf_set_option(core, OPT_INNOVATION_STATS, val)
            lib.eqf_synchronize(core)
            t0 = time.perf_counter()
            flt.run_prepared(prepared, pos, chunk)
            lib.eqf_synchronize(core)
            rates[val].append(chunk / (time.perf_counter() - t0))
            pos += chunk
    upd, dof, nis, logdet = flt.innovation_totals()
    # the kernel's own time, and the frame's launches around it
    lib.eqf_set_option(core, OPT_INNOVATION_STATS, 1)
    lib.eqf_set_option(core, OPT_TIMING, 1)
    spans = []
    which, us = np.zeros(4096, np.int32), np.zeros(4096, np.float32)
    for k in range(30):
        flt.run_prepared(prepared, pos, 1)
        pos += 1
        cnt = lib.eqf_last_kernel_times(core, which.ctypes.data_as(C.POINTER(C.c_int)), us.ctypes.data_as(C.POINTER(C.c_float)), 4096)
        spans += [float(us[i]) for i in range(cnt) if lib.eqf_kernel_name(int(which[i])) == b"k_innovation_stats"]
    lib.eqf_set_option(core, OPT_TIMING, 0)
    landmarks = (flt.sigma_dim() - 21) // 3
    flt.close()
    off, on = float(np.median(rates[0])), float(np.median(rates[1]))
    return {"workload": kind, "N": N, "landmarks_at_end": landmarks, "chunk_frames": chunk, "runs_each": runs, "updates_per_s_off": off, "updates_per_s_on": on,
            "frame_us_off": 1e6 / off, "frame_us_on": 1e6 / on, "cost_us_per_frame": 1e6 / on - 1e6 / off, "cost_percent": 100.0 * (off / on - 1.0),
            "spread_off_percent": 100.0 * (max(rates[0]) - min(rates[0])) / off, "spread_on_percent": 100.0 * (max(rates[1]) - min(rates[1])) / on,
            "kernel_us_median": float(np.median(spans)) if spans else None, "kernel_launches_timed": len(spans), "updates_scored": upd,
            "mean_nis_per_dof": nis / dof if dof else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_innovation_bench.json"))
    ap.add_argument("--chunk", type=int, default=200)
    ap.add_argument("--runs", type=int, default=6, help="chunks per setting (at least five)")
    ap.add_argument("--sizes", default="40,200,500")
    args = ap.parse_args()
    assert args.runs >= 5
    lib = load_eqf_lib()
    rows = []
    for N in (int(v) for v in args.sizes.split(",")):
        for kind in ("quiet", "shipped thresholds"):
            row = measure(kind, N, args.chunk, args.runs, lib)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
