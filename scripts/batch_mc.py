#!/usr/bin/env python3
"""Monte-Carlo throughput of the reference's main_sim study (augmentLandmarkStates before every image, computeNEES after every frame) at maxFeatures 40:
runs x frames per second, for B runs through ONE filter batch (VIOFilterBatch.run_sim: one augment, one step and one NEES launch per frame) and through B
eqvio_filter contexts on B host threads (capi.VIOFilter, the same loop per thread, as scripts/multi_filter.py runs its filters), alternating in one process.

    python scripts/batch_mc.py [--batches 1,8,64,256] [--ctx-batches 1,8,64] [--duration 3] [--reps 2] [--json out.jsonl]
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from eqvio_amd.batch import VIOFilterBatch  # noqa: E402
from eqvio_amd.capi import Settings, SimSettings, SimulationDataServer, VIOFilter  # noqa: E402

MAXF = 40


def settings():
    s = Settings.defaults()
    s.fastRiccati = 1
    return s


def sims(B, duration, fs):
    out = [SimulationDataServer(SimSettings.defaults(randomSeed=k, maxFeatures=MAXF, duration=duration), fs) for k in range(B)]
    fs.cameraOffset[:] = out[0].camera_offset()
    return out


def run_batch(B, duration):
    fs = settings()
    ss = sims(B, duration, fs)
    b = VIOFilterBatch(fs, B, MAXF)
    t0 = time.perf_counter()
    nees = b.run_sim(ss, int(np.ceil(duration * 20)) + 2)
    el = time.perf_counter() - t0
    b.close()
    return int(np.isfinite(nees).sum()), el


def one_context(sd, fs, out, k):
    """main_sim's default loop on one eqvio_filter context (VIOFilter(getInitialCondition()), augment, processVisionData, computeNEES)"""
    s0, tids, tp = sd.true_state(0.0, True)
    f = VIOFilter(fs, max_landmarks=len(tids) + MAXF, sensor=s0, ids=tids, p=tp, time=0.0)
    n = 0
    while True:
        t = sd.next_measurement_type()
        if t == SimulationDataServer.NONE:
            break
        if t == SimulationDataServer.IMU:
            f.process_imu(sd.get_imu())
            continue
        stamp, ids, y = sd.get_vision()
        _, t2, p2 = sd.true_state(stamp, True)
        f.augment_landmark_states(ids, s0, t2, p2)
        f.process_vision(stamp, sd.cam, ids, y)
        s, t3, p3 = sd.true_state(f.get_time(), False)
        f.compute_nees(s, t3, p3)
        n += 1
    f.close()
    out[k] = n


def run_contexts(B, duration):
    fs = settings()
    ss = sims(B, duration, fs)
    out = [0] * B
    ths = [threading.Thread(target=one_context, args=(ss[k], fs, out, k)) for k in range(B)]
    t0 = time.perf_counter()
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    return sum(out), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--ctx-batches", default="1,8,64")
    ap.add_argument("--duration", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (initialise torch's HIP runtime first, as bench.py does)

    run_batch(2, 0.5)  # warm up: code objects, allocations
    rows = []
    ctxb = {int(x) for x in a.ctx_batches.split(",") if x}
    for B in [int(x) for x in a.batches.split(",")]:
        for rep in range(a.reps):
            legs = [("batch", run_batch)] + ([("contexts", run_contexts)] if B in ctxb else [])
            if rep % 2:
                legs.reverse()  # alternate the order of the two legs
            for name, fn in legs:
                frames, el = fn(B, a.duration)
                row = {"path": name, "B": B, "maxFeatures": MAXF, "duration_s": a.duration, "rep": rep, "run_frames": frames, "seconds": el,
                       "run_frames_per_s": frames / el}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
