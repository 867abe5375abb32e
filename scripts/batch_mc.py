#!/usr/bin/env python3
"""Monte-Carlo throughput of the reference's main_sim study (augmentLandmarkStates before every image, computeNEES after every frame) at maxFeatures 40:
runs x frames per second, for B runs through ONE filter batch (VIOFilterBatch.run_sim: one augment, one step and one NEES launch per frame) and through B
eqvio_filter contexts on B host threads (capi.VIOFilter, the same loop per thread, as scripts/multi_filter.py runs its filters), alternating in one process.

    python scripts/batch_mc.py [--batches 1,8,64,256] [--ctx-batches 1,8,64] [--duration 3] [--reps 2] [--json out.jsonl] [--recorded] [--fetch-sweeps K] [--call-times K]

--recorded adds the recorded loop as a third leg (VIOFilterBatch.run_sim(record_dir=...): the consistency launch in place of the NEES launch, five CSV rows per
run and frame into a temporary directory); --fetch-sweeps K times the route it replaces, get_eqf + get_sigma of every slot (what one frame would add), K times
at each B after a plain run; --call-times K times one compute_nees and one consistency call over all slots, K times alternating.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
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


def run_recorded(B, duration):
    fs = settings()
    ss = sims(B, duration, fs)
    b = VIOFilterBatch(fs, B, MAXF)
    d = tempfile.mkdtemp(prefix="batch_mc_")
    try:
        t0 = time.perf_counter()
        nees = b.run_sim(ss, int(np.ceil(duration * 20)) + 2, record_dir=d)
        el = time.perf_counter() - t0
    finally:
        shutil.rmtree(d, ignore_errors=True)
    b.close()
    return int(np.isfinite(nees).sum()), el


def fetch_sweeps(B, duration, sweeps):
    """seconds per sweep of get_eqf + get_sigma over all B slots, after a plain run (the slots hold a run's landmarks)"""
    fs = settings()
    b = VIOFilterBatch(fs, B, MAXF)
    b.run_sim(sims(B, duration, fs), int(np.ceil(duration * 20)) + 2)
    out = []
    for _ in range(sweeps):
        t0 = time.perf_counter()
        for k in range(B):
            b.slot(k).get_eqf()
            b.slot(k).get_sigma()
        out.append(time.perf_counter() - t0)
    b.close()
    return out


def call_times(B, duration, reps):
    """seconds per call of compute_nees and of consistency_records over all B slots after a plain run, alternating: host clock around the whole call (packing,
    packet, launch, copy back, synchronisation), so their difference is the longer kernel plus the 1.2 MB of records in place of B doubles"""
    fs = settings()
    ss = sims(B, duration, fs)
    b = VIOFilterBatch(fs, B, MAXF)
    b.run_sim(ss, int(np.ceil(duration * 20)) + 2)
    entries = [(k, *ss[k].true_state(b.slot(k).get_time(), False)) for k in range(B)]
    out = []
    for _ in range(reps):
        row = {}
        for name, fn in (("compute_nees", b.compute_nees), ("consistency", b.consistency_records)):
            t0 = time.perf_counter()
            _, st = fn(entries)
            row[name] = time.perf_counter() - t0
            assert not np.any(st)
        out.append(row)
    b.close()
    return out


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
    ap.add_argument("--recorded", action="store_true")
    ap.add_argument("--fetch-sweeps", type=int, default=0)
    ap.add_argument("--call-times", type=int, default=0)
    a = ap.parse_args()
    import torch  # noqa: F401  (initialise torch's HIP runtime first, as bench.py does)

    run_batch(2, 0.5)  # warm up: code objects, allocations
    rows = []
    ctxb = {int(x) for x in a.ctx_batches.split(",") if x}
    for B in [int(x) for x in a.batches.split(",")]:
        for rep in range(a.reps):
            legs = [("batch", run_batch)] + ([("batch_recorded", run_recorded)] if a.recorded else []) + ([("contexts", run_contexts)] if B in ctxb else [])
            if rep % 2:
                legs.reverse()  # alternate the order of the legs
            for name, fn in legs:
                frames, el = fn(B, a.duration)
                row = {"path": name, "B": B, "maxFeatures": MAXF, "duration_s": a.duration, "rep": rep, "run_frames": frames, "seconds": el,
                       "run_frames_per_s": frames / el}
                rows.append(row)
                print(json.dumps(row), flush=True)
        if a.fetch_sweeps:
            for rep, el in enumerate(fetch_sweeps(B, min(a.duration, 1.0), a.fetch_sweeps)):
                row = {"path": "get_eqf+get_sigma per slot", "B": B, "maxFeatures": MAXF, "rep": rep, "seconds_per_sweep": el, "slots_per_s": B / el}
                rows.append(row)
                print(json.dumps(row), flush=True)
        if a.call_times:
            for rep, t in enumerate(call_times(B, min(a.duration, 1.0), a.call_times)):
                row = {"path": "one call over all slots", "B": B, "maxFeatures": MAXF, "rep": rep, "compute_nees_s": t["compute_nees"], "consistency_s": t["consistency"]}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
