"""What reading the state estimates of a filter batch costs (eqf_batch_estimates, include/eqf_batch.h) against the per-slot route it replaces, at B slots that
hold simulated landmarks. One JSON line per measurement, host clock around calls that end in a device synchronise, the routes alternating within a repetition:
  estimates_call        ONE eqvio_batch_estimates call over all B slots (one packet, one launch of k_batch_estimate, one copy back)
  state_estimate_x_B    B eqvio_batch_state_estimate calls (each: synchronise, a blocking copy of the slot's 35 landmark planes, Q^-1 q0 on the host)
  plus_get_sigma_x_B    those and B eqvio_batch_get_sigma calls (the whole Sigma of the slot: the only per-slot way to its pose covariance)
  replay_plain / replay_recorded    eqvio_batch_run_prepared without and with the four state files of every slot written (run-frames/s)
All routes go through ctypes with their buffers allocated beforehand. --profile runs the estimates call alone, a fixed number of times, for a kernel trace."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from batch_throughput import prepared, shipped_euroc  # noqa: E402
from eqvio_amd.batch import BatchEstimateRecord, VIOFilterBatch, _dp, _ip  # noqa: E402
from eqvio_amd.simworld import SimWorld  # noqa: E402


def started(s, ws):
    b = VIOFilterBatch(s, len(ws), 64)
    for k, w in enumerate(ws):
        b.start_slot(k, w.true_state(0.0, np.zeros(0, np.int32))[0], np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--maxFeatures", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=20, help="calls (or sweeps over the slots) inside one timed window")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    B, s = a.B, shipped_euroc()
    ws = [SimWorld(seed=1000 + k, num_points=1500, max_features=a.maxFeatures, trajectory="wave" if k % 2 == 0 else "hover", noise_px=0.5) for k in range(B)]
    seqs = [prepared(w, a.warmup + a.frames) for w in ws]
    b = started(s, ws)
    b.run_prepared(seqs, 0, a.warmup)
    b.synchronize()
    slots = np.arange(B, dtype=np.int32)
    rec, times, status = (BatchEstimateRecord * B)(), np.zeros(B), np.zeros(B, np.int32)
    sensor, ids, p = np.zeros(23), np.zeros(64, np.int32), np.zeros(192)
    sig = np.zeros(213 * 213)
    dims = [b.slot(k).sigma_dim() for k in range(B)]
    lib, h = b.lib, b.h

    def estimates():
        assert lib.eqvio_batch_estimates(h, B, _ip(slots), rec, _dp(times), _ip(status)) == 0

    def per_slot(with_sigma):
        for k in range(B):
            assert lib.eqvio_batch_state_estimate(h, k, _dp(sensor), _ip(ids), _dp(p), 64) >= 0
            if with_sigma:
                assert lib.eqvio_batch_get_sigma(h, k, _dp(sig), dims[k]) == 0

    common = {"B": B, "maxFeatures": a.maxFeatures, "mean_landmarks": round(float(np.mean([(d - 21) / 3 for d in dims])), 1)}
    if a.profile:
        for _ in range(a.sweeps):
            estimates()
        print(json.dumps({"path": "estimates_call (profile run)", **common, "calls": a.sweeps}), flush=True)
        return
    routes = [("estimates_call", estimates), ("state_estimate_x_B", lambda: per_slot(False)), ("plus_get_sigma_x_B", lambda: per_slot(True))]
    for _, fn in routes:  # warm every route
        fn()
    for rep in range(a.reps):
        for name, fn in routes if rep % 2 == 0 else routes[::-1]:
            b.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.sweeps):
                fn()
            dt = (time.perf_counter() - t0) / a.sweeps
            print(json.dumps({"path": name, **common, "rep": rep, "ms_per_sweep_of_B_slots": round(1e3 * dt, 4), "us_per_slot": round(1e6 * dt / B, 3)}), flush=True)
    b.close()
    out = tempfile.mkdtemp(prefix="batch_estimates_")
    try:
        for rep in range(3):
            for name in ("replay_plain", "replay_recorded") if rep % 2 == 0 else ("replay_recorded", "replay_plain"):
                bb = started(s, ws)
                bb.run_prepared(seqs, 0, a.warmup, record_dir=os.path.join(out, "warm") if name == "replay_recorded" else None)
                bb.synchronize()
                t0 = time.perf_counter()
                bb.run_prepared(seqs, a.warmup, a.frames, record_dir=os.path.join(out, "rec") if name == "replay_recorded" else None)
                bb.synchronize()
                dt = time.perf_counter() - t0
                print(json.dumps({"path": name, **common, "rep": rep, "run_frames": B * a.frames, "seconds": round(dt, 4), "run_frames_per_s": round(B * a.frames / dt, 1),
                                  "ms_per_frame_of_B_slots": round(1e3 * dt / a.frames, 3)}), flush=True)
                bb.close()
    finally:
        shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    main()
