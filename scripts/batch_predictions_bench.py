"""What asking a filter batch for its feature predictions costs (eqvio_batch_feature_predictions -> eqf_batch_predictions, include/eqf_batch.h) against the
per-slot route it replaces, at B slots that hold simulated landmarks and the next frame's IMU samples in their buffers. One JSON line per measurement, host
clock around calls that end in a device synchronise, the routes alternating within a repetition:
  predictions_call      ONE eqvio_batch_feature_predictions call over all B slots at the next image's stamp (one packet, one launch of k_batch_predict, one copy
                        back; the host's predictState chain on the sensor states included)
  state_estimate_x_B    B eqvio_batch_state_estimate calls (each: synchronise, a blocking copy of the slot's 35 landmark planes, Q^-1 q0 on the host)
  plus_projection_x_B   those, each followed by the pinhole projection of the slot's points in numpy (what is left of the per-slot route once the points are
                        on the host; the IMU chain is not included)
All routes go through ctypes with their buffers allocated beforehand. --profile runs the predictions call alone, a fixed number of times, for a kernel trace."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from batch_throughput import shipped_euroc  # noqa: E402
from eqvio_amd.batch import BatchPredictionRecord, VIOFilterBatch, _dp, _ip  # noqa: E402
from eqvio_amd.capi import Camera, PreparedFrames  # noqa: E402
from eqvio_amd.simworld import SimWorld  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--maxFeatures", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=20, help="calls (or sweeps over the slots) inside one timed window")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    B, s = a.B, shipped_euroc()
    s.useFeaturePredictions = 1
    ws = [SimWorld(seed=1000 + k, num_points=1500, max_features=a.maxFeatures, trajectory="wave" if k % 2 == 0 else "hover", noise_px=0.5) for k in range(B)]
    frames = [list(w.frames(a.warmup + 1)) for w in ws]
    seqs = [PreparedFrames(w.cam, np.array([len(f[0]) for f in fr[:-1]], np.int32), np.concatenate([f[0] for f in fr[:-1]]).reshape(-1),
                           np.array([f[1] for f in fr[:-1]]), np.array([len(f[2]) for f in fr[:-1]], np.int32),
                           np.concatenate([f[2] for f in fr[:-1]]).astype(np.int32), np.concatenate([f[3] for f in fr[:-1]])) for w, fr in zip(ws, frames)]
    b = VIOFilterBatch(s, B, 64)
    for k, w in enumerate(ws):
        b.start_slot(k, w.true_state(0.0, np.zeros(0, np.int32))[0], np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
    b.run_prepared(seqs, 0, a.warmup)
    for k in range(B):  # the next frame's IMU samples: the state a front end asks its predictions in
        for imu in frames[k][a.warmup][0]:
            b.process_imu(k, imu)
    b.synchronize()
    slots = np.arange(B, dtype=np.int32)
    cams = (Camera * B)(*[w.cam for w in ws])
    stamps = np.array([frames[k][a.warmup][1] for k in range(B)])
    rec, status = (BatchPredictionRecord * B)(), np.zeros(B, np.int32)
    sensor, ids, p = np.zeros(23), np.zeros(64, np.int32), np.zeros(192)
    lib, h = b.lib, b.h
    cam0 = ws[0].cam

    def predictions():
        assert lib.eqvio_batch_feature_predictions(h, B, _ip(slots), cams, _dp(stamps), rec, _ip(status)) == 0

    def per_slot(project):
        for k in range(B):
            N = lib.eqvio_batch_state_estimate(h, k, _dp(sensor), _ip(ids), _dp(p), 64)
            assert N >= 0
            if project:
                q = p[: 3 * N].reshape(N, 3)
                np.stack([cam0.fx * q[:, 0] / q[:, 2] + cam0.cx, cam0.fy * q[:, 1] / q[:, 2] + cam0.cy], axis=1)

    predictions()
    assert not np.any(status)
    common = {"B": B, "maxFeatures": a.maxFeatures, "mean_landmarks": round(float(np.mean([r.N for r in rec])), 1),
              "imu_samples_per_slot": round(float(np.mean([len(frames[k][a.warmup][0]) for k in range(B)])), 1)}
    if a.profile:
        for _ in range(a.sweeps):
            predictions()
        print(json.dumps({"path": "predictions_call (profile run)", **common, "calls": a.sweeps}), flush=True)
        return
    routes = [("predictions_call", predictions), ("state_estimate_x_B", lambda: per_slot(False)), ("plus_projection_x_B", lambda: per_slot(True))]
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


if __name__ == "__main__":
    main()
