"""Aggregate vision updates/s of the filter batch (eqvio_amd.batch.VIOFilterBatch.run_prepared) over B slots, each its own simulated sequence with landmark
turnover, at maxFeatures 20 / 40 / 64 and the shipped EuRoC filter settings. One JSON line per (N, B): host clock around run_prepared, ending in a device
synchronise, after a warm-up. The sequences are prepared eqvio_frames (capi.PreparedFrames) replayed in lockstep by eqvio_batch_run_prepared: one C call for
the whole timed run, no Python per frame."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from eqvio_amd.batch import VIOFilterBatch  # noqa: E402
from eqvio_amd.capi import COORD_INVDEPTH, PreparedFrames, Settings  # noqa: E402
from eqvio_amd.simworld import SimWorld  # noqa: E402


def shipped_euroc():
    s = Settings.defaults()
    for k, v in dict(coordinateChoice=COORD_INVDEPTH, fastRiccati=1, useDiscreteInnovationLift=0, useMedianDepth=0, initialSceneDepth=4.0, initialPointVariance=0.05,
                     measurementNoise=1.5, outlierThresholdAbs=6.0, outlierThresholdProb=4.0, featureRetention=0.5).items():
        setattr(s, k, v)
    s.cameraOffset[:] = [0.5, -0.5, 0.5, -0.5, 0, 0, 0]
    return s


def prepared(world, n):
    """eqvio_frames of n frames of the world (built once, outside the timed region)"""
    fr = list(world.frames(n))
    return PreparedFrames(world.cam, np.array([len(f[0]) for f in fr], np.int32), np.concatenate([f[0] for f in fr]).reshape(-1), np.array([f[1] for f in fr]),
                          np.array([len(f[2]) for f in fr], np.int32), np.concatenate([f[2] for f in fr]).astype(np.int32), np.concatenate([f[3] for f in fr]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,40,64")
    ap.add_argument("--batches", default="1,8,32,64,128,256,512")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    s = shipped_euroc()
    for N in [int(x) for x in a.sizes.split(",")]:
        for B in [int(x) for x in a.batches.split(",")]:
            ws = [SimWorld(seed=1000 + k, num_points=1500, max_features=N, trajectory="wave" if k % 2 == 0 else "hover", noise_px=0.5) for k in range(B)]
            seqs = [prepared(w, a.warmup + a.frames) for w in ws]
            b = VIOFilterBatch(s, B, 64)
            for k, w in enumerate(ws):
                sensor, _, _ = w.true_state(0.0, np.zeros(0, np.int32))
                b.start_slot(k, sensor, np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
            b.run_prepared(seqs, 0, a.warmup)
            b.synchronize()
            t0 = time.perf_counter()
            b.run_prepared(seqs, a.warmup, a.frames)
            b.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"metric": "batch_vision_updates_per_s", "maxFeatures": N, "B": B, "frames": a.frames, "seconds": round(dt, 4),
                              "updates_per_s": round(B * a.frames / dt, 1), "step_ms": round(1e3 * dt / a.frames, 3)}), flush=True)
            b.close()


if __name__ == "__main__":
    main()
