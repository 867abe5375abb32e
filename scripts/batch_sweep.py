"""A settings sweep on the filter batch against the same sweep without per-slot settings: V values of measurementNoise over ONE simulated sequence (one seed).
 * sweep:    `eqvio_sim --batch V --sweep measurementNoise=v0,...`: one batch of V slots, slot k with value k, the same simulator seed in every slot;
 * one-slot: V runs of `eqvio_sim --batch 1 --measurementNoise vk`, one after another over the same frames (the same seed).
Both go through eqvio_batch_run_sim (augment, step and NEES: one launch each per frame). The times are eqvio_sim's own: its clock around eqvio_batch_run_sim,
read back from the "runs x frames/s" it prints - process start, context creation and the simulators' construction are in neither figure; the first launch of
every process (code-object load) is in both, once for the sweep and V times for the one-slot runs, as a user of either would pay it. The wall time of the two
command sequences is reported next to it. --api adds the same comparison inside one warm Python process (VIOFilterBatch.run_sim), where no process or
code-object load is left in either figure. One JSON line; the mean NEES every value prints must be the same string on both sides."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(cmd):
    t0 = time.perf_counter()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    wall = time.perf_counter() - t0
    if out.returncode != 0:
        raise SystemExit("%s: exit %d\n%s" % (" ".join(cmd[:4]), out.returncode, out.stderr[-2000:]))
    rows = re.findall(r"run (\d+) seed \d+[^:]*: mean NEES (\S+) over (\d+) frames", out.stdout)
    m = re.search(r"batch of (\d+) runs: .* frames (\d+)  runs x frames/s (\S+)", out.stdout)
    runs, frames, rate = int(m.group(1)), int(m.group(2)), float(m.group(3))
    return [r[1] for r in rows], frames, runs * frames / rate, wall


def api(values, duration, seed):
    """the same comparison through VIOFilterBatch.run_sim in this process, after one warm-up sweep"""
    import torch  # noqa: F401  (the HIP runtime of the torch wheel first, as bench.py)

    from eqvio_amd.batch import VIOFilterBatch
    from eqvio_amd.capi import Settings, SimSettings, SimulationDataServer

    fs = Settings.defaults()
    fs.fastRiccati = 1
    ss = SimSettings.defaults(randomSeed=seed, duration=duration)
    fs.cameraOffset[:] = SimulationDataServer(ss, fs).camera_offset()
    max_frames = int(np.ceil(duration * ss.imageFreq)) + 2
    per = []
    for v in values:
        s = Settings.from_buffer_copy(fs)
        s.measurementNoise = float(v)
        per.append(s)

    def sweep():
        b = VIOFilterBatch(fs, len(per), int(ss.maxFeatures))
        for k, s in enumerate(per):
            b.set_slot_settings(k, s)
        sims = [SimulationDataServer(ss, fs) for _ in per]
        t0 = time.perf_counter()
        nees = b.run_sim(sims, max_frames)
        dt = time.perf_counter() - t0
        b.close()
        return nees, dt

    sweep()
    n_sweep, t_sweep = sweep()
    cols, t_one = [], 0.0
    for s in per:
        b = VIOFilterBatch(s, 1, int(ss.maxFeatures))
        sims = [SimulationDataServer(ss, fs)]
        t0 = time.perf_counter()
        cols.append(b.run_sim(sims, max_frames)[:, 0])
        t_one += time.perf_counter() - t0
        b.close()
    assert np.array_equal(n_sweep, np.stack(cols, axis=1), equal_nan=True), "the sweep's NEES differ from the one-slot batches'"
    n = len(per) * n_sweep.shape[0]
    return {"api_sweep_run_frames_per_s": round(n / t_sweep, 1), "api_one_slot_run_frames_per_s": round(n / t_one, 1), "api_ratio": round(t_one / t_sweep, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", type=int, default=64)
    ap.add_argument("--duration", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--exe", default=os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim"))
    ap.add_argument("--api", action="store_true")
    a = ap.parse_args()
    values = ["%.6g" % v for v in np.geomspace(0.02, 2.0, a.values)]
    common = ["--fastRiccati", "1", "--duration", str(a.duration), "--seed", str(a.seed)]
    run([a.exe, "--batch", "1"] + common)  # one run first: the binary and its libraries are in the page cache for both sides
    nees_sweep, frames, t_sweep, wall_sweep = run([a.exe, "--batch", str(a.values)] + common + ["--sweep", "measurementNoise=" + ",".join(values)])
    nees_one, t_one, wall_one = [], 0.0, 0.0
    for v in values:
        nees, f, t, w = run([a.exe, "--batch", "1"] + common + ["--measurementNoise", v])
        assert f == frames, (f, frames)
        nees_one += nees
        t_one += t
        wall_one += w
    assert nees_sweep == nees_one, "the sweep's mean NEES differ from the one-slot runs'"
    n = a.values * frames
    res = {"metric": "batch_sweep_run_frames_per_s", "values": a.values, "frames": frames, "sweep_s": round(t_sweep, 4), "one_slot_s": round(t_one, 4),
           "sweep_run_frames_per_s": round(n / t_sweep, 1), "one_slot_run_frames_per_s": round(n / t_one, 1), "ratio": round(t_one / t_sweep, 2),
           "sweep_wall_s": round(wall_sweep, 2), "one_slot_wall_s": round(wall_one, 2), "mean_nees_first_last": [float(nees_sweep[0]), float(nees_sweep[-1])]}
    if a.api:
        res.update(api(values, a.duration, a.seed))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
