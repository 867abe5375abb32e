"""What the Normal chart costs in the filter batch (eqf_batch_set_slot_chart: k_batch_normal, k_batch_riccati_normal, k_batch_discrete_normal in front of
k_batch_frame_tail) at B = 256, maxFeatures 40 and the shipped EuRoC settings. One JSON line per measurement; host clock around eqvio_batch_run_prepared, ending in a
device synchronise, after a warm-up; the simulated sequences are built once per process:
  charts    aggregate vision updates/s of a batch whose slots are all InvDepth (the shipped chart) or all Normal, in each of the three propagation modes, in the
            same process, --reps runs each (default six), and their medians
  parent    (--parent-libs DIR: the libraries of the build to compare against) the all-InvDepth fast figure, three runs per process, in the order this, parent,
            parent, this (--parent-first: parent, this, this, parent): six runs of each build, and their medians and spreads
--profile runs every mode of one chart (--profile-chart) once, for a kernel trace of its own."""
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

from batch_riccati_bench import set_mode  # noqa: E402
from batch_throughput import prepared, shipped_euroc  # noqa: E402
from eqvio_amd.batch import VIOFilterBatch  # noqa: E402
from eqvio_amd.capi import COORD_INVDEPTH, COORD_NORMAL  # noqa: E402
from eqvio_amd.simworld import SimWorld  # noqa: E402

CHARTS = {"invdepth": COORD_INVDEPTH, "normal": COORD_NORMAL}


def timed(a, s, ws, seqs, chart, mode):
    b = VIOFilterBatch(s, a.slots, 64)
    for k, w in enumerate(ws):
        if chart != "invdepth":  # (the settings' own chart needs no call: a run against an older build's libraries makes none)
            b.set_slot_chart(k, CHARTS[chart])
        b.start_slot(k, w.true_state(0.0, np.zeros(0, np.int32))[0], np.zeros(0, np.int32), np.zeros((0, 3)), 0.0)
        if mode != "fast":
            set_mode(b, k, mode)
    b.run_prepared(seqs, 0, a.warmup)
    b.synchronize()
    t0 = time.perf_counter()
    b.run_prepared(seqs, a.warmup, a.frames)
    b.synchronize()
    dt = time.perf_counter() - t0
    b.close()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--maxFeatures", type=int, default=40)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--fast-only", action="store_true", help="the all-InvDepth fast figure alone (what --parent-libs runs in both builds)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-chart", choices=sorted(CHARTS), default="normal")
    ap.add_argument("--parent-libs", default=None)
    ap.add_argument("--parent-first", action="store_true", help="with --parent-libs: the order parent, this, this, parent")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def out(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.parent_libs:
        cmd = [sys.executable, os.path.abspath(__file__), "--fast-only", "--reps", "3", "--slots", str(a.slots), "--maxFeatures", str(a.maxFeatures), "--frames", str(a.frames)]
        rates = {"this": [], "parent": []}
        for name in (("parent", "this", "this", "parent") if a.parent_first else ("this", "parent", "parent", "this")):  # A B B A: neither build always runs first
            env = dict(os.environ)
            if name == "parent":
                env["EQVIO_AMD_LIB_DIR"] = os.path.abspath(a.parent_libs)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
            for line in r.stdout.splitlines():
                if line.startswith("{") and '"rep"' in line:
                    d = json.loads(line)
                    rates[name].append(d["updates_per_s"])
                    out({"build": name, **d})
        for name, v in rates.items():
            out({"metric": "batch_fast_invdepth_median_of_six", "build": name, "median_updates_per_s": float(np.median(v)), "min": min(v), "max": max(v)})
        return
    s = shipped_euroc()
    ws = [SimWorld(seed=1000 + k, num_points=1500, max_features=a.maxFeatures, trajectory="wave" if k % 2 == 0 else "hover", noise_px=0.5) for k in range(a.slots)]
    seqs = [prepared(w, a.warmup + a.frames) for w in ws]
    layouts = [("invdepth", "fast")] if a.fast_only else [(a.profile_chart, m) for m in ("fast", "accurate", "discrete")] if a.profile else [
        (c, m) for m in ("fast", "accurate", "discrete") for c in ("invdepth", "normal")]
    rates = {l: [] for l in layouts}
    for rep in range(1 if a.profile else a.reps):
        for chart, mode in layouts:
            dt = timed(a, s, ws, seqs, chart, mode)
            rates[(chart, mode)].append(a.slots * a.frames / dt)
            out({"metric": "batch_chart_updates_per_s", "chart": chart, "mode": mode, "rep": rep, "maxFeatures": a.maxFeatures, "B": a.slots, "frames": a.frames,
                 "seconds": round(dt, 4), "updates_per_s": round(a.slots * a.frames / dt, 1), "step_ms": round(1e3 * dt / a.frames, 3)})
    if not a.profile and not a.fast_only:
        for (chart, mode), v in rates.items():
            out({"metric": "batch_chart_median", "chart": chart, "mode": mode, "reps": len(v), "median_updates_per_s": round(float(np.median(v)), 1), "min": round(min(v), 1),
                 "max": round(max(v), 1)})


if __name__ == "__main__":
    main()
