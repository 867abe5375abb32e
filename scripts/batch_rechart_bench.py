"""Changing the chart of slots that hold landmarks: eqf_batch_convert_chart (one launch of k_batch_rechart, nothing of Sigma over the bus) against the only
route there was before it - read the slot back (eqvio_batch_get_eqf / _get_sigma), T Sigma T^T in numpy, and a fresh slot of the new chart through
eqvio_batch_set_slot_chart + _force_eqf. B = 256 slots of maxFeatures landmarks each (InvDepth, the shipped chart), converted to Normal; one call over 1, 16 and
256 slots, the two routes alternating in one process, --reps repetitions (default five), medians; host clock around the call (every call ends synchronised).
Between repetitions, untimed, the converted slots go back to InvDepth (the device call) and the fresh slots are emptied. One JSON line per count; it also says
how far the two routes' Sigma are apart, so a wrong T in the numpy route would show.
The numpy route's T is written out here in numpy (the closed forms of the reference's coordinateSuite): the landmark block normal_M(q0) conv_ind2euc(q0), the
sensor block of the Normal chart's M. --profile makes the device calls alone, for a kernel trace of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (the HIP runtime of the torch wheel first, as bench.py)

from batch_throughput import shipped_euroc  # noqa: E402
from eqvio_amd.batch import VIOFilterBatch  # noqa: E402
from eqvio_amd.capi import COORD_INVDEPTH, COORD_NORMAL  # noqa: E402
from util import random_spd, reasonable_state  # noqa: E402

E3 = np.array([0.0, 0.0, 1.0])


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rot_from_vectors(a, b):
    """the rotation of least angle with R a = b, for unit vectors"""
    K = skew(np.cross(a, b))
    return np.eye(3) + K + K @ K / (1.0 + a @ b)


def quat_R(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def T_invdepth_to_normal(xi0, q0):
    n = 21 + 3 * len(q0)
    T = np.eye(n)
    R = quat_R(xi0[16:20]).T  # Ad(T0^-1) of the camera offset T0 = (R0, x0): T0^-1 = (R0^T, -R0^T x0)
    x = -R @ xi0[20:23]
    T[12:15, 6:9] = -skew(xi0[13:16])
    T[15:18, 6:9], T[18:21, 9:12], T[18:21, 6:9] = R, R, skew(x) @ R
    for i, p in enumerate(q0):
        r0 = np.linalg.norm(p)
        y0 = p / r0
        Rn = rot_from_vectors(y0, E3)
        Mn = np.stack([Rn[1] / r0, -Rn[0] / r0, -p / (r0 * r0)])
        Rs = rot_from_vectors(-y0, E3)
        i2e = np.stack([2.0 * r0 * Rs.T[:, 0], 2.0 * r0 * Rs.T[:, 1], -r0 * r0 * y0], axis=1)
        T[21 + 3 * i:24 + 3 * i, 21 + 3 * i:24 + 3 * i] = Mn @ i2e
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--maxFeatures", type=int, default=40)
    ap.add_argument("--counts", default="1,16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    B, N = a.slots, a.maxFeatures
    rng = np.random.default_rng(N)
    b = VIOFilterBatch(shipped_euroc(), 2 * B, 64)  # slots B .. 2 B - 1: the fresh slots of the host route
    for k in range(B):
        xi0, Xs, ids, q0, Q = reasonable_state(rng, N, id_offset=100 * k)
        b.start_slot(k, xi0, np.zeros(0, np.int32), np.zeros((0, 3)), 1.0)
        b.slot(k).force_eqf(xi0, Xs, ids, q0, Q, random_spd(rng, 21 + 3 * N))
    empty = b.slot(B).get_eqf(), b.slot(B).get_sigma()

    def device(count, chart):
        assert b.convert_chart([(k, chart) for k in range(count)]) == [0] * count

    def host(count):
        for k in range(count):
            xi0, Xs, ids, q0, Q = b.slot(k).get_eqf()
            S = b.slot(k).get_sigma()
            T = T_invdepth_to_normal(xi0, q0)
            S1 = T @ S @ T.T
            b.set_slot_chart(B + k, COORD_NORMAL)
            b.slot(B + k).force_eqf(xi0, Xs, ids, q0, Q, 0.5 * (S1 + S1.T))

    def reset(count):
        device(count, COORD_INVDEPTH)
        for k in range(count):
            b.slot(B + k).force_eqf(*empty[0], empty[1])
            b.set_slot_chart(B + k, COORD_INVDEPTH)

    device(B, COORD_NORMAL)  # warm-up: the packet buffers grow once
    device(B, COORD_INVDEPTH)
    if a.profile:
        for count in [int(c) for c in a.counts.split(",")]:
            for _ in range(a.reps):
                device(count, COORD_NORMAL)
                device(count, COORD_INVDEPTH)
        return
    for count in [int(c) for c in a.counts.split(",")]:
        dev, hst, apart = [], [], 0.0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            host(count)
            hst.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            device(count, COORD_NORMAL)
            dev.append(1e3 * (time.perf_counter() - t0))
            for k in (0, count - 1):
                Sd, Sh = b.slot(k).get_sigma(), b.slot(B + k).get_sigma()
                apart = max(apart, float(np.linalg.norm(Sd - Sh) / np.linalg.norm(Sh)))
            reset(count)
        print(json.dumps({"metric": "batch_rechart_invdepth_to_normal", "B": B, "N": N, "n": 21 + 3 * N, "slots_converted": count, "reps": a.reps,
                          "convert_chart_ms": {"median": round(float(np.median(dev)), 4), "min": round(min(dev), 4), "max": round(max(dev), 4)},
                          "host_route_ms": {"median": round(float(np.median(hst)), 3), "min": round(min(hst), 3), "max": round(max(hst), 3)},
                          "speedup": round(float(np.median(hst) / np.median(dev)), 1), "routes_apart_rel_fro": apart}), flush=True)
    b.close()


if __name__ == "__main__":
    main()
