"""Copying slot 0 of a filter batch into every other slot: eqf_batch_copy_slots (one launch of k_batch_copy, no transfer) against the host route, which reads
the slot back and forces it into each of the others (eqvio_batch_get_eqf / _get_sigma / _force_eqf). B = 256 slots, so 255 destinations, at N landmarks per
size; median of --reps calls, host clock around the call (every call ends synchronised). Two host routes: the source read once and forced 255 times, and a
read and a force per destination. One JSON line per N. The bytes of a copy are 2 * 8 * (n * n + 35 N) per destination (read and written), n = 21 + 3 N; the
rate printed is that volume over the time of the WHOLE call - packets to the device, launch, kernel, synchronisation - so it is a lower bound of the kernel's."""
import argparse
import ctypes as C
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
from util import random_spd, reasonable_state  # noqa: E402


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40,64")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    B = a.slots
    for N in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(N)
        b = VIOFilterBatch(shipped_euroc(), B, 64)
        for k in range(B):
            xi0, Xs, ids, q0, Q = reasonable_state(rng, N if k == 0 else 5, id_offset=100 * k)
            b.start_slot(k, xi0, np.zeros(0, np.int32), np.zeros((0, 3)), 1.0)
            b.slot(k).force_eqf(xi0, Xs, ids, q0, Q, random_spd(rng, 21 + 3 * len(ids)))
        n = 21 + 3 * N
        src, dst, st = (C.c_int * (B - 1))(*([0] * (B - 1))), (C.c_int * (B - 1))(*range(1, B)), (C.c_int * (B - 1))()
        core = b.core_handle()

        def device():
            assert b.elib.eqf_batch_copy_slots(core, B - 1, src, dst, st) == 0

        def host_read_once():
            s0 = b.slot(0)
            eqf, S = s0.get_eqf(), s0.get_sigma()
            for k in range(1, B):
                b.slot(k).force_eqf(*eqf, S)

        def host_pair_per_slot():
            s0 = b.slot(0)
            for k in range(1, B):
                b.slot(k).force_eqf(*s0.get_eqf(), s0.get_sigma())

        device()  # warm-up: the packet buffers grow once
        assert not any(st)
        ref = b.slot(0).get_sigma()
        assert np.array_equal(ref, b.slot(B - 1).get_sigma()) and np.array_equal(ref, b.slot(B // 2).get_sigma())
        dev = median_ms(device, a.reps)
        once = median_ms(host_read_once, a.reps)
        pair = median_ms(host_pair_per_slot, a.reps)
        moved = 2 * 8 * (n * n + 35 * N) * (B - 1)
        print(json.dumps({"metric": "batch_copy_slot0_into_all", "N": N, "n": n, "destinations": B - 1, "reps": a.reps, "bytes_read_and_written": moved,
                          "copy_slots_ms": {"median": round(dev[0], 4), "min": round(dev[1], 4), "max": round(dev[2], 4)},
                          "copy_slots_TB_per_s_of_the_call": round(moved / (dev[0] * 1e-3) / 1e12, 3),
                          "host_read_once_force_each_ms": round(once[0], 3), "host_read_and_force_each_ms": round(pair[0], 3),
                          "speedup_over_read_once": round(once[0] / dev[0], 1), "speedup_over_read_each": round(pair[0] / dev[0], 1)}), flush=True)
        b.close()


if __name__ == "__main__":
    main()
