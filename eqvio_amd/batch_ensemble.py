"""ctypes binding of the particle ensembles against batch slots: include/eqf_batch_ensemble.h (libeqf_hip.so).

BatchEnsemble(batch, max_particles) holds one cloud of up to max_particles hypotheses of the true state for EVERY slot of a filter batch (a BatchCore, or a
VIOFilterBatch through core_handle()), entirely on the device. One call samples a cloud from every listed slot's Sigma, one call moves every listed cloud with
its slot's IMU sample, one call returns every particle's NEES against its slot; launches and copies per call depend on neither the entries nor any P. numpy
arrays in and out; the compute calls return per-entry status codes, a failing call raises EqfError. The prototypes are declared in a list of their own
(_batch_ensemble_declared)."""
import ctypes as C

import numpy as np

from eqvio_amd.capi import EqfError, _dp, _f64, _i32, _ip, c_double_p, c_int_p, load_eqf_lib
from eqvio_amd.ensemble import _u64


class BensSampleEntry(C.Structure):
    _fields_ = [("slot", C.c_int), ("P", C.c_int), ("seed", C.c_ulonglong), ("stream", C.c_ulonglong)]


class BensIntegrateEntry(C.Structure):
    _fields_ = [("slot", C.c_int), ("imu13", c_double_p), ("dt", C.c_double), ("sigma6", c_double_p), ("seed", C.c_ulonglong), ("stream", C.c_ulonglong)]


def load_batch_ensemble_protos():
    """Declare the prototypes of include/eqf_batch_ensemble.h on libeqf_hip.so."""
    lib = load_eqf_lib()
    if getattr(lib, "_batch_ensemble_declared", None):
        return lib
    vp, P = C.c_void_p, C.POINTER
    protos = {
        "eqf_bens_create": (C.c_int, [P(vp), vp, C.c_int]),
        "eqf_bens_destroy": (None, [vp]),
        "eqf_bens_size": (C.c_int, [vp, C.c_int, c_int_p, c_int_p]),
        "eqf_bens_stats": (C.c_int, [vp, P(C.c_long), P(C.c_long), C.c_int]),
        "eqf_bens_set": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, c_int_p, c_double_p, c_double_p]),
        "eqf_bens_get": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, c_double_p, C.c_int, C.c_int]),
        "eqf_bens_sample_seeded": (C.c_int, [vp, C.c_int, P(BensSampleEntry), c_int_p]),
        "eqf_bens_integrate": (C.c_int, [vp, C.c_int, P(BensIntegrateEntry), c_int_p]),
        "eqf_bens_errors": (C.c_int, [vp, C.c_int, c_double_p]),
        "eqf_bens_nees": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, c_double_p, c_int_p]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    lib._batch_ensemble_declared = sorted(protos)
    return lib


class BatchEnsemble:
    """One eqf_bens against one filter batch. batch: a BatchCore, or a VIOFilterBatch (its eqf_batch is taken through core_handle())."""

    def __init__(self, batch, max_particles):
        self.lib = load_batch_ensemble_protos()
        self.owner = batch  # keeps the batch alive
        self.h = C.c_void_p()
        self.max_particles = int(max_particles)
        self._chk(self.lib.eqf_bens_create(C.byref(self.h), self._batch(), self.max_particles))

    def _chk(self, rc):
        if rc != 0:
            raise EqfError(rc, self.lib.eqf_error_string(rc).decode())

    def _batch(self):
        o = self.owner
        if o is None:
            return None
        return C.c_void_p(o.core_handle()) if hasattr(o, "core_handle") else o.h

    def close(self):
        if self.h:
            self.lib.eqf_bens_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self, slot):
        """(P, N) of the slot's cloud"""
        P, N = C.c_int(), C.c_int()
        self._chk(self.lib.eqf_bens_size(self.h, int(slot), C.byref(P), C.byref(N)))
        return P.value, N.value

    def set(self, slot, ids, sensor, p):
        """the slot's cloud from the host: ids[N], sensor (P, 23), p (P, N, 3)"""
        ids, sensor, p = _i32(ids), _f64(sensor).reshape(-1, 23), _f64(p)
        P, N = sensor.shape[0], len(ids)
        if p.size != 3 * N * P:
            raise ValueError(f"p holds {p.size} doubles, {3 * N * P} expected")
        self._chk(self.lib.eqf_bens_set(self.h, int(slot), P, N, _ip(ids), _dp(sensor), _dp(p)))

    def get(self, slot):
        """(ids[N], sensor (P, 23), p (P, N, 3)) of the slot's cloud"""
        P, N = self.size(slot)
        ids, sensor, p = np.zeros(N, np.int32), np.zeros((P, 23)), np.zeros((P, N, 3))
        rc = self.lib.eqf_bens_get(self.h, int(slot), _ip(ids), _dp(sensor), _dp(p), P, N)
        if rc < 0:
            self._chk(rc)
        return ids, sensor, p

    def sample_seeded(self, entries):
        """entries: list of (slot, P, seed, stream). Every listed slot's cloud becomes P particles stateGroupAction(X, stateChart^-1(L xi_k)) with Sigma_slot = L L^T
        and xi = normals(seed, stream, n, P) of include/eqf_ensemble_random.h, generated on the device. Returns the per-entry status codes."""
        n = len(entries)
        arr = (BensSampleEntry * max(n, 1))()
        for t, (slot, P, seed, stream) in enumerate(entries):
            arr[t].slot, arr[t].P, arr[t].seed, arr[t].stream = int(slot), int(P), _u64(seed), _u64(stream)
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqf_bens_sample_seeded(self.h, n, arr, _ip(status)))
        return [int(v) for v in status[:n]]

    def integrate(self, entries):
        """entries: list of (slot, imu13, dt) or (slot, imu13, dt, sigma6, seed, stream): integrateSystemFunction for every particle of every listed slot with the
        slot's own sample; with sigma6 (gyr xyz, acc xyz standard deviations) particle k's sample is disturbed by sigma6 * normals(seed, stream, 6, P)[:, k].
        Returns the per-entry status codes."""
        n = len(entries)
        arr = (BensIntegrateEntry * max(n, 1))()
        keep = []
        for t, (slot, imu, dt, *rest) in enumerate(entries):
            imu = None if imu is None else _f64(imu).reshape(-1)
            sigma6 = _f64(rest[0]).reshape(-1) if rest and rest[0] is not None else None
            if sigma6 is not None and len(sigma6) != 6:
                raise ValueError("sigma6 must hold six standard deviations")
            keep.append((imu, sigma6))
            arr[t].slot, arr[t].dt = int(slot), float(dt)
            arr[t].imu13 = None if imu is None else _dp(imu)
            arr[t].sigma6 = None if sigma6 is None else _dp(sigma6)
            arr[t].seed, arr[t].stream = (_u64(rest[1]), _u64(rest[2])) if len(rest) > 2 else (0, 0)
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqf_bens_integrate(self.h, n, arr, _ip(status)))
        return [int(v) for v in status[:n]]

    def _slot_n(self, slot):
        lib = self.lib
        lib.eqf_batch_num_landmarks.restype, lib.eqf_batch_num_landmarks.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return 21 + 3 * lib.eqf_batch_num_landmarks(self._batch(), int(slot))

    def errors(self, slot):
        """eps (n, P): computeNEES's error coordinates of every particle of the slot's cloud in the slot's chart"""
        out = np.zeros((self._slot_n(slot), self.size(slot)[0]), order="F")
        self._chk(self.lib.eqf_bens_errors(self.h, int(slot), out.ctypes.data_as(c_double_p)))
        return out

    def nees(self, slots, out=None):
        """(nees (count, max_particles), mean[count], status[count]) for the listed slots: row e holds the slot's P values, the rest of the row and the rows of
        refused entries are left as they were (NaN in a fresh array; pass `out` = (nees, mean) to see that they are not written)."""
        slots = _i32(slots)
        n = len(slots)
        if out is None:
            vals, mean = np.full((max(n, 1), self.max_particles), np.nan), np.full(max(n, 1), np.nan)
        else:
            vals, mean = out
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqf_bens_nees(self.h, n, _ip(slots), _dp(vals), _dp(mean), _ip(status)))
        return vals[:n], mean[:n], [int(v) for v in status[:n]]

    def stats(self, reset=False):
        """(kernel launches, factorisations of Sigma) since the last reset"""
        a, b = C.c_long(), C.c_long()
        self._chk(self.lib.eqf_bens_stats(self.h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value
