"""ctypes binding of the particle ensembles against batch slots: include/eqf_batch_ensemble.h (libeqf_hip.so).

BatchEnsemble(batch, max_particles) holds one cloud of up to max_particles hypotheses of the true state for EVERY slot of a filter batch (a BatchCore, or a
VIOFilterBatch through core_handle()), entirely on the device. One call samples a cloud from every listed slot's Sigma, one call moves every listed cloud with
its slot's IMU sample, one call returns every particle's NEES against its slot; launches and copies per call depend on neither the entries nor any P. numpy
arrays in and out; the compute calls return per-entry status codes, a failing call raises EqfError. The prototypes are declared in a list of their own
(_batch_ensemble_declared).

The measurement side, include/eqf_batch_ensemble_output.h - likelihood, resample_weighted_seeded, covariance per slot - is declared in a second list
(_batch_ensemble_output_declared); follow, eqvio_amd/csrc/eqf_batch_ensemble_follow.h - clouds that follow their slot's landmark turnover - in a third
(_batch_ensemble_follow_declared)."""
import ctypes as C

import numpy as np

from eqvio_amd.capi import EqfError, _dp, _f64, _i32, _ip, c_double_p, c_int_p, load_eqf_lib
from eqvio_amd.ensemble import _u64


class BensSampleEntry(C.Structure):
    _fields_ = [("slot", C.c_int), ("P", C.c_int), ("seed", C.c_ulonglong), ("stream", C.c_ulonglong)]


class BensIntegrateEntry(C.Structure):
    _fields_ = [("slot", C.c_int), ("imu13", c_double_p), ("dt", C.c_double), ("sigma6", c_double_p), ("seed", C.c_ulonglong), ("stream", C.c_ulonglong)]


class BensLikelihoodEntry(C.Structure):
    _fields_ = [("slot", C.c_int), ("cam", C.c_void_p), ("ids", c_int_p), ("y", c_double_p), ("M", C.c_int), ("meas_var", C.c_double)]


class BensResampleEntry(C.Structure):
    _fields_ = [("slot", C.c_int), ("P_new", C.c_int), ("seed", C.c_ulonglong), ("stream", C.c_ulonglong)]


class BensFollowEntry(C.Structure):
    _fields_ = [("slot", C.c_int), ("seed", C.c_ulonglong), ("stream", C.c_ulonglong)]


NMAX = 213  # 21 + 3 * 64: eqf_bens_covariance's block per entry is NMAX * NMAX doubles


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
    output_protos = {
        "eqf_bens_likelihood": (C.c_int, [vp, C.c_int, P(BensLikelihoodEntry), c_double_p, c_double_p, c_double_p, c_double_p, c_int_p]),
        "eqf_bens_resample_weighted_seeded": (C.c_int, [vp, C.c_int, P(BensResampleEntry), c_int_p, c_int_p]),
        "eqf_bens_covariance": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, c_int_p]),
    }
    for name, (res, args) in output_protos.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    lib._batch_ensemble_output_declared = sorted(output_protos)
    follow_protos = {"eqf_bens_follow": (C.c_int, [vp, C.c_int, P(BensFollowEntry), c_int_p, c_int_p, c_int_p])}
    for name, (res, args) in follow_protos.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    lib._batch_ensemble_follow_declared = sorted(follow_protos)
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

    def likelihood(self, entries, out=None):
        """entries: list of (slot, cam, ids, y, meas_var) - one measurement per slot: cam a capi.Camera, ids[M] the measured landmark ids (matched by id to the
        cloud's), y (M, 2). Returns (loglik (count, max_particles), weights (count, max_particles), logsumexp[count], ess[count], status[count]): row e holds the
        slot's P values, the rest of the row and everything of a refused entry are left as they were (NaN in fresh arrays; pass `out` = (loglik, weights,
        logsumexp, ess) to see that they are not written). The normalised weights are kept per slot on the device for resample_weighted_seeded."""
        n = len(entries)
        arr = (BensLikelihoodEntry * max(n, 1))()
        keep = []
        for t, (slot, cam, ids, y, var) in enumerate(entries):
            ids = None if ids is None else _i32(ids)
            y = None if y is None else _f64(y).reshape(-1)
            M = 0 if ids is None else len(ids)
            if y is not None and ids is not None and y.size != 2 * M:
                raise ValueError(f"y holds {y.size} doubles, {2 * M} expected")
            keep.append((cam, ids, y))
            arr[t].slot, arr[t].M, arr[t].meas_var = int(slot), M, float(var)
            arr[t].cam = None if cam is None else C.cast(C.pointer(cam), C.c_void_p)
            arr[t].ids = None if ids is None else _ip(ids)
            arr[t].y = None if y is None else _dp(y)
        if out is None:
            m = max(n, 1)
            out = (np.full((m, self.max_particles), np.nan), np.full((m, self.max_particles), np.nan), np.full(m, np.nan), np.full(m, np.nan))
        ll, w, lse, ess = out
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqf_bens_likelihood(self.h, n, arr, _dp(ll), _dp(w), _dp(lse), _dp(ess), _ip(status)))
        return ll[:n], w[:n], lse[:n], ess[:n], [int(v) for v in status[:n]]

    def resample_weighted_seeded(self, entries, out=None):
        """entries: list of (slot, P_new, seed, stream): weightedResample on the slot's kept weights with uniforms(seed, stream, P_new) of
        include/eqf_ensemble_random.h, generated on the device; the slot's cloud becomes the P_new chosen particles. Returns (src (count, max_particles) int32,
        status[count]): row e holds the P_new source indices, the rest (and the rows of refused entries) are left as they were (-1 in a fresh array)."""
        n = len(entries)
        arr = (BensResampleEntry * max(n, 1))()
        for t, (slot, P_new, seed, stream) in enumerate(entries):
            arr[t].slot, arr[t].P_new, arr[t].seed, arr[t].stream = int(slot), int(P_new), _u64(seed), _u64(stream)
        src = np.full((max(n, 1), self.max_particles), -1, np.int32) if out is None else out
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqf_bens_resample_weighted_seeded(self.h, n, arr, _ip(src), _ip(status)))
        return src[:n], [int(v) for v in status[:n]]

    def covariance(self, slots):
        """([C_e (n_e, n_e) or None for a refused entry], status[count]): estimateParticleCovariance of every listed slot's cloud in the slot's chart"""
        slots = _i32(slots)
        n = len(slots)
        buf = np.full(max(n, 1) * NMAX * NMAX, np.nan)
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqf_bens_covariance(self.h, n, _ip(slots), _dp(buf), _ip(status)))
        mats = []
        for e in range(n):
            if status[e]:
                mats.append(None)
                continue
            d = self._slot_n(slots[e])
            mats.append(buf[e * NMAX * NMAX:e * NMAX * NMAX + d * d].reshape(d, d).T.copy())
        return mats, [int(v) for v in status[:n]]

    def follow(self, entries, out=None):
        """entries: list of (slot, seed, stream). Every listed cloud becomes a cloud over its slot's current landmark ids, in the slot's order: the kept landmarks'
        points moved byte for byte, the dropped ones gone, the added ones drawn on the device from the slot's Sigma conditional on the particle's sensor state and
        kept landmarks, with rows of normals(seed, stream, n, P) of include/eqf_ensemble_random.h. Returns (dropped[count], added[count], status[count]); the
        counts of a refused entry are left as they were (-1 in fresh arrays; pass `out` = (dropped, added) to see that they are not written)."""
        n = len(entries)
        arr = (BensFollowEntry * max(n, 1))()
        for t, (slot, seed, stream) in enumerate(entries):
            arr[t].slot, arr[t].seed, arr[t].stream = int(slot), _u64(seed), _u64(stream)
        dropped, added = (np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)) if out is None else out
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqf_bens_follow(self.h, n, arr, _ip(dropped), _ip(added), _ip(status)))
        return dropped[:n], added[:n], [int(v) for v in status[:n]]

    def stats(self, reset=False):
        """(kernel launches, factorisations of Sigma) since the last reset"""
        a, b = C.c_long(), C.c_long()
        self._chk(self.lib.eqf_bens_stats(self.h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value
