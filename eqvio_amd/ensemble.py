"""ctypes binding of the particle ensemble: include/eqf_ensemble.h (libeqf_hip.so).

ParticleEnsemble holds P hypotheses of the true state on the device and judges them against one context (an EqfCore, or the core of a VIOFilter):
one factorisation of Sigma per nees() / sample() call, whatever P is. numpy arrays in, numpy arrays out, errors raised loudly (EqfError with the
library's code). The prototypes are declared in a list of their own (_ensemble_declared), apart from the loader's _declared list of eqf_hip.h; those of
include/eqf_ensemble_output.h (measure, likelihood, resample_weighted: the measurement side, on the device) in _ensemble_output_declared, those of
include/eqf_ensemble_random.h (the seeded draws, generated on the device) in _ensemble_random_declared.
"""
import ctypes as C

import numpy as np

from eqvio_amd.capi import EqfError, _dp, _f64, _i32, _ip, c_double_p, c_int_p, load_eqf_lib


def _cam_ptr(cam):
    return None if cam is None else C.addressof(cam)


def load_ensemble_protos():
    """Declare the prototypes of include/eqf_ensemble.h, include/eqf_ensemble_output.h and include/eqf_ensemble_random.h on libeqf_hip.so."""
    lib = load_eqf_lib()
    if getattr(lib, "_ensemble_declared", None):
        return lib
    vp, P = C.c_void_p, C.POINTER
    protos = {
        "eqf_ensemble_create": (C.c_int, [P(vp), C.c_int, C.c_int, C.c_int]),
        "eqf_ensemble_destroy": (None, [vp]),
        "eqf_ensemble_size": (C.c_int, [vp, c_int_p, c_int_p]),
        "eqf_ensemble_set": (C.c_int, [vp, C.c_int, C.c_int, c_int_p, c_double_p, c_double_p]),
        "eqf_ensemble_get": (C.c_int, [vp, c_int_p, c_double_p, c_double_p, C.c_int, C.c_int]),
        "eqf_ensemble_sample": (C.c_int, [vp, vp, C.c_int, c_double_p]),
        "eqf_ensemble_integrate": (C.c_int, [vp, c_double_p, C.c_double, c_double_p]),
        "eqf_ensemble_errors": (C.c_int, [vp, vp, c_double_p]),
        "eqf_ensemble_nees": (C.c_int, [vp, vp, c_double_p, c_double_p]),
        "eqf_ensemble_covariance": (C.c_int, [vp, vp, c_double_p]),
        "eqf_ensemble_resample": (C.c_int, [vp, C.c_int, c_int_p]),
        "eqf_ensemble_stats": (C.c_int, [vp, P(C.c_long), P(C.c_long), C.c_int]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    lib._ensemble_declared = sorted(protos)
    # include/eqf_ensemble_output.h, a list of its own
    cam_p = C.c_void_p
    output_protos = {
        "eqf_ensemble_measure": (C.c_int, [vp, cam_p, c_int_p, C.c_int, c_double_p]),
        "eqf_ensemble_likelihood": (C.c_int, [vp, cam_p, c_int_p, c_double_p, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p]),
        "eqf_ensemble_resample_weighted": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, c_int_p]),
    }
    for name, (res, args) in output_protos.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    lib._ensemble_output_declared = sorted(output_protos)
    # include/eqf_ensemble_random.h, a third list
    u64 = C.c_ulonglong
    random_protos = {
        "eqf_ensemble_normals": (C.c_int, [vp, u64, u64, C.c_int, C.c_int, c_double_p]),
        "eqf_ensemble_uniforms": (C.c_int, [vp, u64, u64, C.c_int, c_double_p]),
        "eqf_ensemble_sample_seeded": (C.c_int, [vp, vp, C.c_int, u64, u64]),
        "eqf_ensemble_resample_weighted_seeded": (C.c_int, [vp, C.c_int, c_double_p, u64, u64, c_int_p]),
        "eqf_ensemble_integrate_seeded": (C.c_int, [vp, c_double_p, C.c_double, c_double_p, u64, u64]),
    }
    for name, (res, args) in random_protos.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    lib._ensemble_random_declared = sorted(random_protos)
    return lib


def _u64(v):
    """a seed or a stream: a Python int taken modulo 2^64"""
    return int(v) & 0xFFFFFFFFFFFFFFFF


class ParticleEnsemble:
    """One eqf_ensemble against one context. core_or_filter: an EqfCore, or a VIOFilter (its eqf_ctx is taken through core_handle())."""

    def __init__(self, core_or_filter, max_particles, max_landmarks, device=0):
        self.lib = load_ensemble_protos()
        self.owner = core_or_filter  # keeps the context alive
        self.h = C.c_void_p()
        self.max_particles, self.max_landmarks = int(max_particles), int(max_landmarks)
        self._chk(self.lib.eqf_ensemble_create(C.byref(self.h), device, self.max_particles, self.max_landmarks))

    def _chk(self, rc):
        if rc != 0:
            raise EqfError(rc, self.lib.eqf_error_string(rc).decode())

    def _ctx(self):
        o = self.owner
        return C.c_void_p(o.core_handle()) if hasattr(o, "core_handle") else o.h

    def _ctx_n(self):
        return 21 + 3 * self.lib.eqf_num_landmarks(self._ctx())

    def close(self):
        if self.h:
            self.lib.eqf_ensemble_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        """(P, N)"""
        P, N = C.c_int(), C.c_int()
        self._chk(self.lib.eqf_ensemble_size(self.h, C.byref(P), C.byref(N)))
        return P.value, N.value

    def set(self, ids, sensor, p):
        """ids[N], sensor (P, 23), p (P, N, 3)"""
        ids, sensor, p = _i32(ids), _f64(sensor).reshape(-1, 23), _f64(p)
        P, N = sensor.shape[0], len(ids)
        if p.size != 3 * N * P:
            raise ValueError(f"p holds {p.size} doubles, {3 * N * P} expected")
        self._chk(self.lib.eqf_ensemble_set(self.h, P, N, _ip(ids), _dp(sensor), _dp(p)))

    def get(self):
        """(ids[N], sensor (P, 23), p (P, N, 3))"""
        P, N = self.size
        ids, sensor, p = np.zeros(N, np.int32), np.zeros((P, 23)), np.zeros((P, N, 3))
        rc = self.lib.eqf_ensemble_get(self.h, _ip(ids), _dp(sensor), _dp(p), P, N)
        if rc < 0:
            self._chk(rc)
        return ids, sensor, p

    def sample(self, xi):
        """xi (n, P) standard normals: particle k = stateGroupAction(X, stateChart^-1(L xi[:, k])), Sigma = L L^T"""
        xi = np.asfortranarray(xi, dtype=np.float64)
        if xi.ndim != 2 or xi.shape[0] != self._ctx_n():
            raise ValueError(f"xi must be (n, P) with n = {self._ctx_n()}")
        self._chk(self.lib.eqf_ensemble_sample(self.h, self._ctx(), xi.shape[1], xi.ctypes.data_as(c_double_p)))

    def integrate(self, imu, dt, offsets=None):
        """integrateSystemFunction for every particle; offsets (P, 6): gyr and acc disturbances per particle"""
        imu = _f64(imu)
        if offsets is None:
            self._chk(self.lib.eqf_ensemble_integrate(self.h, _dp(imu), float(dt), None))
            return
        offsets = _f64(offsets)
        if offsets.shape != (self.size[0], 6):
            raise ValueError("offsets must be (P, 6)")
        self._chk(self.lib.eqf_ensemble_integrate(self.h, _dp(imu), float(dt), _dp(offsets)))

    def errors(self):
        """eps (n, P): computeNEES's error coordinates of every particle in the context's chart"""
        out = np.zeros((self._ctx_n(), self.size[0]), order="F")
        self._chk(self.lib.eqf_ensemble_errors(self.h, self._ctx(), out.ctypes.data_as(c_double_p)))
        return out

    def nees(self):
        """(nees[P], mean)"""
        out, mean = np.zeros(self.size[0]), C.c_double()
        self._chk(self.lib.eqf_ensemble_nees(self.h, self._ctx(), _dp(out), C.byref(mean)))
        return out, mean.value

    def covariance(self):
        """(1 / P) sum eps_k eps_k^T, (n, n), exactly symmetric"""
        n = self._ctx_n()
        out = np.zeros((n, n), order="F")
        self._chk(self.lib.eqf_ensemble_covariance(self.h, self._ctx(), out.ctypes.data_as(c_double_p)))
        return out

    def resample(self, idx):
        idx = _i32(idx)
        self._chk(self.lib.eqf_ensemble_resample(self.h, len(idx), _ip(idx)))

    # ---- include/eqf_ensemble_output.h: the measurement side, no context involved
    def measure(self, cam, ids):
        """(P, M, 2): cam.projectPoint of the points ids[M] of every particle"""
        ids = _i32(ids)
        out = np.zeros((self.size[0], len(ids), 2))
        self._chk(self.lib.eqf_ensemble_measure(self.h, _cam_ptr(cam), _ip(ids), len(ids), _dp(out)))
        return out

    def likelihood(self, cam, ids, y, meas_var):
        """(loglik[P], weights[P], logsumexp, ess) of the measurement y (M, 2) of the landmarks ids[M] under every particle; the weights are kept on the device"""
        ids, y = _i32(ids), _f64(y).reshape(-1)
        if y.size != 2 * len(ids):
            raise ValueError(f"y holds {y.size} doubles, {2 * len(ids)} expected")
        P = self.size[0]
        ll, w, lse, ess = np.zeros(P), np.zeros(P), C.c_double(), C.c_double()
        self._chk(self.lib.eqf_ensemble_likelihood(self.h, _cam_ptr(cam), _ip(ids), _dp(y), len(ids), float(meas_var), _dp(ll), _dp(w), C.byref(lse), C.byref(ess)))
        return ll, w, lse.value, ess.value

    def resample_weighted(self, u, weights=None):
        """weightedResample with the uniforms u[P_new] by the kept weights (or weights[P]); returns the source index of every new particle"""
        u = _f64(u).reshape(-1)
        src = np.zeros(len(u), np.int32)
        wp = None
        if weights is not None:
            weights = _f64(weights).reshape(-1)
            if len(weights) != self.size[0]:
                raise ValueError("weights must be (P,)")
            wp = _dp(weights)
        self._chk(self.lib.eqf_ensemble_resample_weighted(self.h, len(u), wp, _dp(u), _ip(src)))
        return src

    # ---- include/eqf_ensemble_random.h: seeded draws generated on the device; seeds and streams are ints taken modulo 2^64
    def normals(self, seed, stream, rows, P):
        """(rows, P) standard normals of (seed, stream): entry (r, k) depends on seed, stream, r and k alone"""
        out = np.zeros((max(int(rows), 0), max(int(P), 0)), order="F")
        self._chk(self.lib.eqf_ensemble_normals(self.h, _u64(seed), _u64(stream), int(rows), int(P), out.ctypes.data_as(c_double_p)))
        return out

    def uniforms(self, seed, stream, count):
        """count uniforms in (0, 1) of (seed, stream)"""
        out = np.zeros(max(int(count), 0))
        self._chk(self.lib.eqf_ensemble_uniforms(self.h, _u64(seed), _u64(stream), int(count), _dp(out)))
        return out

    def sample_seeded(self, P, seed, stream):
        """sample(normals(seed, stream, n, P)) without the upload: the normals are generated where sample reads them"""
        self._chk(self.lib.eqf_ensemble_sample_seeded(self.h, self._ctx(), int(P), _u64(seed), _u64(stream)))

    def resample_weighted_seeded(self, P_new, seed, stream, weights=None):
        """resample_weighted(uniforms(seed, stream, P_new), weights); returns the source index of every new particle"""
        src = np.zeros(max(int(P_new), 0), np.int32)
        wp = None
        if weights is not None:
            weights = _f64(weights).reshape(-1)
            if len(weights) != self.size[0]:
                raise ValueError("weights must be (P,)")
            wp = _dp(weights)
        self._chk(self.lib.eqf_ensemble_resample_weighted_seeded(self.h, int(P_new), wp, _u64(seed), _u64(stream), _ip(src)))
        return src

    def integrate_seeded(self, imu, dt, sigma6, seed, stream):
        """integrate(imu, dt, offsets = (sigma6[:, None] * normals(seed, stream, 6, P)).T); sigma6: gyr xyz, acc xyz standard deviations (None is refused)"""
        imu = _f64(imu)
        sp = None
        if sigma6 is not None:
            sigma6 = _f64(sigma6).reshape(-1)
            if len(sigma6) != 6:
                raise ValueError("sigma6 must hold six standard deviations")
            sp = _dp(sigma6)
        self._chk(self.lib.eqf_ensemble_integrate_seeded(self.h, _dp(imu), float(dt), sp, _u64(seed), _u64(stream)))

    def stats(self, reset=False):
        """(kernel launches, factorisations of Sigma) since the last reset"""
        a, b = C.c_long(), C.c_long()
        self._chk(self.lib.eqf_ensemble_stats(self.h, C.byref(a), C.byref(b), int(reset)))
        return a.value, b.value
