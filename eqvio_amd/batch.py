"""ctypes binding of the filter batch: include/eqf_batch.h (device level, libeqf_hip.so) and include/eqvio_batch.h (filter level, libeqvio_filter.so).

VIOFilterBatch holds B independent reference VIOFilters (fast or, per slot, accurate Riccati with the continuous or the discrete state matrix; at most 64 landmarks each) whose frames go to the GPU together:
one device call per step and mode, one workgroup per slot. BatchCore is the device level on its own. .slot(k) is a view with the method names of capi.VIOFilter, so the per-filter test helpers work on a slot unchanged.
The prototypes are declared in lists of their own (_batch_declared), apart from the loaders' _declared lists of eqf_hip.h / eqvio_filter.h.
"""
import ctypes as C
import os

import numpy as np

from eqvio_amd.capi import Camera, Settings, c_double_p, c_int_p, load_eqf_lib, load_filter_lib

EQF_BATCH_MAX_LANDMARKS = 64
BATCH_REMOVED_OLD, BATCH_REMOVED_OUTLIERS, BATCH_ADDED, BATCH_EMPTY, BATCH_UPDATED, BATCH_REMOVED_INVALID = 1, 2, 4, 8, 16, 32
RICCATI_FAST, RICCATI_ACCURATE = 0, 1  # EQVIO_BATCH_RICCATI_* (include/eqvio_batch.h)
STATE_MATRIX_CONTINUOUS, STATE_MATRIX_DISCRETE = 0, 1  # EQVIO_BATCH_STATE_MATRIX_*


class BatchFrame(C.Structure):
    """eqf_batch_frame (include/eqf_batch.h)."""

    _fields_ = [("slot", C.c_int), ("cam", Camera), ("imu13_mean", c_double_p), ("dt_total", C.c_double), ("k", C.c_int), ("imu13_k", c_double_p),
                ("dt_k", c_double_p), ("M", C.c_int), ("ids", c_int_p), ("y", c_double_p)]


class BatchTruth(C.Structure):
    """eqf_batch_truth (include/eqf_batch.h)."""

    _fields_ = [("slot", C.c_int), ("sensor", c_double_p), ("n_true", C.c_int), ("ids", c_int_p), ("p", c_double_p)]


class BatchAugmentEntry(C.Structure):
    """eqf_batch_augment_entry (include/eqf_batch.h)."""

    _fields_ = [("slot", C.c_int), ("n_new", C.c_int), ("new_ids", c_int_p), ("n_prov", C.c_int), ("prov_ids", c_int_p), ("prov_p", c_double_p)]


EQF_BATCH_NBLOCKS = 7
BLOCK_NAMES = ("bias", "attitude", "position", "pose", "velocity", "camera", "sensor")  # EQF_BLOCK_* order


class BatchConsistencyRecord(C.Structure):
    """eqf_batch_consistency_record (include/eqf_batch.h)."""

    _fields_ = [("N", C.c_int), ("lu", C.c_int), ("nees", C.c_double), ("block", C.c_double * EQF_BATCH_NBLOCKS),
                ("eps", C.c_double * (21 + 3 * EQF_BATCH_MAX_LANDMARKS)), ("sigma_diag", C.c_double * (21 + 3 * EQF_BATCH_MAX_LANDMARKS)),
                ("ids", C.c_int * EQF_BATCH_MAX_LANDMARKS), ("lm_quad", C.c_double * EQF_BATCH_MAX_LANDMARKS), ("lm_err", C.c_double * EQF_BATCH_MAX_LANDMARKS)]

    def trimmed(self):
        """The record as a dict of numpy arrays trimmed to n = 21 + 3 N and N."""
        N, n = self.N, 21 + 3 * self.N
        return {"N": N, "lu": self.lu, "nees": self.nees, "block": np.array(self.block), "eps": np.array(self.eps)[:n], "sigma_diag": np.array(self.sigma_diag)[:n],
                "ids": np.array(self.ids, dtype=np.int32)[:N], "lm_quad": np.array(self.lm_quad)[:N], "lm_err": np.array(self.lm_err)[:N]}


class BatchEstimateRecord(C.Structure):
    """eqf_batch_estimate_record (include/eqf_batch.h)."""

    _fields_ = [("N", C.c_int), ("reserved", C.c_int), ("sensor", C.c_double * 23), ("sigma_sensor", C.c_double * (21 * 21)),
                ("ids", C.c_int * EQF_BATCH_MAX_LANDMARKS), ("p", C.c_double * (3 * EQF_BATCH_MAX_LANDMARKS)), ("p_world", C.c_double * (3 * EQF_BATCH_MAX_LANDMARKS))]

    def trimmed(self):
        """The record as a dict of numpy arrays trimmed to N: sensor[23], sigma_sensor (21, 21), ids[N], p (N, 3), p_world (N, 3)."""
        N = self.N
        return {"N": N, "sensor": np.array(self.sensor), "sigma_sensor": np.array(self.sigma_sensor).reshape(21, 21).T.copy(),
                "ids": np.array(self.ids, dtype=np.int32)[:N], "p": np.array(self.p)[: 3 * N].reshape(N, 3), "p_world": np.array(self.p_world)[: 3 * N].reshape(N, 3)}


class BatchPredictionEntry(C.Structure):
    """eqf_batch_prediction_entry (include/eqf_batch.h)."""

    _fields_ = [("slot", C.c_int), ("cam", Camera), ("k", C.c_int), ("imu13_k", c_double_p), ("dt_k", c_double_p)]


class BatchPredictionRecord(C.Structure):
    """eqf_batch_prediction_record (include/eqf_batch.h)."""

    _fields_ = [("N", C.c_int), ("reserved", C.c_int), ("sensor", C.c_double * 23), ("ids", C.c_int * EQF_BATCH_MAX_LANDMARKS),
                ("p", C.c_double * (3 * EQF_BATCH_MAX_LANDMARKS)), ("y", C.c_double * (2 * EQF_BATCH_MAX_LANDMARKS)),
                ("out_cov", C.c_double * (4 * EQF_BATCH_MAX_LANDMARKS))]

    def trimmed(self):
        """The record as a dict of numpy arrays trimmed to N: sensor[23], ids[N], p (N, 3), y (N, 2), out_cov (N, 2, 2)."""
        N = self.N
        return {"N": N, "sensor": np.array(self.sensor), "ids": np.array(self.ids, dtype=np.int32)[:N], "p": np.array(self.p)[: 3 * N].reshape(N, 3),
                "y": np.array(self.y)[: 2 * N].reshape(N, 2), "out_cov": np.array(self.out_cov)[: 4 * N].reshape(N, 2, 2)}


def load_batch_protos():
    """Declare the prototypes of include/eqf_batch.h on libeqf_hip.so and of include/eqvio_batch.h on libeqvio_filter.so."""
    elib, flib = load_eqf_lib(), load_filter_lib()
    if getattr(flib, "_batch_declared", None):
        return elib, flib
    vp, P = C.c_void_p, C.POINTER
    eprotos = {
        "eqf_batch_create": (C.c_int, [P(vp), C.c_int, C.c_int, C.c_int, P(Settings)]),
        "eqf_batch_destroy": (None, [vp]),
        "eqf_batch_slots": (C.c_int, [vp]),
        "eqf_batch_max_landmarks": (C.c_int, [vp]),
        "eqf_batch_set_slot_settings": (C.c_int, [vp, C.c_int, P(Settings)]),
        "eqf_batch_get_slot_settings": (C.c_int, [vp, C.c_int, P(Settings)]),
        "eqf_batch_check_settings": (C.c_int, [P(Settings)]),
        "eqf_batch_set_slot_chart": (C.c_int, [vp, C.c_int, C.c_int]),
        "eqf_batch_get_slot_chart": (C.c_int, [vp, C.c_int]),
        "eqf_batch_num_landmarks": (C.c_int, [vp, C.c_int]),
        "eqf_batch_set_state": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, c_int_p, c_double_p, c_double_p, C.c_int]),
        "eqf_batch_get_state": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, c_int_p, c_double_p, c_double_p, C.c_int]),
        "eqf_batch_set_sigma": (C.c_int, [vp, C.c_int, c_double_p, C.c_int]),
        "eqf_batch_get_sigma": (C.c_int, [vp, C.c_int, c_double_p, C.c_int]),
        "eqf_batch_state_estimate": (C.c_int, [vp, C.c_int, c_double_p, c_int_p, c_double_p, C.c_int]),
        "eqf_batch_sensor_estimate": (C.c_int, [vp, C.c_int, c_double_p]),
        "eqf_batch_step": (C.c_int, [vp, C.c_int, P(BatchFrame), c_int_p]),
        "eqf_batch_step_accurate": (C.c_int, [vp, C.c_int, P(BatchFrame), c_int_p]),
        "eqf_batch_step_discrete": (C.c_int, [vp, C.c_int, P(BatchFrame), c_int_p]),
        "eqf_batch_last_riccati": (C.c_int, [vp, C.c_int, c_int_p, c_int_p]),
        "eqf_batch_last_result": (C.c_int, [vp, C.c_int, c_int_p, c_double_p]),
        "eqf_batch_stream": (vp, [vp]),
        "eqf_batch_synchronize": (C.c_int, [vp]),
        "eqf_batch_nees": (C.c_int, [vp, C.c_int, P(BatchTruth), c_double_p, c_int_p]),
        "eqf_batch_nees_lu_fallbacks": (C.c_int, [vp, C.c_int, P(C.c_long)]),
        "eqf_batch_consistency": (C.c_int, [vp, C.c_int, P(BatchTruth), P(BatchConsistencyRecord), c_int_p]),
        "eqf_batch_estimates": (C.c_int, [vp, C.c_int, c_int_p, P(BatchEstimateRecord), c_int_p]),
        "eqf_batch_predictions": (C.c_int, [vp, C.c_int, P(BatchPredictionEntry), P(BatchPredictionRecord), c_int_p]),
        "eqf_batch_augment": (C.c_int, [vp, C.c_int, P(BatchAugmentEntry), c_int_p]),
        "eqf_batch_last_innovation": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, c_double_p]),
        "eqf_batch_innovation_totals": (C.c_int, [vp, C.c_int, P(C.c_long), P(C.c_long), c_double_p, c_double_p]),
        "eqf_batch_reset_innovation_totals": (C.c_int, [vp, C.c_int]),
        "eqf_batch_copy_slots": (C.c_int, [vp, C.c_int, c_int_p, c_int_p, c_int_p]),
        "eqf_batch_convert_chart": (C.c_int, [vp, C.c_int, c_int_p, c_int_p, c_int_p]),
        "eqf_batch_load_ctx": (C.c_int, [vp, vp, C.c_int, c_int_p, c_int_p]),
        "eqf_batch_store_ctx": (C.c_int, [vp, C.c_int, vp]),
    }
    fprotos = {
        "eqvio_batch_create": (C.c_int, [P(vp), P(Settings), C.c_int, C.c_int, C.c_int]),
        "eqvio_batch_create_slot_from_state": (C.c_int, [vp, C.c_int, c_double_p, c_int_p, c_double_p, C.c_int, C.c_double]),
        "eqvio_batch_destroy": (None, [vp]),
        "eqvio_batch_last_error": (C.c_char_p, [vp]),
        "eqvio_batch_slots": (C.c_int, [vp]),
        "eqvio_batch_set_slot_settings": (C.c_int, [vp, C.c_int, P(Settings)]),
        "eqvio_batch_get_slot_settings": (C.c_int, [vp, C.c_int, P(Settings)]),
        "eqvio_batch_set_slot_riccati": (C.c_int, [vp, C.c_int, C.c_int]),
        "eqvio_batch_get_slot_riccati": (C.c_int, [vp, C.c_int]),
        "eqvio_batch_set_slot_state_matrix": (C.c_int, [vp, C.c_int, C.c_int]),
        "eqvio_batch_get_slot_state_matrix": (C.c_int, [vp, C.c_int]),
        "eqvio_batch_set_slot_chart": (C.c_int, [vp, C.c_int, C.c_int]),
        "eqvio_batch_get_slot_chart": (C.c_int, [vp, C.c_int]),
        "eqvio_batch_process_imu": (C.c_int, [vp, C.c_int, c_double_p]),
        "eqvio_batch_process_vision": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, P(Camera), c_int_p, c_int_p, c_double_p, c_int_p]),
        "eqvio_batch_run_prepared": (C.c_int, [vp, P(vp), C.c_int, C.c_int]),
        "eqvio_batch_run_prepared_recorded": (C.c_int, [vp, P(vp), C.c_int, C.c_int, C.c_char_p]),
        "eqvio_batch_estimates": (C.c_int, [vp, C.c_int, c_int_p, P(BatchEstimateRecord), c_double_p, c_int_p]),
        "eqvio_batch_feature_predictions": (C.c_int, [vp, C.c_int, c_int_p, P(Camera), c_double_p, P(BatchPredictionRecord), c_int_p]),
        "eqvio_batch_state_estimate": (C.c_int, [vp, C.c_int, c_double_p, c_int_p, c_double_p, C.c_int]),
        "eqvio_batch_get_eqf": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, c_int_p, c_double_p, c_double_p, C.c_int]),
        "eqvio_batch_force_eqf": (C.c_int, [vp, C.c_int, c_double_p, c_double_p, c_int_p, c_double_p, c_double_p, C.c_int, c_double_p]),
        "eqvio_batch_sigma_dim": (C.c_int, [vp, C.c_int]),
        "eqvio_batch_get_sigma": (C.c_int, [vp, C.c_int, c_double_p, C.c_int]),
        "eqvio_batch_get_time": (C.c_double, [vp, C.c_int]),
        "eqvio_batch_is_initialised": (C.c_int, [vp, C.c_int]),
        "eqvio_batch_core": (vp, [vp]),
        "eqvio_batch_compute_nees": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, c_int_p, c_int_p, c_double_p, c_double_p, c_int_p]),
        "eqvio_batch_augment_landmark_states": (C.c_int, [vp, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p, c_int_p]),
        "eqvio_batch_run_sim": (C.c_int, [vp, P(vp), C.c_int, c_double_p, c_int_p]),
        "eqvio_batch_consistency": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, c_int_p, c_int_p, c_double_p, P(BatchConsistencyRecord), c_int_p]),
        "eqvio_batch_run_sim_recorded": (C.c_int, [vp, P(vp), C.c_int, c_double_p, c_int_p, C.c_char_p]),
        "eqvio_batch_last_innovation": (C.c_int, [vp, C.c_int, c_int_p, c_double_p, c_double_p]),
        "eqvio_batch_innovation_totals": (C.c_int, [vp, C.c_int, P(C.c_long), P(C.c_long), c_double_p, c_double_p]),
        "eqvio_batch_reset_innovation_totals": (C.c_int, [vp, C.c_int]),
        "eqvio_batch_copy_slots": (C.c_int, [vp, C.c_int, c_int_p, c_int_p, c_int_p]),
        "eqvio_batch_convert_chart": (C.c_int, [vp, C.c_int, c_int_p, c_int_p, c_int_p]),
        "eqvio_batch_load_filter": (C.c_int, [vp, vp, C.c_int, c_int_p, c_int_p]),
        "eqvio_batch_store_filter": (C.c_int, [vp, C.c_int, vp]),
    }
    for lib, protos in ((elib, eprotos), (flib, fprotos)):
        for name, (res, args) in protos.items():
            if os.environ.get("EQVIO_AMD_LIB_DIR") and name in ("eqf_batch_load_ctx", "eqf_batch_store_ctx", "eqvio_batch_load_filter", "eqvio_batch_store_filter", "eqf_batch_step_accurate", "eqf_batch_last_riccati",
                                                                   "eqvio_batch_set_slot_riccati", "eqvio_batch_get_slot_riccati", "eqf_batch_step_discrete",
                                                                   "eqvio_batch_set_slot_state_matrix", "eqvio_batch_get_slot_state_matrix", "eqf_batch_set_slot_chart",
                                                                   "eqf_batch_get_slot_chart", "eqvio_batch_set_slot_chart", "eqvio_batch_get_slot_chart", "eqf_batch_convert_chart",
                                                                   "eqvio_batch_convert_chart") and not hasattr(lib, name):
                continue  # same-box A/B against the libraries of an older commit (as capi.load_eqf_lib): entry points that commit did not have yet
            fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
    elib._batch_declared = sorted(eprotos)
    flib._batch_declared = sorted(fprotos)
    return elib, flib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _ip(a):
    return a.ctypes.data_as(c_int_p)


class BatchError(RuntimeError):
    def __init__(self, msg, code):
        super().__init__(msg)
        self.code = code


class BatchCore:
    """The device level of the batch (include/eqf_batch.h) on its own: B slots without the host half of a VIOFilter. Either a batch of its own
    (BatchCore(settings, slots)) or a view of the one behind a VIOFilterBatch (BatchCore.of(batch)), which stays the owner."""

    def __init__(self, settings, slots, max_landmarks=EQF_BATCH_MAX_LANDMARKS, device=0):
        self.elib, _ = load_batch_protos()
        self.h = C.c_void_p()
        self.owner = None
        rc = self.elib.eqf_batch_create(C.byref(self.h), device, slots, max_landmarks, C.byref(settings))
        if rc != 0:
            raise BatchError(f"eqf_batch_create: {rc} ({self.elib.eqf_error_string(rc).decode()})", rc)

    @classmethod
    def of(cls, batch):
        self = cls.__new__(cls)
        self.elib, self.h, self.owner = batch.elib, C.c_void_p(batch.core_handle()), batch
        return self

    def _chk(self, rc):
        if rc != 0:
            raise BatchError("eqf_batch: " + self.elib.eqf_error_string(rc).decode(), rc)

    def close(self):
        if self.h and self.owner is None:
            self.elib.eqf_batch_destroy(self.h)
        self.h = C.c_void_p()

    def set_slot_chart(self, k, chart):
        """Slot k's coordinate chart on its own (eqf_batch_set_slot_chart), COORD_NORMAL included; raises BatchError with EQF_E_BAD_ARG when refused."""
        self._chk(self.elib.eqf_batch_set_slot_chart(self.h, k, chart))

    def slot_chart(self, k):
        rc = self.elib.eqf_batch_get_slot_chart(self.h, k)
        if rc < 0:
            self._chk(rc)
        return rc

    def convert_chart(self, pairs):
        """pairs: list of (slot, chart). Slot `slot` is re-expressed in `chart` while it holds landmarks, Sigma <- T Sigma T^T, in ONE launch and without a
        transfer (eqf_batch_convert_chart): state, ids, other settings, totals and last result are kept. Returns the per-pair status codes (EQF_E_BAD_ARG: bad
        index, repeated slot, or a chart outside the enum; that slot is untouched); raises BatchError when the call itself failed."""
        n = len(pairs)
        slots, charts = _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.elib.eqf_batch_convert_chart(self.h, n, _ip(slots), _ip(charts), _ip(status)))
        return [int(v) for v in status[:n]]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, k, xi0, Xs, ids, q0, Q):
        xi0, Xs, ids, q0, Q = _f64(xi0), _f64(Xs), _i32(ids), _f64(q0), _f64(Q)
        self._chk(self.elib.eqf_batch_set_state(self.h, k, _dp(xi0), _dp(Xs), _ip(ids), _dp(q0), _dp(Q), len(ids)))

    def get_state(self, k):
        cap = EQF_BATCH_MAX_LANDMARKS
        xi0, Xs, ids, q0, Q = np.zeros(23), np.zeros(23), np.zeros(cap, np.int32), np.zeros(3 * cap), np.zeros(5 * cap)
        N = self.elib.eqf_batch_get_state(self.h, k, _dp(xi0), _dp(Xs), _ip(ids), _dp(q0), _dp(Q), cap)
        if N < 0:
            self._chk(N)
        return xi0, Xs, ids[:N].copy(), q0[: 3 * N].reshape(N, 3).copy(), Q[: 5 * N].reshape(N, 5).copy()

    def set_sigma(self, k, Sigma):
        S = np.asfortranarray(Sigma, dtype=np.float64)
        self._chk(self.elib.eqf_batch_set_sigma(self.h, k, S.ctypes.data_as(c_double_p), S.shape[0]))

    def get_sigma(self, k):
        n = 21 + 3 * self.elib.eqf_batch_num_landmarks(self.h, k)
        out = np.zeros((n, n), order="F")
        self._chk(self.elib.eqf_batch_get_sigma(self.h, k, out.ctypes.data_as(c_double_p), n))
        return out

    def _step(self, fn, entries):
        n = len(entries)
        arr = (BatchFrame * max(n, 1))()
        keep = []
        for e, (slot, cam, imus, dts, ids, y, *rest) in enumerate(entries):
            imus, dts, ids, y = _f64(imus).reshape(-1), _f64(dts).reshape(-1), _i32(ids), _f64(y).reshape(-1)
            mean = _f64(rest[0]) if rest and rest[0] is not None else None
            keep.append((imus, dts, ids, y, mean))
            arr[e].slot, arr[e].cam, arr[e].k, arr[e].M = slot, cam, len(dts), len(ids)
            arr[e].imu13_mean = _dp(mean) if mean is not None else None
            arr[e].dt_total = float(rest[1]) if len(rest) > 1 else 0.0
            arr[e].imu13_k = _dp(imus) if len(dts) else None
            arr[e].dt_k = _dp(dts) if len(dts) else None
            arr[e].ids = _ip(ids) if len(ids) else None
            arr[e].y = _dp(y) if len(ids) else None
        status = np.zeros(max(n, 1), np.int32)
        self._chk(fn(self.h, n, arr, _ip(status)))
        return status[:n].copy()

    def step(self, entries):
        """eqf_batch_step. entries: list of (slot, cam, imus[k, 13], dts[k], ids[M], y[2 M], imu13_mean, dt_total); returns the per-entry status codes."""
        return self._step(self.elib.eqf_batch_step, entries)

    def step_accurate(self, entries):
        """eqf_batch_step_accurate: the frame with one accurate Riccati step per IMU sample. entries as step's; imu13_mean and dt_total may be left out."""
        return self._step(self.elib.eqf_batch_step_accurate, entries)

    def step_discrete(self, entries):
        """eqf_batch_step_discrete: the frame with one discrete-state-matrix Riccati step per IMU sample. entries as step_accurate's."""
        return self._step(self.elib.eqf_batch_step_discrete, entries)

    def augment(self, entries):
        """eqf_batch_augment. entries: list of (slot, new_ids, provided_ids, provided_p[n, 3]): augmentLandmarkStates of every listed slot in one launch - the
        landmarks whose id is not in new_ids leave, the ids of new_ids the slot does not hold are appended with their provided points. Returns the per-entry
        status codes."""
        n = len(entries)
        arr = (BatchAugmentEntry * max(n, 1))()
        keep = []
        for e, (slot, new_ids, prov_ids, prov_p) in enumerate(entries):
            new_ids, prov_ids, prov_p = _i32(new_ids), _i32(prov_ids), _f64(prov_p).reshape(-1)
            keep.append((new_ids, prov_ids, prov_p))
            arr[e].slot, arr[e].n_new, arr[e].new_ids, arr[e].n_prov = int(slot), len(new_ids), _ip(new_ids), len(prov_ids)
            arr[e].prov_ids, arr[e].prov_p = _ip(prov_ids), _dp(prov_p)
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.elib.eqf_batch_augment(self.h, n, arr, _ip(status)))
        return status[:n].copy()

    def last_riccati(self, k):
        """(samples with dt > 0, most squarings) of slot k's last accurate or discrete step (eqf_batch_last_riccati)."""
        n, sq = C.c_int(), C.c_int()
        self._chk(self.elib.eqf_batch_last_riccati(self.h, k, C.byref(n), C.byref(sq)))
        return n.value, sq.value

    def last_result(self, k):
        flags, depth = C.c_int(), C.c_double()
        self._chk(self.elib.eqf_batch_last_result(self.h, k, C.byref(flags), C.byref(depth)))
        return flags.value, depth.value


class VIOFilterBatch:
    """B reference VIOFilters on one MI355X, advanced together (include/eqvio_batch.h). Every slot starts as VIOFilter(settings) and initialises itself from
    its first IMU sample, unless it is started from a state (start_slot)."""

    def __init__(self, settings, slots, max_landmarks=EQF_BATCH_MAX_LANDMARKS, device=0):
        self.elib, self.lib = load_batch_protos()
        self.h = C.c_void_p()
        self.settings = settings
        self.max_landmarks = max_landmarks
        rc = self.lib.eqvio_batch_create(C.byref(self.h), C.byref(settings), device, slots, max_landmarks)
        if rc != 0:
            raise BatchError(f"eqvio_batch_create: {rc} ({self.elib.eqf_error_string(rc).decode() if rc < 0 else 'see last error'})", rc)
        self.slots = slots

    def _chk(self, rc):
        if rc != 0:
            raise BatchError("eqvio_batch: " + (self.lib.eqvio_batch_last_error(self.h).decode() if rc == -1 else self.elib.eqf_error_string(rc).decode()), rc)

    def close(self):
        if self.h:
            self.lib.eqvio_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_slot_settings(self, k, settings):
        """Slot k's own settings from its next frame on (eqvio_batch_set_slot_settings): gains, thresholds, depth, lift choices and chart are per slot, so one
        step runs B different tunings. A refusal (fastRiccati 0, the Normal chart, a chart change on a slot that holds landmarks) raises BatchError with the
        EQF_E_* code and leaves the slot as it was. The initial-value fields only matter to a slot that has not initialised yet."""
        rc = self.lib.eqvio_batch_set_slot_settings(self.h, k, C.byref(settings))
        if rc != 0:
            raise BatchError(f"set_slot_settings({k}): " + (self.lib.eqvio_batch_last_error(self.h).decode() if rc == -1 else self.elib.eqf_error_string(rc).decode()), rc)

    def get_slot_settings(self, k):
        out = Settings()
        self._chk(self.lib.eqvio_batch_get_slot_settings(self.h, k, C.byref(out)))
        return out

    def set_slot_riccati(self, k, mode):
        """The propagation slot k's frames take from its next frame on (eqvio_batch_set_slot_riccati): RICCATI_FAST (every slot starts with it) or
        RICCATI_ACCURATE, the reference's default - one accurate Riccati step per IMU sample. k None: every slot. A bad mode or slot raises BatchError with
        EQF_E_BAD_ARG and changes nothing."""
        rc = self.lib.eqvio_batch_set_slot_riccati(self.h, -1 if k is None else k, mode)
        if rc != 0:
            raise BatchError(f"set_slot_riccati({k}, {mode}): " + self.elib.eqf_error_string(rc).decode(), rc)

    def slot_riccati(self, k):
        rc = self.lib.eqvio_batch_get_slot_riccati(self.h, k)
        if rc < 0:
            raise BatchError(f"slot_riccati({k}): " + self.elib.eqf_error_string(rc).decode(), rc)
        return rc

    def set_slot_state_matrix(self, k, kind):
        """The state matrix slot k's accurate Riccati steps use from its next frame on (eqvio_batch_set_slot_state_matrix): STATE_MATRIX_CONTINUOUS (every
        slot starts with it) or STATE_MATRIX_DISCRETE, the reference's useDiscreteStateMatrix. It matters only while the slot's Riccati mode is
        RICCATI_ACCURATE. k None: every slot. A bad kind or slot raises BatchError with EQF_E_BAD_ARG and changes nothing."""
        rc = self.lib.eqvio_batch_set_slot_state_matrix(self.h, -1 if k is None else k, kind)
        if rc != 0:
            raise BatchError(f"set_slot_state_matrix({k}, {kind}): " + self.elib.eqf_error_string(rc).decode(), rc)

    def set_slot_chart(self, k, chart):
        """Slot k's coordinate chart on its own, from its next frame on (eqvio_batch_set_slot_chart): COORD_EUCLIDEAN, COORD_INVDEPTH or COORD_NORMAL - the way to
        the Normal chart, which the settings calls refuse. k None: every slot (all of them or none). A chart outside the enum, a bad slot, or a slot that holds
        landmarks under another chart raises BatchError with EQF_E_BAD_ARG and changes nothing."""
        rc = self.lib.eqvio_batch_set_slot_chart(self.h, -1 if k is None else k, chart)
        if rc:
            raise BatchError(f"set_slot_chart({k}, {chart}): " + self.elib.eqf_error_string(rc).decode(), rc)

    def slot_chart(self, k):
        rc = self.lib.eqvio_batch_get_slot_chart(self.h, k)
        if rc < 0:
            raise BatchError(f"slot_chart({k}): " + self.elib.eqf_error_string(rc).decode(), rc)
        return rc

    def slot_state_matrix(self, k):
        rc = self.lib.eqvio_batch_get_slot_state_matrix(self.h, k)
        if rc < 0:
            raise BatchError(f"slot_state_matrix({k}): " + self.elib.eqf_error_string(rc).decode(), rc)
        return rc

    def last_riccati(self, k):
        """(samples, max_squarings) of slot k's last accurate or discrete step (eqf_batch_last_riccati): the samples that had dt > 0 and the most squarings
        one of its exponentials took (0 in the discrete mode); 0, 0 after a fast step or a copy into the slot."""
        n, sq = C.c_int(), C.c_int()
        self._chk(self.elib.eqf_batch_last_riccati(self.core_handle(), k, C.byref(n), C.byref(sq)))
        return n.value, sq.value

    def start_slot(self, k, sensor, ids, p, time):
        sensor, ids, p = _f64(sensor), _i32(ids), _f64(p)
        self._chk(self.lib.eqvio_batch_create_slot_from_state(self.h, k, _dp(sensor), _ip(ids), _dp(p), len(ids), time))

    def process_imu(self, k, imu13):
        imu13 = _f64(imu13)
        self._chk(self.lib.eqvio_batch_process_imu(self.h, k, _dp(imu13)))

    def process_vision(self, entries):
        """entries: list of (slot, stamp, camera, ids, y). One device step; returns the per-entry status codes."""
        n = len(entries)
        slots = _i32([e[0] for e in entries])
        stamps = _f64([e[1] for e in entries])
        cams = (Camera * max(n, 1))(*[e[2] for e in entries])
        counts = _i32([len(e[3]) for e in entries])
        ids = _i32(np.concatenate([np.asarray(e[3], np.int32) for e in entries]) if n else np.zeros(0, np.int32))
        y = _f64(np.concatenate([np.asarray(e[4], np.float64).ravel() for e in entries]) if n else np.zeros(0))
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_process_vision(self.h, n, _ip(slots), _dp(stamps), cams, _ip(counts), _ip(ids), _dp(y), _ip(status)))
        return status[:n].copy()

    def run_prepared(self, sequences, first=0, count=None, record_dir=None):
        """Lockstep replay (eqvio_batch_run_prepared): sequences[k] is slot k's capi.PreparedFrames (or None); frame j of every slot goes in one device step, a
        slot whose sequence has ended sits out. Returns the number of steps run. With record_dir every slot's IMUState.csv, camera.csv, bias.csv and points.csv
        go to record_dir/run_<k>/, one row per frame the slot ran (eqvio_batch_run_prepared_recorded); the slots end in the same state, bit for bit."""
        if len(sequences) > self.slots:
            raise ValueError("more sequences than slots")
        arr = (C.c_void_p * self.slots)(*([q.h if q is not None else None for q in sequences] + [None] * (self.slots - len(sequences))))
        n = max(len(q) for q in sequences if q is not None)
        count = n - first if count is None else count
        if record_dir is None:
            rc = self.lib.eqvio_batch_run_prepared(self.h, arr, first, count)
        else:
            rc = self.lib.eqvio_batch_run_prepared_recorded(self.h, arr, first, count, os.fsencode(record_dir))
        if rc < 0:
            self._chk(rc)
        return rc

    def state_estimates(self, slots, rec=None):
        """The estimate records of the listed slots in ONE launch (eqvio_batch_estimates): returns (records, times, status) - the untrimmed BatchEstimateRecord
        array (rec, or a new zeroed one; a refused entry's record is left as it was; .trimmed() gives numpy arrays), each slot's get_time() and the per-entry
        status codes. Only the records cross to the host."""
        n = len(slots)
        sl = _i32(list(slots) if n else np.zeros(1, np.int32))
        rec = (BatchEstimateRecord * max(n, 1))() if rec is None else rec
        times, status = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_estimates(self.h, n, _ip(sl), rec, _dp(times), _ip(status)))
        return rec, times[:n].copy(), status[:n].copy()

    def predictions(self, entries, rec=None):
        """Device level (eqf_batch_predictions). entries: list of (slot, cam, imus[k, 13], dts[k]): the slot's estimate taken through integrateSystemFunction
        with the k samples and dts, its landmarks projected through cam, and their output covariances at the current estimate, for every listed slot in ONE
        launch. Returns (records, status): the untrimmed BatchPredictionRecord array (rec, or a new zeroed one; a refused entry's record is left as it was;
        .trimmed() gives numpy arrays) and the per-entry status codes."""
        n = len(entries)
        arr = (BatchPredictionEntry * max(n, 1))()
        keep = []
        for e, (slot, cam, imus, dts) in enumerate(entries):
            imus, dts = _f64(imus).reshape(-1), _f64(dts).reshape(-1)
            keep.append((imus, dts))
            arr[e].slot, arr[e].cam, arr[e].k = slot, cam, len(dts)
            arr[e].imu13_k = _dp(imus) if len(dts) else None
            arr[e].dt_k = _dp(dts) if len(dts) else None
        rec = (BatchPredictionRecord * max(n, 1))() if rec is None else rec
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.elib.eqf_batch_predictions(self.core_handle(), n, arr, rec, _ip(status)))
        return rec, status[:n].copy()

    def feature_predictions(self, entries, rec=None):
        """Filter level (eqvio_batch_feature_predictions). entries: list of (slot, cam, stamp): getFeaturePredictions(cam, stamp) of every listed slot in ONE
        launch, each slot's samples and dts taken from its own IMU buffer and time. A slot whose settings have useFeaturePredictions off gets N = 0. Returns
        (records, status) as predictions."""
        n = len(entries)
        slots = _i32([e[0] for e in entries] if n else np.zeros(1, np.int32))
        cams = (Camera * max(n, 1))(*[e[1] for e in entries])
        stamps = _f64([e[2] for e in entries] if n else np.zeros(1))
        rec = (BatchPredictionRecord * max(n, 1))() if rec is None else rec
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_feature_predictions(self.h, n, _ip(slots), cams, _dp(stamps), rec, _ip(status)))
        return rec, status[:n].copy()

    def compute_nees(self, entries):
        """entries: list of (slot, true_sensor[23], true_ids, true_p[n, 3]). viewEqFState().computeNEES of every listed slot in ONE launch; returns the NEES
        values and the per-entry status codes (eqf_batch_nees; NaN where the status is not 0)."""
        n = len(entries)
        slots = _i32([e[0] for e in entries])
        sensors = _f64(np.concatenate([np.asarray(e[1], np.float64).ravel() for e in entries]) if n else np.zeros(0))
        counts = _i32([len(e[2]) for e in entries])
        ids = _i32(np.concatenate([np.asarray(e[2], np.int32) for e in entries]) if n else np.zeros(0, np.int32))
        p = _f64(np.concatenate([np.asarray(e[3], np.float64).ravel() for e in entries]) if n else np.zeros(0))
        nees, status = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_compute_nees(self.h, n, _ip(slots), _dp(sensors), _ip(counts), _ip(ids), _dp(p), _dp(nees), _ip(status)))
        return nees[:n].copy(), status[:n].copy()

    def consistency_records(self, entries, rec=None):
        """eqvio_batch_consistency on entries as compute_nees's: the untrimmed BatchConsistencyRecord array (rec, or a new zeroed one; a refused entry's
        record is left as it was) and the per-entry status codes."""
        n = len(entries)
        slots = _i32([e[0] for e in entries])
        sensors = _f64(np.concatenate([np.asarray(e[1], np.float64).ravel() for e in entries]) if n else np.zeros(0))
        counts = _i32([len(e[2]) for e in entries])
        ids = _i32(np.concatenate([np.asarray(e[2], np.int32) for e in entries]) if n else np.zeros(0, np.int32))
        p = _f64(np.concatenate([np.asarray(e[3], np.float64).ravel() for e in entries]) if n else np.zeros(0))
        rec = (BatchConsistencyRecord * max(n, 1))() if rec is None else rec
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_consistency(self.h, n, _ip(slots), _dp(sensors), _ip(counts), _ip(ids), _dp(p), rec, _ip(status)))
        return rec, status[:n].copy()

    def consistency(self, entries):
        """entries as compute_nees's. The consistency record of every listed slot in ONE launch (eqvio_batch_consistency): returns a list of dicts of numpy
        arrays trimmed to n = 21 + 3 N and N (nees, lu, block[7] in BLOCK_NAMES order, eps, sigma_diag, ids, lm_quad, lm_err; None where the status is not 0)
        and the per-entry status codes. Only the records cross to the host."""
        rec, status = self.consistency_records(entries)
        return [rec[e].trimmed() if status[e] == 0 else None for e in range(len(entries))], status

    def augment_landmark_states(self, entries):
        """entries: list of (slot, new_ids, provided_ids, provided_p[n, 3]). augmentLandmarkStates of every listed slot in ONE launch; returns the per-entry
        status codes (eqf_batch_augment)."""
        n = len(entries)
        slots = _i32([e[0] for e in entries])
        new_counts = _i32([len(e[1]) for e in entries])
        new_ids = _i32(np.concatenate([np.asarray(e[1], np.int32) for e in entries]) if n else np.zeros(0, np.int32))
        prov_counts = _i32([len(e[2]) for e in entries])
        prov_ids = _i32(np.concatenate([np.asarray(e[2], np.int32) for e in entries]) if n else np.zeros(0, np.int32))
        prov_p = _f64(np.concatenate([np.asarray(e[3], np.float64).ravel() for e in entries]) if n else np.zeros(0))
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_augment_landmark_states(self.h, n, _ip(slots), _ip(new_counts), _ip(new_ids), _ip(prov_counts), _ip(prov_ids), _dp(prov_p),
                                                               _ip(status)))
        return status[:n].copy()

    def run_sim(self, sims, max_frames, record_dir=None):
        """The reference's main_sim loop over the slots in lockstep (eqvio_batch_run_sim): sims[k] is slot k's capi.SimulationDataServer (or None). Returns the
        NEES of every frame and slot, shape (frames run, slots), NaN where a slot had no frame. With record_dir every run's consistency files (nees.csv,
        poseConsistency.csv, cameraConsistency.csv, biasConsistency.csv, landmarkError.csv) go to record_dir/run_<k>/ (eqvio_batch_run_sim_recorded); the
        returned array is the same, bit for bit."""
        if len(sims) > self.slots:
            raise ValueError("more simulations than slots")
        arr = (C.c_void_p * self.slots)(*([s.h if s is not None else None for s in sims] + [None] * (self.slots - len(sims))))
        nees = np.zeros(max(max_frames, 1) * self.slots)
        done = C.c_int()
        if record_dir is None:
            self._chk(self.lib.eqvio_batch_run_sim(self.h, arr, max_frames, _dp(nees), C.byref(done)))
        else:
            self._chk(self.lib.eqvio_batch_run_sim_recorded(self.h, arr, max_frames, _dp(nees), C.byref(done), os.fsencode(record_dir)))
        return nees[: done.value * self.slots].reshape(done.value, self.slots).copy()

    def nees_lu_fallbacks(self, k):
        out = C.c_long()
        self._chk(self.elib.eqf_batch_nees_lu_fallbacks(self.core_handle(), k, C.byref(out)))
        return out.value

    def synchronize(self):
        self._chk(self.elib.eqf_batch_synchronize(self.core_handle()))

    def core_handle(self):
        return self.lib.eqvio_batch_core(self.h)

    def last_result(self, k):
        flags, depth = C.c_int(), C.c_double()
        self._chk(self.elib.eqf_batch_last_result(self.core_handle(), k, C.byref(flags), C.byref(depth)))
        return flags.value, depth.value

    def last_innovation(self, k):
        """(dof, nis, logdet) of slot k's last step (eqvio_batch_last_innovation): the rows m of the matched measurement, yTilde^T S^-1 yTilde and log det S
        of its update; 0, 0, 0 after an empty measurement, m, NaN, NaN after a failed update. The innovation log-likelihood is
        -0.5 * (nis + logdet + dof * log(2 pi))."""
        dof, nis, logdet = C.c_int(), C.c_double(), C.c_double()
        self._chk(self.lib.eqvio_batch_last_innovation(self.h, k, C.byref(dof), C.byref(nis), C.byref(logdet)))
        return dof.value, nis.value, logdet.value

    def innovation_totals(self, k):
        """(updates, dof, nis, logdet): the sums over slot k's updated steps since the last reset, in step order (eqvio_batch_innovation_totals)."""
        n, dof, nis, logdet = C.c_long(), C.c_long(), C.c_double(), C.c_double()
        self._chk(self.lib.eqvio_batch_innovation_totals(self.h, k, C.byref(n), C.byref(dof), C.byref(nis), C.byref(logdet)))
        return n.value, dof.value, nis.value, logdet.value

    def reset_innovation_totals(self, k=None):
        """Clears slot k's totals, or every slot's (k None)."""
        self._chk(self.lib.eqvio_batch_reset_innovation_totals(self.h, -1 if k is None else k))

    def copy_slots(self, pairs):
        """pairs: list of (src, dst). Slot dst becomes slot src as it was before the call - state, landmarks, Sigma, IMU buffer, time, initialised flag - in
        ONE launch, without a transfer (eqvio_batch_copy_slots); any mapping goes in one call (fan-out, swap, cycle). dst keeps its own settings and innovation
        totals. Returns the per-pair status codes (EQF_E_BAD_ARG: bad index, repeated destination, or a chart other than the source's while it holds
        landmarks; that destination is untouched); raises BatchError when the call itself failed."""
        n = len(pairs)
        src, dst = _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_copy_slots(self.h, n, _ip(src), _ip(dst), _ip(status)))
        return [int(v) for v in status[:n]]

    def convert_chart(self, pairs):
        """pairs: list of (slot, chart). Slot `slot` is re-expressed in `chart` (COORD_*) while it holds landmarks - Sigma <- T Sigma T^T on the device, ONE
        launch, no transfer (eqvio_batch_convert_chart). It stays the same filter: state, ids, other settings, Riccati mode, state-matrix choice, innovation
        totals, last result, IMU buffer and time are kept. Returns the per-pair status codes (EQF_E_BAD_ARG: bad index, repeated slot, or a chart outside the
        enum; that slot is untouched); raises BatchError when the call itself failed."""
        n = len(pairs)
        slots, charts = _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_convert_chart(self.h, n, _ip(slots), _ip(charts), _ip(status)))
        return [int(v) for v in status[:n]]

    def load_filter(self, filter, slots):
        """Every listed slot becomes the capi.VIOFilter `filter` - EqF state, IMU buffer, time, initialised flag - in ONE launch, without Sigma or the
        landmarks crossing to the host (eqvio_batch_load_filter). The slots keep their own settings and innovation totals; the filter is unchanged. Returns the
        per-slot status codes (EQF_E_BAD_ARG: bad index, repeated slot, or a chart other than the filter's while it holds landmarks; that slot is untouched);
        raises BatchError when the whole call is refused (Normal chart or float Sigma store: EQF_E_UNSUPPORTED; more landmarks than the batch's capacity:
        EQF_E_CAPACITY) or failed."""
        n = len(slots)
        sl = _i32(list(slots) if n else np.zeros(1, np.int32))
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.eqvio_batch_load_filter(self.h, filter.h, n, _ip(sl), _ip(status)))
        return [int(v) for v in status[:n]]

    def load_core(self, core, slots):
        """The device level of load_filter (eqf_batch_load_ctx): every listed slot comes to hold the EqF state of the capi.EqfCore `core` - xi0, X, ids,
        landmarks, Sigma - bit for bit, in ONE launch. The slots' IMU buffers, times and initialised flags are not touched. Returns the per-slot status codes;
        raises BatchError when the whole call is refused or failed."""
        n = len(slots)
        sl = _i32(list(slots) if n else np.zeros(1, np.int32))
        status = np.zeros(max(n, 1), np.int32)
        self._chk(self.elib.eqf_batch_load_ctx(self.core_handle(), core.h, n, _ip(sl), _ip(status)))
        return [int(v) for v in status[:n]]

    def slot(self, k):
        if not 0 <= k < self.slots:
            raise IndexError(k)
        return BatchSlot(self, k)


class BatchSlot:
    """One slot of a VIOFilterBatch with capi.VIOFilter's method names. process_vision advances this slot alone (a step of one entry)."""

    def __init__(self, batch, k):
        self.b, self.k = batch, k
        self.cap = EQF_BATCH_MAX_LANDMARKS

    def set_slot_settings(self, settings):
        self.b.set_slot_settings(self.k, settings)

    def get_slot_settings(self):
        return self.b.get_slot_settings(self.k)

    @property
    def riccati(self):
        """RICCATI_FAST or RICCATI_ACCURATE (VIOFilterBatch.set_slot_riccati)."""
        return self.b.slot_riccati(self.k)

    @riccati.setter
    def riccati(self, mode):
        self.b.set_slot_riccati(self.k, mode)

    @property
    def state_matrix(self):
        """STATE_MATRIX_CONTINUOUS or STATE_MATRIX_DISCRETE (VIOFilterBatch.set_slot_state_matrix)."""
        return self.b.slot_state_matrix(self.k)

    @state_matrix.setter
    def state_matrix(self, kind):
        self.b.set_slot_state_matrix(self.k, kind)

    @property
    def chart(self):
        """COORD_EUCLIDEAN, COORD_INVDEPTH or COORD_NORMAL (VIOFilterBatch.set_slot_chart)."""
        return self.b.slot_chart(self.k)

    @chart.setter
    def chart(self, chart):
        self.b.set_slot_chart(self.k, chart)

    def convert_chart(self, chart):
        """This slot re-expressed in `chart` while it holds landmarks (VIOFilterBatch.convert_chart); a refusal raises BatchError with its code."""
        rc = self.b.convert_chart([(self.k, int(chart))])[0]
        if rc != 0:
            raise BatchError(f"convert_chart({self.k}, {chart}): " + self.b.elib.eqf_error_string(rc).decode(), rc)

    def copy_to(self, dsts):
        """This slot into every slot of dsts (one slot or a list), one launch (VIOFilterBatch.copy_slots); returns the status codes."""
        dsts = [dsts] if isinstance(dsts, (int, np.integer)) else list(dsts)
        return self.b.copy_slots([(self.k, int(d)) for d in dsts])

    def store_to(self, target):
        """This slot into a capi.VIOFilter (EqF state and the host half: eqvio_batch_store_filter) or a capi.EqfCore (EqF state alone: eqf_batch_store_ctx),
        one launch, as set_state + set_sigma with the slot's values would leave it. The slot is unchanged; a refusal raises BatchError with its code."""
        from eqvio_amd.capi import EqfCore

        if isinstance(target, EqfCore):
            self.b._chk(self.b.elib.eqf_batch_store_ctx(self.b.core_handle(), self.k, target.h))
        else:
            self.b._chk(self.b.lib.eqvio_batch_store_filter(self.b.h, self.k, target.h))

    def process_imu(self, imu13):
        self.b.process_imu(self.k, imu13)

    def process_vision(self, stamp, cam, ids, y):
        st = self.b.process_vision([(self.k, stamp, cam, ids, y)])
        if st[0] != 0:
            raise BatchError(f"slot {self.k}: {self.b.elib.eqf_error_string(int(st[0])).decode()}", int(st[0]))

    def compute_nees(self, sensor, ids, p):
        nees, st = self.b.compute_nees([(self.k, sensor, ids, p)])
        if st[0] != 0:
            raise BatchError(f"slot {self.k}: {self.b.elib.eqf_error_string(int(st[0])).decode()}", int(st[0]))
        return float(nees[0])

    def consistency(self, sensor, ids, p):
        """This slot's consistency record (VIOFilterBatch.consistency), a dict of numpy arrays trimmed to n and N."""
        rec, st = self.b.consistency([(self.k, sensor, ids, p)])
        if st[0] != 0:
            raise BatchError(f"slot {self.k}: {self.b.elib.eqf_error_string(int(st[0])).decode()}", int(st[0]))
        return rec[0]

    def augment_landmark_states(self, new_ids, sensor, ids, p):
        """capi.VIOFilter's signature; the provided state's sensor part is not used (nor is it by the reference)."""
        st = self.b.augment_landmark_states([(self.k, new_ids, ids, p)])
        if st[0] != 0:
            raise BatchError(f"slot {self.k}: {self.b.elib.eqf_error_string(int(st[0])).decode()}", int(st[0]))

    def feature_predictions(self, cam, stamp):
        """getFeaturePredictions(cam, stamp) of this slot (VIOFilterBatch.feature_predictions): (ids[N], y (N, 2), out_cov (N, 2, 2))."""
        rec, st = self.b.feature_predictions([(self.k, cam, stamp)])
        if st[0] != 0:
            raise BatchError(f"slot {self.k}: {self.b.elib.eqf_error_string(int(st[0])).decode()}", int(st[0]))
        r = rec[0].trimmed()
        return r["ids"], r["y"], r["out_cov"]

    def state_estimate(self):
        s, ids, p = np.zeros(23), np.zeros(self.cap, np.int32), np.zeros(3 * self.cap)
        N = self.b.lib.eqvio_batch_state_estimate(self.b.h, self.k, _dp(s), _ip(ids), _dp(p), self.cap)
        if N < 0:
            self.b._chk(N)
        return s, ids[:N].copy(), p[: 3 * N].reshape(N, 3).copy()

    def get_eqf(self):
        xi0, Xs = np.zeros(23), np.zeros(23)
        ids, q0, Q = np.zeros(self.cap, np.int32), np.zeros(3 * self.cap), np.zeros(5 * self.cap)
        N = self.b.lib.eqvio_batch_get_eqf(self.b.h, self.k, _dp(xi0), _dp(Xs), _ip(ids), _dp(q0), _dp(Q), self.cap)
        if N < 0:
            self.b._chk(N)
        return xi0, Xs, ids[:N].copy(), q0[: 3 * N].reshape(N, 3).copy(), Q[: 5 * N].reshape(N, 5).copy()

    def force_eqf(self, xi0_sensor, X_sensor, ids, q0, Q, Sigma):
        xi0_sensor, X_sensor, ids, q0, Q = _f64(xi0_sensor), _f64(X_sensor), _i32(ids), _f64(q0), _f64(Q)
        S = np.asfortranarray(Sigma, dtype=np.float64)
        self.b._chk(self.b.lib.eqvio_batch_force_eqf(self.b.h, self.k, _dp(xi0_sensor), _dp(X_sensor), _ip(ids), _dp(q0), _dp(Q), len(ids), S.ctypes.data_as(c_double_p)))

    def sigma_dim(self):
        return self.b.lib.eqvio_batch_sigma_dim(self.b.h, self.k)

    def get_sigma(self):
        n = self.sigma_dim()
        out = np.zeros((n, n), order="F")
        self.b._chk(self.b.lib.eqvio_batch_get_sigma(self.b.h, self.k, out.ctypes.data_as(c_double_p), n))
        return out

    def get_time(self):
        return self.b.lib.eqvio_batch_get_time(self.b.h, self.k)

    def is_initialised(self):
        return bool(self.b.lib.eqvio_batch_is_initialised(self.b.h, self.k))
