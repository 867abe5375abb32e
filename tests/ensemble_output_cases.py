"""Planted cases of the ensemble's measurement side (include/eqf_ensemble_output.h): tests/test_ensemble_output_cases.py proves them on the CPU,
tests/test_gpu_ensemble_output.py runs them on the device.

A case is P particles over M + 2 landmarks (two more than are measured, in another order), one camera of the three models, a measurement y of M landmarks
in yet another order, a measurement variance (the shipped measurementNoise^2 = 4 px^2) and P uniforms. Everything that is "truth" is restated with
oracle/indep/eqvio_ref.py's measure, a log-sum-exp in numpy and the reference's sequential weightedResample loop; nothing here calls the product. A
reference is computed once per case and shared.

The particles scatter 0.25 m around landmarks 4 - 12 m in front of the camera (about 14 px a coordinate), so that at M = 70 the exponents lie far below
log(DBL_MIN): the reference's plain exp(-q / 2) sums to exactly 0.0 there while the log-domain weights are finite - the reason for the feature, pinned.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(ROOT, "oracle", "indep")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from ensemble_cases import PINHOLE, STAT_SEEDS, R, StatFixture, flat_sensor, state_of  # noqa: E402
from eqvio_ref import Camera as RCam  # noqa: E402

CAM_NAMES = ("pinhole", "radtan", "equidistant")  # index = EQVIO_CAMERA_*
CAM_DIST = {0: (), 1: (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), 2: (-0.013721808247486035, 0.020727425669427896, -0.012786476702685545, 0.0025242267320687625)}
SIZES_M = (0, 1, 2, 11, 70)
SIZES_P = (1, 2, 31, 32, 33, 257)
MEAS_VAR = 4.0  # Settings.defaults().measurementNoise ** 2
MARGIN_CPU, MARGIN_GPU = 1e-8, 1e-9


def size_cases():
    """(camera model, M, P): every M with every camera model, P dealt round so that every P is seen"""
    return [(c, M, SIZES_P[(i + 2 * c) % len(SIZES_P)]) for c in range(3) for i, M in enumerate(SIZES_M)]


def case_key(cam, M, P):
    return f"{CAM_NAMES[cam]}-M{M}-P{P}"


def ref_camera(model):
    return RCam(model, *PINHOLE, CAM_DIST[model])


def device_camera(model):
    from eqvio_amd.capi import Camera

    if model == 0:
        return Camera.pinhole(*PINHOLE, 752, 480)
    if model == 1:
        return Camera.radtan(*PINHOLE, 752, 480, *CAM_DIST[1])
    return Camera.equidistant(*PINHOLE, 752, 480, *CAM_DIST[2])


def log_weights(ll):
    """(weights, logsumexp, ess) of log-likelihoods; a non-finite entry counts as -infinity"""
    ll = np.asarray(ll, float)
    fin = np.isfinite(ll)
    mx = np.max(ll[fin])
    e = np.where(fin, np.exp(np.where(fin, ll, mx) - mx), 0.0)
    s = e.sum()
    w = e / s
    return w, float(mx + np.log(s)), float(1.0 / np.sum(w * w))


def weighted_resample(w, u):
    """weightedResample (test/testing_utilities.h:55-74) on normalised weights w[P] with uniforms u[P_new]: the source index of every new particle"""
    P, Pn = len(w), len(u)
    idx, j, total = np.zeros(Pn, np.int32), 0, w[0]
    for k in range(Pn):
        thr = (u[k] + k) / Pn
        while total < thr and j + 1 < P:
            j += 1
            total += w[j]
        idx[k] = j
    return idx


def running_sums(w):
    """the loop's own running sums: w[0], then += w[j] in ascending j"""
    out, total = np.zeros(len(w)), 0.0
    for j in range(len(w)):
        total = w[j] if j == 0 else total + w[j]
        out[j] = total
    return out


def margin(w, u):
    """min over (j, k) of |cum_j - thr_k|: how far every comparison of the loop is from going the other way"""
    cum, Pn = running_sums(w), len(u)
    thr = (np.asarray(u, float) + np.arange(Pn)) / Pn
    return float(np.min(np.abs(cum[:, None] - thr[None, :])))


class OutputCase:
    """ids / sensor / p: the ensemble's particles (N = M + 2 landmarks); mids / y: the measurement; u: the uniforms"""

    def __init__(self, cam, M, P, seed=0):
        self.cam, self.M, self.P, self.N, self.var = cam, M, P, M + 2, MEAS_VAR
        rng = np.random.default_rng([seed, cam, M, P])
        N = self.N
        self.ids = rng.permutation(N).astype(np.int32) * 3 + 5
        q = np.column_stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(4, 12, N)])
        self.p = q[None, :, :] + 0.25 * rng.normal(size=(P, N, 3))
        self.sensor = rng.normal(size=(P, 23))
        for lo in (6, 16):
            self.sensor[:, lo:lo + 4] /= np.linalg.norm(self.sensor[:, lo:lo + 4], axis=1, keepdims=True)
        self.mpos = rng.permutation(N)[:M]  # the measured landmarks' places in the ensemble, in the measurement's order
        self.mids = self.ids[self.mpos].copy()
        rc = ref_camera(cam)
        y0 = np.array([R.project(rc, q[t]) for t in self.mpos], float).reshape(M, 2)
        self.y = y0 + np.sqrt(self.var) * rng.normal(size=(M, 2))
        self.u = rng.uniform(size=P)

    @functools.cached_property
    def measured(self):
        """(P, M, 2): oracle/indep's measure of every particle, picked by id"""
        rc = ref_camera(self.cam)
        out = np.zeros((self.P, self.M, 2))
        for k in range(self.P):
            y = R.measure(state_of(self.sensor[k], self.ids, self.p[k]), rc)
            for j, i in enumerate(self.mids):
                out[k, j] = np.asarray(y[int(i)], float)
        return out

    @functools.cached_property
    def quad(self):
        """q_k = sum_j |y_j - measure_k,j|^2 / var"""
        e = (self.y[None, :, :] - self.measured).reshape(self.P, -1)
        return np.einsum("ki,ki->k", e, e) / self.var

    @functools.cached_property
    def loglik(self):
        return -0.5 * self.quad

    @functools.cached_property
    def weights(self):
        return log_weights(self.loglik)

    @functools.cached_property
    def src(self):
        return weighted_resample(self.weights[0], self.u)

    @functools.cached_property
    def margin(self):
        return margin(self.weights[0], self.u)


@functools.lru_cache(maxsize=None)
def get_case(cam, M, P, seed=0):
    return OutputCase(cam, M, P, seed)


class StatOutputCase(OutputCase):
    """StatFixture's own output check at N = 2, P = 1000: its particles (the restated sampling), its measurement, variance and uniforms; all landmarks measured"""

    def __init__(self):
        f = StatFixture(2, 1000, STAT_SEEDS[(2, "output")])
        self.fixture = f
        self.cam, self.M, self.P, self.N, self.var = 0, 2, 1000, 2, f.var
        eps = np.linalg.cholesky(f.sigma0) @ f.xi
        ident = R.group_identity([int(i) for i in f.ids])
        parts = [R.state_action(ident, R.state_chart_inv("invdepth", eps[:, k], f.xi0)) for k in range(f.P)]
        self.ids = f.ids.copy()
        self.sensor = np.array([flat_sensor(s.sensor) for s in parts])
        self.p = np.array([np.asarray(s.p, float).reshape(2, 3) for s in parts])
        self.mpos = np.arange(2)
        self.mids, y = f.meas_flat()
        self.y = y.reshape(2, 2)
        self.u = f.uniforms


@functools.lru_cache(maxsize=None)
def stat_case():
    return StatOutputCase()
