"""Planted cases of the particle-ensemble tests (tests/test_ensemble_cases.py proves them on the CPU, tests/test_gpu_ensemble.py runs them on the device).

A case is a filter (xi0, X, ids, q0, Q, Sigma) of one chart and size, P columns of standard normals, an IMU sample and per-particle input offsets. Everything
that is "truth" is restated with oracle/indep/eqvio_ref.py (state_chart, state_chart_inv, state_action, group_inv, integrate_system, compute_nees) and
numpy's Cholesky; nothing here calls the product. Results are cached per case: a reference is computed once and shared by the tests that need it.

`python tests/ensemble_cases.py` rewrites tests/golden/ensemble_identity_baseline.json (what the restatement itself loses on NEES(sampled particle) = |xi|^2 / n).
"""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(ROOT, "oracle", "indep")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from eqvio_ref import EqVIORef, F64, State  # noqa: E402
from eqvio_ref import Camera as RCam  # noqa: E402
from util import random_imu, reasonable_state  # noqa: E402

R = EqVIORef(F64())
CHART_NAMES = ("euclid", "invdepth", "normal")  # index = EQVIO_COORD_*
BASELINE_PATH = os.path.join(HERE, "golden", "ensemble_identity_baseline.json")

# sizes: the edges of the 32-wide panels and row tiles. n = 21 (odd, padded, one panel), 24, 27, 33 (second panel begins), 54, 231 (8 panels, above the batch's 64 landmarks)
SIZES_N = (0, 1, 2, 4, 11, 70)
SIZES_P = (32, 31, 257, 33, 2, 1)


def size_cases():
    """(chart, N, P): every N with every chart (P dealt round so that each chart sees every P), and every P with every chart at N = 4 (n = 33)."""
    out = []
    for c in range(3):
        for k, N in enumerate(SIZES_N):
            out.append((c, N, SIZES_P[(k + c) % len(SIZES_P)]))
        for P in SIZES_P:
            if (c, 4, P) not in out:
                out.append((c, 4, P))
    return out


def case_key(chart, N, P):
    return f"{CHART_NAMES[chart]}-N{N}-P{P}"


def planted_sigma(rng, chart, N):
    """Unit-diagonal correlation (0.6 I + 0.4 low rank) between standard deviations that keep every sampled particle a reasonable state:
    sensor 0.01; points 0.1 m (Euclid), bearing 0.005 and inverse depth 0.002 at rho0 ~ 0.05 (InvDepth), bearing 0.005 and log depth 0.02 (Normal)."""
    n = 21 + 3 * N
    d = np.full(n, 0.01)
    lm = {0: (0.1, 0.1, 0.1), 1: (0.005, 0.005, 0.002), 2: (0.005, 0.005, 0.02)}[chart]
    for i in range(N):
        d[21 + 3 * i:24 + 3 * i] = lm
    G = rng.normal(size=(n, 6))
    C = G @ G.T
    s = 1.0 / np.sqrt(np.diag(C))
    C = 0.6 * np.eye(n) + 0.4 * (s[:, None] * C * s[None, :])
    S = d[:, None] * C * d[None, :]
    return 0.5 * (S + S.T)


def flat_sensor(s):
    return R.sensor_to_flat(s)


def state_of(sensor23, ids, p):
    return State(R.sensor_from_flat(sensor23), [int(i) for i in ids], np.asarray(p, float).reshape(len(ids), 3))


class Case:
    def __init__(self, chart, N, P, seed=0):
        self.chart, self.N, self.P, self.kind = chart, N, P, CHART_NAMES[chart]
        self.n = 21 + 3 * N
        rng = np.random.default_rng([seed, chart, N, P])
        self.xi0f, self.Xsf, self.ids, self.q0, self.Q = reasonable_state(rng, N, id_offset=7, shuffle_ids=True)
        self.Sigma = planted_sigma(rng, chart, N)
        self.xi = rng.normal(size=(self.n, P))
        self.imu = random_imu(rng, bias_vel=True)
        self.dt = 0.05
        self.offsets = rng.normal(size=(P, 6)) * 0.05
        # the truth handed to the device holds two more landmarks, in another order
        self.extra_ids = np.array([100001, 100002], np.int32)
        self.extra_p = rng.uniform(-1, 1, (P, 2, 3)) + np.array([0, 0, 15.0])
        self.perm = rng.permutation(N + 2)
        self.xi0 = R.state_from_flat(self.xi0f, self.ids, self.q0.reshape(N, 3))
        self.X = R.group_from_flat(self.Xsf, self.ids, self.Q.reshape(N, 5))

    # ---- the restated sampling: numpy Cholesky + state_chart_inv + state_action
    @functools.cached_property
    def L(self):
        return np.linalg.cholesky(self.Sigma)

    @functools.cached_property
    def sampled(self):
        """(sensor (P, 23), p (P, N, 3)) of particle_k = state_action(X, state_chart_inv(L xi_k ; xi0))"""
        eps = self.L @ self.xi
        sens, pts = np.zeros((self.P, 23)), np.zeros((self.P, self.N, 3))
        for k in range(self.P):
            st = R.state_action(self.X, R.state_chart_inv(self.kind, eps[:, k], self.xi0))
            sens[k], pts[k] = flat_sensor(st.sensor), np.asarray(st.p, float).reshape(self.N, 3)
        return sens, pts

    @functools.cached_property
    def truth_x(self):
        """the sampled particles as a truth with extra landmarks in another order: (ids (N + 2), sensor (P, 23), p (P, N + 2, 3))"""
        sens, pts = self.sampled
        ids = np.concatenate([self.ids, self.extra_ids]).astype(np.int32)[self.perm]
        p = np.concatenate([pts, self.extra_p], axis=1)[:, self.perm, :]
        return ids, sens, np.ascontiguousarray(p)

    def restated_errors(self, ids, sensor, p):
        """eps (n, P) = state_chart(state_action(X^-1, truth restricted to the filter's ids) ; xi0) for any truth"""
        ids = [int(i) for i in ids]
        idx = [ids.index(int(i)) for i in self.ids]
        Xinv = R.group_inv(self.X)
        out = np.zeros((self.n, len(sensor)))
        for k in range(len(sensor)):
            trunc = State(R.sensor_from_flat(sensor[k]), self.X.ids, np.asarray(p[k], float).reshape(-1, 3)[idx])
            out[:, k] = R.state_chart(self.kind, R.state_action(Xinv, trunc), self.xi0)
        return out

    @functools.cached_property
    def eps_truth(self):
        return self.restated_errors(*self.truth_x)

    @functools.cached_property
    def nees_restated(self):
        """compute_nees's formula for every particle at once: e^T Sigma^-1 e / n with one solve"""
        E = self.eps_truth
        return np.einsum("ik,ik->k", E, np.linalg.solve(self.Sigma, E)) / self.n

    @property
    def nees_identity(self):
        return np.einsum("ik,ik->k", self.xi, self.xi) / self.n

    @functools.cached_property
    def identity_baseline(self):
        """what the restatement itself loses on NEES(sampled particle k) = |xi_k|^2 / n, worst particle, relative"""
        return float(np.max(np.abs(self.nees_restated - self.nees_identity) / self.nees_identity))

    def integrated(self, sensor, p, offsets=None, dt=None):
        """integrate_system for every particle of (sensor (P, 23), p (P, N, 3)); offsets (P, 6) disturb gyr and acc"""
        dt = self.dt if dt is None else dt
        so, po = np.zeros_like(sensor), np.zeros_like(p)
        ids = list(range(p.shape[1]))
        for k in range(len(sensor)):
            imu = R.imu_from_flat(self.imu)
            if offsets is not None:
                imu = dict(imu, gyr=imu["gyr"] + offsets[k, 0:3], acc=imu["acc"] + offsets[k, 3:6])
            st = R.integrate_system(State(R.sensor_from_flat(sensor[k]), ids, p[k]), imu, dt)
            so[k], po[k] = flat_sensor(st.sensor), np.asarray(st.p, float).reshape(-1, 3)
        return so, po


@functools.lru_cache(maxsize=None)
def get_case(chart, N, P, seed=0):
    return Case(chart, N, P, seed)


def align_quats(a, b):
    """a's sensor rows with the sign of each quaternion (pose 6:10, camera 16:20) chosen as in b: q and -q are the same rotation"""
    a = np.array(a, float, copy=True).reshape(-1, 23)
    b = np.asarray(b, float).reshape(-1, 23)
    for lo in (6, 16):
        flip = np.einsum("ij,ij->i", a[:, lo:lo + 4], b[:, lo:lo + 4]) < 0
        a[flip, lo:lo + 4] *= -1
    return a


def load_baseline():
    with open(BASELINE_PATH) as f:
        return json.load(f)


# ---- the reference's statistical suite (test/test_FilterStatistics.cpp), restated at any size ------------------------------------------------------------
STAT_BANDS = {"initial": 0.1, "true_input": 1.0, "random_input": 0.1, "output": 0.5}  # :98, :116, :139, :167
STAT_SEEDS = {(2, "initial"): 1, (2, "true_input"): 22, (2, "random_input"): 3, (2, "output"): 4, (40, "initial"): 1, (40, "true_input"): 2}
PINHOLE = (458.654, 457.296, 367.215, 248.375)


class StatFixture:
    """FilterStatisticsTest's constructor (:30-53) at N landmarks: InvDepth, the variances of :32-41, filter = (xi0, Identity, Sigma0), and P columns of
    normals for the particles. The particles are eps = L xi through the exact chart inverse (the ensemble's sampling), not through exp(liftInnovation)."""

    def __init__(self, N, P, seed):
        from eqvio_amd.capi import COORD_INVDEPTH, Settings

        self.N, self.P, self.n = N, P, 21 + 3 * N
        self.rng = np.random.default_rng([seed, N])
        self.ids = np.arange(N, dtype=np.int32)
        s = Settings.defaults()
        s.coordinateChoice = COORD_INVDEPTH
        s.initialPointVariance = s.initialPointDepthVariance = 0.01**2
        s.initialBiasOmegaVariance = s.initialBiasAccelVariance = 0.01**2
        s.initialVelocityVariance = 0.1**2
        s.initialPositionVariance = 0.001**2
        # 0 * inputGain, 0 * stateGain in the propagation checks (:110-111, :133-134)
        for name in ("biasOmegaProcessVariance", "biasAccelProcessVariance", "attitudeProcessVariance", "positionProcessVariance", "velocityProcessVariance",
                     "cameraAttitudeProcessVariance", "cameraPositionProcessVariance", "pointProcessVariance", "velGyrNoise", "velAccNoise", "velGyrBiasWalk", "velAccBiasWalk"):
            setattr(s, name, 0.0)
        s.useEquivariantOutput, s.useDiscreteInnovationLift = 1, 0  # performVisionUpdate's defaults (VIO_eqf.h:107-109)
        self.settings = s
        self.xi0f = np.zeros(23)
        self.xi0f[0:6] = self.rng.uniform(-1, 1, 6)
        for lo in (6, 16):
            q = self.rng.normal(size=4)
            self.xi0f[lo:lo + 4] = q / np.linalg.norm(q)
        self.xi0f[10:13], self.xi0f[13:16], self.xi0f[20:23] = self.rng.uniform(-1, 1, 3), self.rng.uniform(-1, 1, 3), self.rng.uniform(-1, 1, 3)
        self.q0 = self.rng.uniform(-1, 1, (N, 3)) * 10.0
        self.q0[:, 2] += 20.0
        self.Xsf = np.zeros(23)
        self.Xsf[6] = self.Xsf[16] = 1.0
        self.Q = np.tile(np.array([1.0, 0, 0, 0, 1.0]), (N, 1))
        self.sigma0 = np.diag(s.initial_cov_diag(N))
        self.xi = self.rng.normal(size=(self.n, P))
        self.var = s.measurementNoise**2
        self.rcam = RCam(0, *PINHOLE)
        self.xi0 = R.state_from_flat(self.xi0f, self.ids, self.q0)
        self.true_vel = np.zeros(13)
        self.random_vel = np.zeros(13)
        self.random_vel[1:7] = self.rng.uniform(-1, 1, 6)
        y0 = R.measure(self.xi0, self.rcam)
        self.meas = {int(i): y0[int(i)] + np.sqrt(self.var) * self.rng.normal(size=2) for i in self.ids}
        self.uniforms = self.rng.uniform(size=P)

    def resample_indices(self, sensor, p):
        """the measurement likelihood and weightedResample (test/testing_utilities.h:55-74) on particles (sensor (P, 23), p (P, N, 3)): the source index of every new particle"""
        P = len(sensor)
        w = np.zeros(P)
        for k in range(P):
            y = R.measure(state_of(sensor[k], self.ids, p[k]), self.rcam)
            err = np.concatenate([self.meas[int(i)] - y[int(i)] for i in self.ids])
            w[k] = np.exp(-0.5 * err @ err / self.var)
        w /= w.sum()
        idx, j, total = [], 0, w[0]
        for k in range(P):
            thr = (self.uniforms[k] + k) / P
            while total < thr and j + 1 < P:
                j += 1
                total += w[j]
            idx.append(j)
        return np.array(idx, np.int32)

    def meas_flat(self):
        return self.ids.copy(), np.concatenate([self.meas[int(i)] for i in self.ids])


def restated_statistics(N, P, check, seed):
    """The mean NEES the reference's check would see (one value for "initial" and "output", five for the propagation checks), with the oracle filter on the CPU for
    the filter's side and the restated maps for the particles'."""
    from eqvio_amd.capi import Camera
    from oracle_binding import OracleFilter

    f = StatFixture(N, P, seed)
    orc = OracleFilter(f.settings)
    orc.set_eqf(f.xi0f, f.Xsf, f.ids, f.q0, f.Q, f.sigma0)
    L = np.linalg.cholesky(f.sigma0)
    eps = L @ f.xi
    ident = R.group_identity([int(i) for i in f.ids])
    parts = [R.state_action(ident, R.state_chart_inv("invdepth", eps[:, k], f.xi0)) for k in range(P)]

    def mean_nees():
        return float(np.mean([orc.compute_nees(flat_sensor(s.sensor), f.ids, np.asarray(s.p, float)) for s in parts]))

    if check == "initial":
        return [mean_nees()]
    if check in ("true_input", "random_input"):
        vel, dt = (f.true_vel, 0.2) if check == "true_input" else (f.random_vel, 0.05)
        out = []
        for rep in range(5):
            parts = [R.integrate_system(s, R.imu_from_flat(vel), dt) for s in parts]
            orc.integrate_riccati_discrete(vel, dt)
            orc.integrate_observer(vel, dt, True)
            out.append(mean_nees())
        return out
    sens = np.array([flat_sensor(s.sensor) for s in parts])
    pts = np.array([np.asarray(s.p, float).reshape(N, 3) for s in parts])
    idx = f.resample_indices(sens, pts)
    parts = [parts[j] for j in idx]
    mids, y = f.meas_flat()
    orc.vision_update(Camera.pinhole(*PINHOLE, 752, 480), mids, y)
    return [mean_nees()]


if __name__ == "__main__":
    base = {case_key(*c): get_case(*c).identity_baseline for c in size_cases()}
    with open(BASELINE_PATH, "w") as fh:
        json.dump(base, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(base, indent=1, sort_keys=True))
