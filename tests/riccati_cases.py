"""Planted frames for the filter batch's accurate Riccati mode (helper module, not a test): eqf_batch_step_accurate / k_batch_riccati
(eqvio_amd/csrc/eqf_batch.hpp). One case is one batch_scenarios.Scenario - a planted state and Sigma, the buffered IMU samples, the measurement - at an edge of
the per-sample propagation: no landmark, one, the sizes 40 and 64, one / two / ten samples, a sample with dt = 0 between two others, a step long and fast
enough that the exponential needs squarings, landmark turnover, discarded outliers.

 * oracle_settings(s) is s with fastRiccati = 0: what the case's oracle runs with. The batch's own settings keep fastRiccati = 1.
 * walk(settings, sc) takes the case through the oracle's VIO_eqf calls sample by sample - integrateUpToTime with fastRiccati == false - and reports the
   infinity norm of dt [A B] of every sample with dt > 0; tests/test_batch_riccati_cases.py checks on the CPU that every case is the edge it claims.
 * propagation_only(sc) is the case with an empty measurement: with removeLostLandmarks = 0 the frame then is integrateUpToTime and nothing else."""
import copy

import numpy as np

import batch_scenarios as bs
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, Settings
from oracle_binding import OracleFilter
from util import estimate_landmarks, imu_selection, project, random_imu, random_spd, reasonable_state

DT = 0.005  # the sample spacing of the small-step cases: |dt [A B]|_inf stays below the scaling threshold 0.25
DT_LONG = 0.35
NORM_EDGE = 0.25  # k_batch_riccati scales by 2^-s until the norm is at most this


def oracle_settings(s):
    o = Settings.from_buffer_copy(bytes(s))
    o.fastRiccati = 0
    return o


def imus_at(rng, stamps, gyro=0.05):
    """one IMU sample per stamp: gyroscope rates of scale `gyro` rad/s, accelerometer near gravity"""
    scale = np.array([1] + [gyro] * 3 + [0.2] * 3 + [0] * 6)
    return np.stack([random_imu(rng, stamp=t) * scale + np.array([0] * 4 + [0, 0, 9.0] + [0] * 6) for t in stamps])


NEAR = 0.3  # the cases' landmarks are about 6 m away instead of 20: a Euclidean landmark's rows of A and B grow with |q0| (the skew(q_hat) blocks, twice), and
# at 20 m 0.005 |[A B]|_inf is already 0.55, past the scaling threshold


def make(settings, name, seed, N, rel_stamps, frame, *, gyro=0.05, lost=0, new=0, abs_out=(), noise_px=0.5, t0=2.0):
    """One planted frame: IMU samples at t0 + rel_stamps, the image at t0 + frame. lost: landmarks the frame does not measure; new: new ids; abs_out:
    (state index, pixel offset) pairs."""
    rng = np.random.default_rng(seed)
    cam = bs.PINHOLE
    stamp = t0 + frame
    xi0, Xs, ids, q0, Q = reasonable_state(rng, N)
    q0 *= NEAR
    Sigma = random_spd(rng, 21 + 3 * N)
    imus = imus_at(rng, [t0 + r for r in rel_stamps], gyro)
    state = (xi0, Xs, ids, q0, Q)
    gone = bs.spread(N, lost) if lost else []
    measured = [i for i in range(N) if i not in gone]
    Qp = bs.propagated(settings, state, Sigma, t0, stamp, imus).get_eqf()[4]
    pix = project(cam, estimate_landmarks(q0, Qp)) + rng.normal(size=(N, 2)) * noise_px
    for i, off in abs_out:
        ang = rng.uniform(0, 2 * np.pi)
        pix[i] += off * np.array([np.cos(ang), np.sin(ang)])
    meas = {int(ids[i]): pix[i] for i in measured}
    new_ids = [int(ids[j]) + 1 for j in bs.spread(N, new)] if N else list(range(1, 3 * new, 3))
    for nid in new_ids:
        meas[nid] = np.array([rng.uniform(150, cam.width - 150), rng.uniform(100, cam.height - 100)])
    mid = np.array(sorted(meas), np.int32)
    y = np.array([meas[int(i)] for i in mid]).reshape(-1)
    plan = dict(measured=measured, lost=gone, new=new_ids, abs=[i for i, _ in abs_out])
    return bs.Scenario(name, state, Sigma, cam, t0, stamp, imus, mid, y, "full", plan)


def evenly(k, dt=DT):
    return [i * dt for i in range(k)], k * dt


def build(settings, tag):
    """the cases of one chart"""
    cases = [make(settings, f"{tag}_n0_k1", 100, 0, *evenly(1)), make(settings, f"{tag}_n1_k2", 101, 1, *evenly(2)), make(settings, f"{tag}_n40_k10", 102, 40, *evenly(10)),
             make(settings, f"{tag}_n64_k2", 103, 64, *evenly(2)), make(settings, f"{tag}_n40_k1", 104, 40, *evenly(1))]
    # a sample whose successor has its stamp: dt = 0 in the middle, dt > 0 either side
    cases.append(make(settings, f"{tag}_zero_dt_mid", 105, 40, [0.0, DT, DT], 2 * DT))
    # two long steps at a few rad/s: |dt [A B]|_inf >= 1, the squaring branch
    cases.append(make(settings, f"{tag}_long_k2", 106, 40, *evenly(2, DT_LONG), gyro=3.0))
    cases.append(make(settings, f"{tag}_turnover", 107, 40, *evenly(2), lost=5, new=5))
    cases.append(make(settings, f"{tag}_outliers", 108, 40, *evenly(2), abs_out=[(5, 30.0), (17, 40.0)], noise_px=0.2))
    return cases


SETTINGS = {"euclid": lambda **kw: bs.shipped_euroc(coordinateChoice=COORD_EUCLIDEAN, **kw), "invdepth": lambda **kw: bs.shipped_euroc(coordinateChoice=COORD_INVDEPTH, **kw)}
_built = {}


def cases(chart, **kw):
    """(batch settings, oracle settings, cases) of a chart; built once per process and settings"""
    key = (chart, tuple(sorted(kw.items())))
    if key not in _built:
        s = SETTINGS[chart](**kw)
        _built[key] = (s, oracle_settings(s), build(s, chart))
    return _built[key]


def is_long(sc):
    return "_long_" in sc.name


def expected_samples(sc):
    return int(np.sum(imu_selection(sc.imus, sc.t0, sc.stamp)[0] > 0))


def propagation_only(sc):
    """the case with an empty measurement"""
    out = copy.copy(sc)
    out.mid, out.y = np.zeros(0, np.int32), np.zeros(0)
    return out


def walk(settings, sc, accurate=True):
    """integrateUpToTime by the oracle's VIO_eqf calls: per sample the Riccati step (dt > 0) and the observer step; with accurate=False the fast branch (one
    Riccati step with the mean sample in front). Returns the oracle and the infinity norms of dt [A B] of the samples with dt > 0."""
    orc = OracleFilter(settings)
    orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    dts, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
    norms = []
    if not accurate:
        orc.integrate_riccati_fast(mean, total)
    for u, dt in zip(sc.imus, dts):
        if dt > 0:
            AB = np.hstack([orc.state_matrix_A(u), orc.input_matrix_B()])
            norms.append(dt * np.max(np.sum(np.abs(AB), axis=1)))
            if accurate:
                orc.integrate_riccati_accurate(u, dt)
        orc.integrate_observer(u, dt, bool(settings.useDiscreteVelocityLift))
    return orc, norms
