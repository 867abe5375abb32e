"""Planted frames for the filter batch (helper module, not a test): one Scenario is everything ONE processVisionData call of one slot needs - a planted
state and Sigma, the buffered IMU samples, the measurement - built from a seed and a few parameters, with no simulated world. The scenarios of GROUPS sit at
the size and bookkeeping edges of k_batch_frame (eqvio_amd/csrc/eqf_batch.hpp) that the simulated sizes never reach; every scenario of a group shares the
group's settings, so a group is one batch and one device step.

 * describe(settings, sc) runs a scenario through the CPU oracle ALONE and reports what it is: sizes, outlier candidates and discards, invalid landmarks, the
   smallest eigenvalue of the innovation covariance. tests/test_batch_scenarios.py checks that every scenario is the edge it claims to be.
 * run(batch, settings, scenarios) runs them on the device, all in ONE step, and through their oracles; tests/test_gpu_batch_edges.py compares.

The filter settings shared by the batch tests (shipped_euroc, reference_defaults, CAMERAS) live here as well."""
from dataclasses import dataclass, field

import numpy as np

from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, Camera, Settings
from oracle_binding import OracleFilter, oracle_cam_undistort
from run_configs import parity
from util import estimate_landmarks, imu_selection, project, random_imu, random_spd, reasonable_state

REMOVED_OLD, REMOVED_OUTLIERS, ADDED, EMPTY, UPDATED, REMOVED_INVALID = 1, 2, 4, 8, 16, 32  # EQF_BATCH_* (include/eqf_batch.h)
EQF_E_NONFINITE, EQF_E_NOT_SPD, EQF_E_CAPACITY = -1, -2, -4


def shipped_euroc(**kw):  # the shipped EuRoC configuration's filter settings: InvDepth, fixed depth, shipped thresholds
    s = Settings.defaults()
    vals = dict(coordinateChoice=COORD_INVDEPTH, fastRiccati=1, useDiscreteInnovationLift=0, useMedianDepth=0, initialSceneDepth=4.0, initialPointVariance=0.05,
                measurementNoise=1.5, outlierThresholdAbs=6.0, outlierThresholdProb=4.0, featureRetention=0.5)
    vals.update(kw)
    for k, v in vals.items():
        setattr(s, k, v)
    s.cameraOffset[:] = [0.5, -0.5, 0.5, -0.5, 0, 0, 0]
    return s


def reference_defaults(**kw):  # VIOFilterSettings.h defaults (Euclidean, median depth, thresholds 1e8), fast Riccati
    s = Settings.defaults()
    s.fastRiccati = 1
    s.cameraOffset[:] = [0.5, -0.5, 0.5, -0.5, 0, 0, 0]
    for k, v in kw.items():
        setattr(s, k, v)
    return s


CAMERAS = {
    "pinhole": None,
    "radtan": Camera.radtan(458.654, 457.296, 367.215, 248.375, 752, 480, -0.28, 0.07, 2e-4, 2e-5),
    "equidistant": Camera.equidistant(458.654, 457.296, 367.215, 248.375, 752, 480, -0.01, 0.02, -0.005, 0.001),
}
PINHOLE = Camera.pinhole(458.654, 457.296, 367.215, 248.375, 752, 480)
FRAME_DT = 0.05
SMALL = 1e-4  # scale of the rows of Sigma that are planted small (probabilistic-only outliers)


@dataclass
class Scenario:
    name: str
    state: tuple          # xi0[23], Xs[23], ids[N], q0[N, 3], Q[N, 5]
    Sigma: np.ndarray
    cam: Camera
    t0: float
    stamp: float
    imus: np.ndarray      # k rows of 13, stamps in [t0, stamp)
    mid: np.ndarray       # measurement ids, ascending
    y: np.ndarray         # 2 M pixels
    oracle: str = "full"  # "full": OracleFilter.process_vision; "no_update": propagation and bookkeeping only; "none": the frame is refused
    plan: dict = field(default_factory=dict)  # what the builder planted: measured / lost / new / abs / prob / invalid (state indices or ids), tie

    @property
    def N(self):
        return len(self.state[2])


def spread(n, count):
    """count distinct indices of range(n), evenly spread, both ends included when count >= 2"""
    if count >= n:
        return list(range(n))
    if count == 1:
        return [n - 1]
    return sorted(set(int(round(v)) for v in np.linspace(0, n - 1, count)))


def frame_imus(rng, t0, stamp, k):
    scale = np.array([1] + [0.05] * 3 + [0.2] * 3 + [0] * 6)
    return np.stack([random_imu(rng, stamp=t0 + (stamp - t0) * i / k) * scale + np.array([0] * 4 + [0, 0, 9.0] + [0] * 6) for i in range(k)])


def propagated(settings, state, Sigma, t0, stamp, imus, riccati=False):
    """A fresh oracle after the frame's observer steps (and, on request, its Riccati step), driven by the VIO_eqf calls"""
    orc = OracleFilter(settings)
    orc.set_eqf(*state, Sigma, time=t0)
    dts, mean, total = imu_selection(imus, t0, stamp)
    if riccati:
        orc.integrate_riccati_fast(mean, total)
    for u, dt in zip(imus, dts):
        orc.integrate_observer(u, dt, bool(settings.useDiscreteVelocityLift))
    return orc


def make(settings, name, seed, N, *, measured=None, new=0, abs_out=(), prob_out=(), invalid=(), k=2, cam=None, noise_px=0.5, tie_at_median=False,
         sigma_edit=None, oracle="full", t0=2.0):
    """One planted frame. measured: state indices the frame measures (default all); new: number of new ids, interleaved with the old ones in id order;
    abs_out / prob_out: (state index, pixel offset) pairs - the prob_out landmarks and the sensor block get SMALL rows in Sigma, so that only their chi^2
    statistic fires; invalid: state indices whose scale a is planted below 1e-8; tie_at_median: two kept landmarks share the median depth exactly."""
    rng = np.random.default_rng(seed)
    cam = cam or PINHOLE
    stamp = t0 + FRAME_DT
    xi0, Xs, ids, q0, Q = reasonable_state(rng, N)  # ids 0, 3, 6, ...: ascending with the index, with room between them
    n = 21 + 3 * N
    Sigma = random_spd(rng, n)
    if prob_out:
        d = np.ones(n)
        d[:21] = SMALL
        for i, _ in prob_out:
            d[21 + 3 * i:24 + 3 * i] = SMALL
        Sigma = d[:, None] * Sigma * d[None, :]
    for i in invalid:
        Q[i, 4] = 5e-9
    imus = frame_imus(rng, t0, stamp, k)
    measured = list(range(N)) if measured is None else sorted(measured)
    plan = dict(measured=measured, lost=[i for i in range(N) if i not in measured], abs=[i for i, _ in abs_out], prob=[i for i, _ in prob_out], invalid=list(invalid))
    if tie_at_median:
        kept = measured if settings.removeLostLandmarks else list(range(N))
        Qp = propagated(settings, (xi0, Xs, ids, q0, Q), Sigma, t0, stamp, imus).get_eqf()[4]
        d2 = np.sum(estimate_landmarks(q0, Qp)[kept] ** 2, axis=1)
        order = np.argsort(d2)
        a, b = kept[order[len(kept) // 2]], kept[order[len(kept) // 2 + 1]]
        q0[b], Q[b] = q0[a], Q[a]
        plan["tie"] = (a, b)
    state = (xi0, Xs, ids, q0, Q)
    Qp = propagated(settings, state, Sigma, t0, stamp, imus).get_eqf()[4]
    pix = project(cam, estimate_landmarks(q0, Qp)) + rng.normal(size=(N, 2)) * noise_px
    for i, off in list(abs_out) + list(prob_out):
        ang = rng.uniform(0, 2 * np.pi)
        pix[i] += off * np.array([np.cos(ang), np.sin(ang)])
    meas = {int(ids[i]): pix[i] for i in measured}
    new_ids = [int(ids[j]) + 1 for j in spread(N, new)] if N else list(range(1, 3 * new, 3))
    for nid in new_ids:
        meas[nid] = np.array([rng.uniform(150, cam.width - 150), rng.uniform(100, cam.height - 100)])
    plan["new"] = new_ids
    mid = np.array(sorted(meas), np.int32)
    y = np.array([meas[int(i)] for i in mid]).reshape(-1)
    if sigma_edit is not None:
        sigma_edit(Sigma)
    return Scenario(name, state, Sigma, cam, t0, stamp, imus, mid, y, oracle, plan)


# ------------------------------------------------------------------------------------------------ what a scenario is, by the oracle alone
def ranked_discards(absE, probE, thrAbs, thrProb, max_outliers):
    """removeOutliers' choice (src/VIOFilter.cpp:304-364): absolute outliers first, largest error first, then the probabilistic-only ones; at most max_outliers.
    Returns (absolute candidates, probabilistic-only candidates, discarded), state indices."""
    a = [i for i in range(len(absE)) if absE[i] >= 0 and absE[i] > thrAbs]
    p = [i for i in range(len(absE)) if absE[i] >= 0 and i not in a and probE[i] > thrProb]
    ranked = sorted(a, key=lambda i: -absE[i]) + sorted(p, key=lambda i: -probE[i])
    return a, p, ranked[:max_outliers]


def describe(settings, sc):
    """The scenario through the oracle alone. Returns a dict: N_before, lost, n_abs, n_prob (candidates), max_outliers, discarded (ids, predicted from the
    oracle's statistics by ranked_discards), new (ids), invalid (ids the oracle removed after its update), ids_after (the oracle's), ids_predicted, flags
    (predicted EQF_BATCH_* word), min_eig_S (of C Sigma C^T + R before the update; None without an update), distinct (no two candidate errors equal),
    median (depth the new landmarks got, from the oracle's new origin points; None without new ones), stats."""
    ids0 = sc.state[2]
    M = len(sc.mid)
    orc = propagated(settings, sc.state, sc.Sigma, sc.t0, sc.stamp, sc.imus, riccati=True)
    lost = [int(i) for i in ids0 if settings.removeLostLandmarks and i not in set(sc.mid.tolist())]
    for i in reversed(range(len(ids0))):
        if int(ids0[i]) in lost:
            orc.remove_landmark_by_index(i)
    surv = orc.get_eqf()[2]
    absE, probE = orc.outlier_stats(sc.cam, sc.mid, sc.y)
    max_out = int((1.0 - settings.featureRetention) * M)
    a, p, disc = ranked_discards(absE, probE, settings.outlierThresholdAbs, settings.outlierThresholdProb, max_out)
    vals = [absE[i] for i in a] + [probE[i] for i in p]
    discarded = [int(surv[i]) for i in disc]
    for i in sorted(disc, reverse=True):
        orc.remove_landmark_by_index(i)
    kept = [int(i) for i in surv if int(i) not in discarded]
    new = [int(i) for i in sc.mid if int(i) not in set(surv.tolist())]
    matched = [int(i) for i in sc.mid if int(i) not in discarded]
    out = dict(N_before=len(ids0), lost=lost, n_abs=len(a), n_prob=len(p), max_outliers=max_out, discarded=discarded, new=new, distinct=len(set(vals)) == len(vals),
               stats=(absE, probE), min_eig_S=None, median=None, kept_depth2=np.sum(orc.state_estimate()[2] ** 2, axis=1))
    if sc.oracle == "none":
        return out
    full = OracleFilter(settings)
    full.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    for u in sc.imus:
        full.process_imu(u)
    if sc.oracle == "full":
        full.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
    else:
        oracle_without_update(full, settings, sc)
    _, _, ids_after, q0_after, _ = full.get_eqf()
    if new:
        j, at = list(sc.mid).index(new[0]), {int(i): q for i, q in zip(ids_after, q0_after)}
        if new[0] in at:
            out["median"] = np.linalg.norm(at[new[0]]) / np.linalg.norm(oracle_cam_undistort(sc.cam, sc.y[2 * j:2 * j + 2]))
        orc.add_landmarks(np.array(new, np.int32), np.array([at.get(i, np.ones(3)) for i in new]), settings.initialPointVariance)
    out["ids_after"] = [int(i) for i in ids_after]
    out["invalid"] = [i for i in kept + new if i not in out["ids_after"]]
    out["ids_predicted"] = [i for i in kept + new if i not in out["invalid"]]
    updated = bool(matched) and sc.oracle == "full"
    out["flags"] = ((REMOVED_OLD if lost else 0) | (REMOVED_OUTLIERS if discarded else 0) | (ADDED if new else 0) | (0 if matched else EMPTY) |
                    (UPDATED if updated else 0) | (REMOVED_INVALID if out["invalid"] else 0))
    if matched:  # S of the update, from the oracle's C and Sigma at the propagated, compacted state
        C = orc.output_matrix_C(sc.cam, np.array(matched, np.int32), np.array([sc.y[2 * list(sc.mid).index(i) + c] for i in matched for c in range(2)]),
                                bool(settings.useEquivariantOutput))
        assert not np.any(C[:, :21])  # the output does not read the sensor states: S is made of the landmark blocks of Sigma alone
        S = C[:, 21:] @ orc.get_sigma()[21:, 21:] @ C[:, 21:].T + settings.measurementNoise**2 * np.eye(C.shape[0])
        out["min_eig_S"] = float(np.linalg.eigvalsh(0.5 * (S + S.T))[0]) if np.all(np.isfinite(S)) else float("nan")
        with np.errstate(all="ignore"):
            out["T_finite"] = bool(np.all(np.isfinite(orc.get_sigma() @ C.T)))
    return out


def oracle_without_update(orc, settings, sc):
    """What a slot holds after EQF_E_NOT_SPD / EQF_E_NONFINITE: the frame's propagation and landmark bookkeeping (removeOldLandmarks, addNewLandmarks with
    the fixed depth; these scenarios have no outlier) without the vision update. orc has the frame's IMU samples already."""
    assert not settings.useMedianDepth
    dts, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
    orc.integrate_riccati_fast(mean, total)
    for u, dt in zip(sc.imus, dts):
        orc.integrate_observer(u, dt, bool(settings.useDiscreteVelocityLift))
    ids = orc.get_eqf()[2]
    have = set(sc.mid.tolist())
    if settings.removeLostLandmarks:
        for i in reversed(range(len(ids))):
            if int(ids[i]) not in have:
                orc.remove_landmark_by_index(i)
    ids = set(orc.get_eqf()[2].tolist())
    new = [j for j, i in enumerate(sc.mid) if int(i) not in ids]
    if new:
        p = np.array([oracle_cam_undistort(sc.cam, sc.y[2 * j:2 * j + 2]) * settings.initialSceneDepth for j in new])
        orc.add_landmarks(sc.mid[new], p, settings.initialPointVariance)


# ------------------------------------------------------------------------------------------------ the runner
@dataclass
class Result:
    status: int
    flags: int
    depth: float
    ids_dev: np.ndarray
    ids_orc: np.ndarray
    parity: tuple  # run_configs.parity (state, Sigma); None when the ids differ or the scenario has no oracle
    orc: object
    eqf: tuple     # the slot after the frame: get_eqf() + (Sigma,)
    before: tuple  # ... and before it


def slot_arrays(slot):
    return tuple(slot.get_eqf()) + (slot.get_sigma(),)


def run(batch, settings, scenarios, slots=None):
    """Every scenario in its slot (scenario i in slots[i], default i), ONE batch.process_vision over all of them, each scenario's oracle next to it."""
    slots = list(range(len(scenarios))) if slots is None else list(slots)
    orcs, before = [], []
    for k, sc in zip(slots, scenarios):
        xi0 = sc.state[0]
        batch.start_slot(k, xi0, np.zeros(0, np.int32), np.zeros((0, 3)), sc.t0)
        batch.slot(k).force_eqf(*sc.state, sc.Sigma)
        orc = OracleFilter(settings)
        orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
        for u in sc.imus:
            batch.process_imu(k, u)
            orc.process_imu(u)
        orcs.append(orc)
        before.append(slot_arrays(batch.slot(k)))
    status = batch.process_vision([(k, sc.stamp, sc.cam, sc.mid, sc.y) for k, sc in zip(slots, scenarios)])
    out = []
    for k, sc, orc, st, bf in zip(slots, scenarios, orcs, status, before):
        if sc.oracle == "full":
            orc.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
        elif sc.oracle == "no_update":
            oracle_without_update(orc, settings, sc)
        flags, depth = batch.last_result(k)
        ids_dev, ids_orc = batch.slot(k).get_eqf()[2], orc.get_eqf()[2]
        with np.errstate(all="ignore"):  # the overflow scenario's Sigma is beyond what a Frobenius norm can square
            par = parity(batch.slot(k), orc) if sc.oracle != "none" and np.array_equal(ids_dev, ids_orc) else None
        out.append(Result(int(st), flags, depth, ids_dev, ids_orc, par, orc, slot_arrays(batch.slot(k)), bf))
    return out


def true_of(orc, rng):
    """A true state near the oracle's estimate, ids in any order (for compute_nees)"""
    es, eids, ep = orc.state_estimate()
    ts = es.copy()
    ts[0:6] += rng.normal(size=6) * 1e-3
    ts[13:16] += rng.normal(size=3) * 1e-2
    perm = rng.permutation(len(eids))
    return ts, eids[perm], (ep * (1.0 + rng.normal(size=ep.shape) * 1e-3))[perm]


# ------------------------------------------------------------------------------------------------ the scenarios
SIZES = [1, 2, 7, 8, 9, 14, 15, 16, 17, 30, 31, 32, 33, 46, 47, 48, 56, 62, 63, 64]
C_ABS, C_PROB = 5, 6
ABS_OUT = [(63, 30.0), (5, 12.0), (17, 15.0), (33, 18.0), (48, 21.0)]
PROB_OUT = [(0, 2.5), (9, 2.9), (31, 3.3), (32, 3.7), (50, 4.1), (62, 4.5)]
RANK_CAPS = [0, 1, C_ABS - 1, C_ABS, C_ABS + 1, C_ABS + C_PROB - 1, 32]


def retention_for(max_outliers, M=64):
    return 1.0 - (max_outliers + 0.5) / M


def plant_not_spd(S):  # landmark blocks negative definite: the first pivot of S = C Sigma C^T + R is <= 0
    S[21:, 21:] = -1e6 * np.eye(S.shape[0] - 21)


def plant_overflow(S):
    """A huge but finite cross term between the position error (row 9: no landmark row of A reads it, so S = C Sigma C^T + R stays what it was) and one
    landmark: T = Sigma C^T overflows in row 9, every pivot of S is finite and positive, Gamma is not finite."""
    S[9, 21 + 3 * 40] = S[21 + 3 * 40, 9] = 1e307


def size_grid(settings, cam_extra=True):
    scs = [make(settings, f"size{N}", 1000 + N, N) for N in SIZES]
    if cam_extra:
        scs.append(make(settings, "size64_radtan", 1900, 64, cam=CAMERAS["radtan"]))
    return scs


def partial(settings):
    return [make(settings, f"partial{M}", 2000 + M, 64, measured=spread(64, M)) for M in (0, 1, 8, 33, 63)] + [make(settings, "partial_full40", 2100, 40)]


def turnover(settings, median):
    scs = [make(settings, f"turnover{r}", 3000 + r, 64, measured=[i for i in range(64) if i not in spread(64, r)], new=r) for r in (1, 16, 63, 64)]
    if median:
        scs.append(make(settings, "turnover16_tie", 3100, 64, measured=[i for i in range(64) if i not in spread(64, 16)], new=16, tie_at_median=True))
    scs.append(make(settings, "over_capacity", 3200, 64, new=1, oracle="none"))
    return scs


def ranking(settings):
    return [make(settings, "rank64", 4000, 64, abs_out=ABS_OUT, prob_out=PROB_OUT, noise_px=0.2),
            make(settings, "rank12", 4001, 12, abs_out=[(11, 14.0), (2, 9.0)], prob_out=[(0, 3.0), (7, 4.0)], noise_px=0.2)]


def truncation(settings):
    return [make(settings, "trunc10", 4100, 10, abs_out=[(9, 20.0)], noise_px=0.2)]


def invalid_ends(settings):
    return [make(settings, "invalid0", 5000, 64, invalid=[0]), make(settings, "neighbour64", 5001, 64), make(settings, "invalid63", 5002, 64, invalid=[63]),
            make(settings, "invalid0_31_63", 5003, 64, invalid=[0, 31, 63]), make(settings, "neighbour33", 5004, 33)]


def failures(settings):
    meas = [i for i in range(64) if i not in (7, 50)]
    return [make(settings, "good_a", 6000, 64, measured=meas, new=2), make(settings, "not_spd", 6001, 64, measured=meas, new=2, sigma_edit=plant_not_spd, oracle="no_update"),
            make(settings, "good_b", 6002, 64), make(settings, "nonfinite", 6003, 64, measured=meas, new=2, sigma_edit=plant_overflow, oracle="no_update"),
            make(settings, "good_c", 6004, 17)]


def unequal_imu(settings):
    combos = [(k, N) for k in (1, 2, 10, 45) for N in (5, 40, 64)]
    order = np.random.default_rng(7).permutation(len(combos))
    return [make(settings, f"imu{combos[i][0]}_N{combos[i][1]}", 7000 + int(i), combos[i][1], k=combos[i][0]) for i in order]


RANK_SETTINGS = dict(pointProcessVariance=1e-8)  # so that the planted-small landmark blocks stay small through the propagation
GROUPS = {}
for _chart, _cn in ((COORD_EUCLIDEAN, "euclid"), (COORD_INVDEPTH, "invdepth")):
    for _lift in (0, 1):
        for _out in (0, 1):
            GROUPS[f"sizes_{_cn}_lift{_lift}_out{_out}"] = (lambda c=_chart, l=_lift, o=_out: shipped_euroc(coordinateChoice=c, useDiscreteInnovationLift=l, useEquivariantOutput=o), size_grid)
    GROUPS[f"partial_{_cn}"] = (lambda c=_chart: shipped_euroc(coordinateChoice=c, removeLostLandmarks=0), partial)
    GROUPS[f"turnover_fixed_{_cn}"] = (lambda c=_chart: shipped_euroc(coordinateChoice=c), lambda s: turnover(s, False))
    GROUPS[f"turnover_median_{_cn}"] = (lambda c=_chart: shipped_euroc(coordinateChoice=c, useMedianDepth=1, initialSceneDepth=7.5), lambda s: turnover(s, True))
    GROUPS[f"unequal_imu_{_cn}"] = (lambda c=_chart: shipped_euroc(coordinateChoice=c), unequal_imu)
for _cap in RANK_CAPS:
    GROUPS[f"rank_cap{_cap}"] = (lambda m=_cap: shipped_euroc(featureRetention=retention_for(m), **RANK_SETTINGS), ranking)
GROUPS["rank_truncation"] = (lambda: shipped_euroc(featureRetention=0.9, **RANK_SETTINGS), truncation)
GROUPS["invalid_ends"] = (shipped_euroc, invalid_ends)
GROUPS["failures"] = (lambda: shipped_euroc(outlierThresholdAbs=1e8, outlierThresholdProb=1e8), failures)
GROUPS["failures_euclid"] = (lambda: shipped_euroc(coordinateChoice=COORD_EUCLIDEAN, outlierThresholdAbs=1e8, outlierThresholdProb=1e8), failures)

_built = {}


def build_group(name):
    """(settings, scenarios) of a group; built once per process"""
    if name not in _built:
        make_settings, make_scenarios = GROUPS[name]
        s = make_settings()
        _built[name] = (s, make_scenarios(s))
    return _built[name]
