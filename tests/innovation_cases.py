"""Innovation statistics of the filter batch (helper module, not a test): the planted frames (tests/batch_scenarios.py) on which eqf_batch_last_innovation is
checked, and their reference values.

reference(settings, sc) forms dof, NIS = yTilde^T S^-1 yTilde and log det S from the CPU oracle ALONE, at the state the update sees: propagated, the lost
landmarks and the discarded outliers removed, the new landmarks appended. S = C Sigma C^T + R comes from output_matrix_C and get_sigma (as
batch_scenarios.describe builds it), yTilde is the measurement minus the projection of the oracle's estimate; the rest is numpy. exact(ref) evaluates the same
two numbers from the same S and yTilde with 50 digits (mpmath), which is what tells how much of a gap is the float64 evaluation's own.

tests/test_batch_innovation_api.py checks on the CPU that every frame is well conditioned and that the scores tell tunings apart;
tests/test_gpu_batch_innovation.py holds the device to the reference."""
from dataclasses import dataclass

import numpy as np

import batch_scenarios as bs
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH
from oracle_binding import oracle_cam_project, oracle_cam_undistort
from slot_settings_cases import clone, tracking

GRID = (1, 8, 31, 32, 33, 63, 64)          # N = M: m = 2, 16, 62, 64, 66, 126, 128
NOISES = (0.4, 1.0, 1.5, 3.0)              # measurementNoise of the four per-slot tunings
COND_MAX = 1e6


@dataclass
class Reference:
    dof: int
    nis: float
    logdet: float
    cond: float
    S: np.ndarray
    yt: np.ndarray
    matched: list


def reference(settings, sc):
    """dof, NIS and log det S of the frame's update, from the oracle alone"""
    orc = bs.propagated(settings, sc.state, sc.Sigma, sc.t0, sc.stamp, sc.imus, riccati=True)
    ids0, have = sc.state[2], set(sc.mid.tolist())
    if settings.removeLostLandmarks:
        for i in reversed(range(len(ids0))):
            if int(ids0[i]) not in have:
                orc.remove_landmark_by_index(i)
    surv = orc.get_eqf()[2]
    absE, probE = orc.outlier_stats(sc.cam, sc.mid, sc.y)
    _, _, disc = bs.ranked_discards(absE, probE, settings.outlierThresholdAbs, settings.outlierThresholdProb, int((1.0 - settings.featureRetention) * len(sc.mid)))
    discarded = {int(surv[i]) for i in disc}
    for i in sorted(disc, reverse=True):
        orc.remove_landmark_by_index(i)
    kept = set(orc.get_eqf()[2].tolist())
    new = [j for j, i in enumerate(sc.mid) if int(i) not in kept and int(i) not in discarded]
    if new:  # addNewLandmarks: the bearing at the median depth of the landmarks that stay (the element nth_element leaves at position nk / 2), or the fixed depth
        d2 = np.sum(orc.state_estimate()[2] ** 2, axis=1)
        depth = float(np.sqrt(np.sort(d2)[len(d2) // 2])) if settings.useMedianDepth and len(d2) else settings.initialSceneDepth
        orc.add_landmarks(sc.mid[new], np.array([oracle_cam_undistort(sc.cam, sc.y[2 * j:2 * j + 2]) * depth for j in new]), settings.initialPointVariance)
    matched = [j for j, i in enumerate(sc.mid) if int(i) not in discarded]
    m = 2 * len(matched)
    if m == 0:
        return Reference(0, 0.0, 0.0, 1.0, np.zeros((0, 0)), np.zeros(0), [])
    ym = np.array([sc.y[2 * j + c] for j in matched for c in range(2)])
    C = orc.output_matrix_C(sc.cam, sc.mid[matched], ym, bool(settings.useEquivariantOutput))
    S = C @ orc.get_sigma() @ C.T + settings.measurementNoise**2 * np.eye(m)
    S = 0.5 * (S + S.T)
    _, eids, ep = orc.state_estimate()
    at = {int(i): p for i, p in zip(eids, ep)}
    yt = ym - np.concatenate([oracle_cam_project(sc.cam, at[int(sc.mid[j])]) for j in matched])
    if not np.all(np.isfinite(S)) or np.linalg.eigvalsh(S)[0] <= 0:
        return Reference(m, float("nan"), float("nan"), float("inf"), S, yt, matched)
    L = np.linalg.cholesky(S)
    z = np.linalg.solve(L, yt)
    return Reference(m, float(z @ z), float(2.0 * np.sum(np.log(np.diag(L)))), float(np.linalg.cond(S)), S, yt, matched)


def exact(ref, digits=50):
    """NIS and log det S of the same S and yTilde, evaluated with `digits` digits (a Cholesky factorisation and a forward substitution in mpmath); floats"""
    import mpmath as mp

    with mp.workdps(digits):
        m = ref.dof
        A = [[mp.mpf(float(ref.S[i, j])) for j in range(i + 1)] for i in range(m)]
        y = [mp.mpf(float(v)) for v in ref.yt]
        nis, logdet = mp.mpf(0), mp.mpf(0)
        for k in range(m):  # row k of L and entry k of z = L^-1 yTilde
            row = A[k]
            for j in range(k):
                row[j] = (row[j] - mp.fdot(row[:j], A[j][:j])) / A[j][j]
            d = mp.sqrt(row[k] - mp.fdot(row[:k], row[:k]))
            row[k] = d
            y[k] = (y[k] - mp.fdot(row[:k], y[:k])) / d
            nis += y[k] * y[k]
            logdet += 2 * mp.log(d)
        return float(nis), float(logdet)


def log_likelihood(dof, nis, logdet):
    return -0.5 * (nis + logdet + dof * np.log(2.0 * np.pi))


# ------------------------------------------------------------------------------------------------ the frames
# Every frame plants Sigma at the scale of a filter that is tracking (slot_settings_cases.tracking, x 1e-5): at the planted scale C Sigma C^T dwarfs R, so the
# score would not read measurementNoise, and S of the large frames is worse conditioned.
_built = {}


def tracking_euclid(S):
    """the Euclidean chart's rows of C are smaller than the InvDepth chart's: x 1e-3 puts C Sigma C^T next to R there (x 1e-5 would leave R alone in S, and
    the half-pixel noise of the planted measurement would make every landmark a probabilistic outlier)"""
    S *= 1e-3


def _once(name, fn):
    if name not in _built:
        _built[name] = fn()
    return _built[name]


def grid(chart=COORD_INVDEPTH, out=1):
    """(settings, scenarios): N = M over GRID, one batch"""
    def build():
        s = bs.shipped_euroc(coordinateChoice=chart, useEquivariantOutput=out)
        return s, [bs.make(s, f"inn{N}", 11000 + N, N, sigma_edit=tracking) for N in GRID]
    return _once(("grid", chart, out), build)


def variants33():
    """[(settings, scenario)]: both charts and both outputs at N = 33, one slot each (per-slot settings)"""
    def build():
        res = []
        for chart in (COORD_EUCLIDEAN, COORD_INVDEPTH):
            for out in (0, 1):
                s = bs.shipped_euroc(coordinateChoice=chart, useEquivariantOutput=out)
                res.append((s, bs.make(s, f"inn33_c{chart}_o{out}", 11100 + 2 * chart + out, 33, sigma_edit=tracking if chart == COORD_INVDEPTH else tracking_euclid)))
        return res
    return _once("variants33", build)


RANK_CAP = 5  # of the 5 absolute and 6 probabilistic-only candidates of the ranking frame: the cap binds


def dof_frames():
    """[(name, settings, scenario)]: frames whose matched measurement is not the measurement"""
    def build():
        rank = bs.shipped_euroc(featureRetention=bs.retention_for(RANK_CAP), **bs.RANK_SETTINGS)
        turn = bs.shipped_euroc()
        keep = bs.shipped_euroc(removeLostLandmarks=0)
        return [("rank64_cap", rank, bs.make(rank, "rank64", 4000, 64, abs_out=bs.ABS_OUT, prob_out=bs.PROB_OUT, noise_px=0.2)),
                ("turnover16", turn, bs.make(turn, "turnover16", 11200, 64, measured=[i for i in range(64) if i not in bs.spread(64, 16)], new=16, sigma_edit=tracking)),
                ("keep_lost_8of64", keep, bs.make(keep, "partial8", 11201, 64, measured=bs.spread(64, 8), sigma_edit=tracking))]
    return _once("dof", build)


def noise_frames():
    """(base settings, [(settings, scenario)]): the same frame (N = 12) under four measurementNoise values"""
    def build():
        base = bs.shipped_euroc()
        sc = bs.make(base, "noise12", 11300, 12, sigma_edit=tracking)
        return base, [(clone(base, measurementNoise=v), sc) for v in NOISES]
    return _once("noise", build)


def all_frames():
    """[(name, settings, scenario)] of every frame with an update the GPU test compares: the CPU test checks their conditioning"""
    out = []
    s, scs = grid()
    out += [(sc.name, s, sc) for sc in scs]
    out += [(sc.name, s, sc) for s, sc in variants33()]
    out += dof_frames()
    out += [(f"noise{s.measurementNoise}", s, sc) for s, sc in noise_frames()[1]]
    return out
