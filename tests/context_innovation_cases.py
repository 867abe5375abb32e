"""Innovation statistics of the single-filter context path (helper module, not a test): the planted frames on which eqf_last_innovation is checked, and their
reference values.

The frames are context_scenarios.Scenario objects - the existing ones by name where the form exists only there, new ones at the smallest shapes otherwise - and
run through context_scenarios.run_oracle unchanged. The reference of a frame's update is formed from the CPU oracle ALONE, as tests/innovation_cases.reference
does for the filter batch, at the state the update sees (propagated; on the select route the landmarks bs.ranked_discards picks on the oracle's outlier_stats
removed, which run_oracle does in front of its vision_update): S = C Sigma C^T + R from output_matrix_C and get_sigma, yTilde = the measurement minus the
projection of the oracle's estimate, then a numpy Cholesky factorisation for dof, NIS = yTilde^T S^-1 yTilde and log det S. exact(ref) evaluates the same two
numbers from the same S and yTilde in extended precision.

tests/test_context_innovation_cases.py checks on the CPU that every frame is well conditioned and its reference exact; tests/test_gpu_context_innovation.py holds
the device to the reference."""
from dataclasses import replace

import numpy as np

import context_scenarios as cs
import innovation_cases as ic
from context_scenarios import BY_NAME, Scenario, run_oracle  # noqa: F401  (re-exported: the tests take them from here)
from eqvio_amd.capi import OPT_INNOVATION_STATS, OPT_LIVE_COLUMNS_FIRST, OPT_LOOKAHEAD, OPT_SPECULATIVE
from oracle_binding import OracleFilter, oracle_cam_project

# A Cholesky factorisation and its two triangular solves are backward stable: to first order the relative error of NIS is a small multiple of cond(S) x 2^-53.
# With a factor 3 for the three triangular operations, the GPU bound of 1e-9 can be asked of a frame up to cond(S) = 1e-9 / (3 x 1.1e-16) = 3e6.
COND_MAX = 3e6
TOL = 1e-9
EXACT_GAP = 1e-10
MP_MAX_DOF = 130  # innovation_cases.exact (mpmath, 50 digits) up to here, a numpy longdouble Cholesky factorisation above


def reference_at(orc, settings, cam, mid, y):
    """ic.Reference of the update the oracle is about to apply with the measurement (mid, y)"""
    m = 2 * len(mid)
    y = np.asarray(y, dtype=np.float64)
    C = orc.output_matrix_C(cam, mid, y, bool(settings.useEquivariantOutput))
    S = C @ orc.get_sigma() @ C.T + settings.measurementNoise**2 * np.eye(m)
    S = 0.5 * (S + S.T)
    _, eids, ep = orc.state_estimate()
    at = {int(i): p for i, p in zip(eids, ep)}
    yt = y - np.concatenate([oracle_cam_project(cam, at[int(i)]) for i in mid])
    if not np.all(np.isfinite(S)) or np.linalg.eigvalsh(S)[0] <= 0:
        return ic.Reference(m, float("nan"), float("nan"), float("inf"), S, yt, list(range(len(mid))))
    L = np.linalg.cholesky(S)
    z = np.linalg.solve(L, yt)
    return ic.Reference(m, float(z @ z), float(2.0 * np.sum(np.log(np.diag(L)))), float(np.linalg.cond(S)), S, yt, list(range(len(mid))))


class _RecordingOracle(OracleFilter):
    """the oracle run_oracle drives, noting the reference of every update in front of it"""

    def vision_update(self, cam, ids, y, stamp=0.0):
        self.references.append(reference_at(self, self.settings, cam, np.asarray(ids, np.int32), y))
        return super().vision_update(cam, ids, y, stamp)

    references = None


_runs = {}


def oracle_run(sc):
    """(context_scenarios.OracleRun, [ic.Reference per frame]) of the scenario, once per process: run_oracle itself, with an oracle that notes the references"""
    if sc.name not in _runs:
        refs = []

        def make(settings):
            orc = _RecordingOracle(settings)
            orc.references = refs
            return orc

        keep, cs.OracleFilter = cs.OracleFilter, make
        try:
            run = run_oracle(sc)
        finally:
            cs.OracleFilter = keep
        assert len(refs) == sc.frames
        _runs[sc.name] = (run, refs)
    return _runs[sc.name]


def exact(ref):
    """(NIS, log det S) of the same S and yTilde in extended precision"""
    if ref.dof <= MP_MAX_DOF:
        return ic.exact(ref)
    m = ref.dof
    A = ref.S.astype(np.longdouble)
    L = np.zeros((m, m), np.longdouble)
    for k in range(m):  # column k of L
        col = A[k:, k] - L[k:, :k] @ L[k, :k]
        L[k:, k] = col / np.sqrt(col[0])
    z = np.zeros(m, np.longdouble)
    y = ref.yt.astype(np.longdouble)
    for k in range(m):
        z[k] = (y[k] - L[k, :k] @ z[:k]) / L[k, k]
    return float(z @ z), float(2 * np.sum(np.log(np.diag(L))))


def exact_gap(ref):
    """(relative gap of NIS, absolute gap of log det S) between the float64 reference and its extended-precision evaluation"""
    nis, logdet = exact(ref)
    return abs(ref.nis - nis) / abs(nis), abs(ref.logdet - logdet)


# ------------------------------------------------------------------------------------------------ the frames
def _new(name, route, chart, N, seed, **kw):
    return Scenario(name, route, chart, N, list(range(N)), seed, **kw)


def _frames():
    f = []
    # update route: one tile of width 2; exactly one tile; two chain panels, the second of width 2; 3 panels (the smallest look-ahead form); 13 panels with a ragged
    # last one; 17 panels (the second look-ahead form); 33 panels (the natural chain)
    for N in (1, 16, 17, 40, 200, 257):
        f.append((_new(f"inn_update_N{N}", "update", "invdepth", N, 7000 + N), ()))
    f.append((BY_NAME["update_inv_N513"], ()))
    # staged route: the speculative tail and the ZB forms (2 frames each: ZB = 2 or k_build_Z, then ZB = 3)
    for N in (40, 129, 257):
        f.append((_new(f"inn_staged_N{N}", "staged", "invdepth", N, 7100 + N, k=3), ()))
    # select route: live columns first (3 and 12 panels), masked columns factorised (above 16 panels, two launches for the decision)
    for name in ("select_inv_N40_M36", "select_inv_N200_M190", "select_inv_N513_M257"):
        f.append((BY_NAME[name], ()))
    # forced chain
    f.append((_new("inn_chain_N40", "update", "invdepth", 40, 7040), ((OPT_LOOKAHEAD, 0),)))
    f.append((_new("inn_chain_N200", "update", "invdepth", 200, 7200), ((OPT_LOOKAHEAD, 0),)))
    f.append((replace(BY_NAME["select_inv_N200_M190"], name="inn_select_N200_all_columns"), ((OPT_LIVE_COLUMNS_FIRST, 0),)))
    # charts and outputs
    f.append((_new("inn_euclid_N40", "update", "euclid", 40, 7301), ()))
    f.append((_new("inn_normal_N40", "update", "normal", 40, 7302), ()))
    f.append((_new("inn_out0_N33", "update", "invdepth", 33, 7303, star=0), ()))
    f.append((_new("inn_out1_N33", "update", "invdepth", 33, 7304, star=1), ()))
    return f


FRAMES = _frames()  # [(Scenario, options)]
FRAME_BY_NAME = {sc.name: (sc, opts) for sc, opts in FRAMES}
assert len(FRAME_BY_NAME) == len(FRAMES)
SELECT = ("select_inv_N40_M36", "select_inv_N200_M190", "select_inv_N513_M257", "inn_select_N200_all_columns")
NOT_SPD = _new("inn_not_spd_N8", "update", "invdepth", 8, 7400)


def not_spd_sigma(sc):
    """A planted Sigma under which S = C Sigma C^T + R has a non-positive pivot: the planted one with its landmark blocks' diagonal far below zero"""
    _, _, _, Sigma = cs.planted(sc)
    S = Sigma.copy()
    for i in range(21, S.shape[0]):
        S[i, i] = -1e3
    return S


def sequence_reference(settings, orc, imus, stamp, cam, mid, y):
    """(ic.Reference, oracle at the state the update sees) of the frame a VIOFilter is about to process from the state of `orc` (left untouched): the steps of
    innovation_cases.reference - propagation, lost landmarks, the outlier decision, new landmarks - on a fresh oracle, from one frame of a running sequence"""
    import batch_scenarios as bs
    from oracle_binding import oracle_cam_undistort

    mid, y = np.asarray(mid, np.int32), np.asarray(y, np.float64)
    o = bs.propagated(settings, orc.get_eqf(), orc.get_sigma(), orc.get_time(), stamp, imus, riccati=True)
    ids0, have = o.get_eqf()[2], set(mid.tolist())
    if settings.removeLostLandmarks:
        for i in reversed(range(len(ids0))):
            if int(ids0[i]) not in have:
                o.remove_landmark_by_index(i)
    surv = o.get_eqf()[2]
    known = set(surv.tolist())
    sel = [j for j, i in enumerate(mid) if int(i) in known]
    discarded = set()
    if sel:
        absE, probE = o.outlier_stats(cam, mid[sel], np.array([y[2 * j + c] for j in sel for c in range(2)]))
        _, _, disc = bs.ranked_discards(absE, probE, settings.outlierThresholdAbs, settings.outlierThresholdProb, int((1.0 - settings.featureRetention) * len(mid)))
        discarded = {int(surv[i]) for i in disc}
        for i in sorted(disc, reverse=True):
            o.remove_landmark_by_index(i)
    kept = set(o.get_eqf()[2].tolist())
    new = [j for j, i in enumerate(mid) if int(i) not in kept and int(i) not in discarded]
    if new:
        d2 = np.sum(o.state_estimate()[2] ** 2, axis=1)
        depth = float(np.sqrt(np.sort(d2)[len(d2) // 2])) if settings.useMedianDepth and len(d2) else settings.initialSceneDepth
        o.add_landmarks(mid[new], np.array([oracle_cam_undistort(cam, y[2 * j:2 * j + 2]) * depth for j in new]), settings.initialPointVariance)
    matched = [j for j, i in enumerate(mid) if int(i) not in discarded]
    ym = np.array([y[2 * j + c] for j in matched for c in range(2)])
    return reference_at(o, settings, cam, mid[matched], ym), o, (mid[matched], ym)


# ------------------------------------------------------------------------------------------------ the device
def drive_frame(core, sc, fr):
    """one frame of the scenario on the context, by its route (context_scenarios.run_device's calls); returns what the update call returned"""
    s = sc.settings()
    cam = cs.CAMERAS[sc.cam]
    Qd, Pd = s.input_gain_diag12(), s.state_gain_diag8()
    var = s.measurementNoise**2
    if sc.route == "update":
        core.integrate_riccati_fast(fr.mean, fr.total, Qd, Pd)
        core.vision_update(cam, fr.mid, fr.y, var, bool(sc.star), bool(sc.lift))
        return (1,)
    core.stage_measurement(fr.mid, fr.y)
    core.propagate_fast(fr.mean, fr.total, Qd, Pd, fr.imus, fr.dts, bool(sc.vel_lift))
    if sc.route == "staged":
        return core.stats_then_update(cam, fr.mid, fr.y, sc.thr_abs, sc.thr_prob, var, bool(sc.star), bool(sc.lift))
    return core.stats_select_update(cam, fr.mid, fr.y, sc.thr_abs, sc.thr_prob, sc.cap, var, bool(sc.star), bool(sc.lift))


def run_device(sc, orun, options=(), stats=True):
    """The frames of orun on a fresh context of exactly N landmarks with the innovation statistics on (stats) or off. Returns a dict: per frame the update call's
    result, last_innovation() (None with stats off) and (get_state(), state_estimate(), Sigma); the totals at the end; context_scenarios.read_counters."""
    from eqvio_amd.capi import EqfCore

    core = EqfCore(sc.N, cs.CHART_NAMES[sc.chart])
    try:
        for opt, val in options:
            core.set_option(opt, val)
        if sc.route == "select":
            core.set_option(OPT_SPECULATIVE, 0)
        core.set_option(OPT_INNOVATION_STATS, 1 if stats else 0)
        core.set_state(*orun.state0)
        core.set_sigma(orun.Sigma0)
        out = dict(results=[], innovation=[], after=[])
        for fr in orun.frames:
            out["results"].append(drive_frame(core, sc, fr))
            out["innovation"].append(core.last_innovation() if stats else None)
            out["after"].append((core.get_state(), core.state_estimate(), core.get_sigma()))
        out["totals"] = core.innovation_totals()
        out["counters"] = cs.read_counters(core)
        return out
    finally:
        core.close()
