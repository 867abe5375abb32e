"""Per-slot settings of the filter batch (helper module, not a test): the cases of ONE step in which every slot runs its own tuning. A case is a slot's
settings (the batch's shipped EuRoC / InvDepth settings with one thing changed) and a planted frame (tests/batch_scenarios.py) on which that thing matters.
`other` names what the case is told apart from: the batch's settings (what a kernel that ignored the slot's settings would run with) or, for the three
outlier-cap slots that share one frame, the next cap.

tests/test_batch_slot_settings_api.py shows on the CPU oracle alone that every case differs from its `other` by far more than the 1e-9 the GPU test
(tests/test_gpu_batch_slot_settings.py) holds each slot to against ITS OWN oracle."""
from dataclasses import dataclass

import numpy as np

import batch_scenarios as bs
from eqvio_amd.capi import COORD_EUCLIDEAN, Settings
from oracle_binding import OracleFilter

IMU_NOISES = dict(velGyrNoise=0.3, velAccNoise=0.8, velGyrBiasWalk=0.2, velAccBiasWalk=0.5)
PROCESS_VARIANCES = dict(biasOmegaProcessVariance=0.11, biasAccelProcessVariance=0.23, attitudeProcessVariance=0.31, positionProcessVariance=0.43,
                         velocityProcessVariance=0.59, cameraAttitudeProcessVariance=0.67, cameraPositionProcessVariance=0.73, pointProcessVariance=0.89)
# the ranking frame: N = 16, 3 absolute and 2 probabilistic-only outliers (pointProcessVariance 1e-8 keeps the planted-small rows small, as bs.RANK_SETTINGS)
RANK_ABS, RANK_PROB, RANK_N = [(15, 14.0), (2, 9.0), (8, 11.0)], [(0, 3.0), (7, 4.0)], 16
CAPS = (0, 2, 5)


def clone(s, **kw):
    c = Settings.from_buffer_copy(s)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def same_bytes(a, b):
    return bytes(a) == bytes(b)


@dataclass
class Case:
    name: str
    settings: Settings   # the slot's own
    sc: bs.Scenario
    other: Settings      # what the case must be told apart from, on the same frame
    kind: str = "sigma"  # how: "sigma" (Sigma+ beyond 1e-6 relative), "discards", "depth", "ids", "state" (the lift: it never reaches Sigma)
    call: bool = True    # False: the slot is never given settings


def tracking(S):
    """Sigma of a filter that is tracking: the planted random SPD matrix scaled down, so that R, the output approximation and the observer's lift weigh in
    Sigma+ (at the planted scale S = C Sigma C^T dwarfs R and the update is a projection whatever the settings)"""
    S *= 1e-5


def rank_settings(base, cap):
    return clone(base, featureRetention=bs.retention_for(cap, RANK_N), **bs.RANK_SETTINGS)


_cases = None


def cases():
    """built once per process; base is bs.shipped_euroc()"""
    global _cases
    if _cases is not None:
        return _cases
    base = bs.shipped_euroc()
    out = []

    def add(name, kw, make_kw, kind="sigma", other=None, call=True, N=12, seed=None):
        s = clone(base, **kw)
        sc = bs.make(s, name, 9000 + len(out) if seed is None else seed, N, **{"sigma_edit": tracking, **make_kw})
        out.append(Case(name, s, sc, base if other is None else other, kind, call))

    add("unmodified", {}, {}, call=False)
    add("equal_to_batch", {}, {})
    add("measurementNoise", dict(measurementNoise=0.4), {})
    add("imu_noises", IMU_NOISES, {})
    add("process_variances", PROCESS_VARIANCES, {})
    for i, cap in enumerate(CAPS):  # one frame, three caps: told apart from the next cap
        s = rank_settings(base, cap)
        sc = bs.make(s, f"cap{cap}", 9100, RANK_N, abs_out=RANK_ABS, prob_out=RANK_PROB, noise_px=0.2)
        out.append(Case(f"cap{cap}", s, sc, rank_settings(base, CAPS[(i + 1) % len(CAPS)]), "discards"))
    # the thresholds themselves: nothing is a candidate any more, against the same cap with the batch's thresholds
    s = clone(rank_settings(base, 5), outlierThresholdAbs=1e8, outlierThresholdProb=1e8)
    out.append(Case("thresholds", s, bs.make(s, "thresholds", 9100, RANK_N, abs_out=RANK_ABS, prob_out=RANK_PROB, noise_px=0.2), rank_settings(base, 5), "discards"))
    add("useEquivariantOutput", dict(useEquivariantOutput=0), {})
    add("useDiscreteInnovationLift", dict(useDiscreteInnovationLift=1), dict(sigma_edit=None, noise_px=1.5), "state")  # the shipped settings have 0: the slot runs the other lift
    add("useDiscreteVelocityLift", dict(useDiscreteVelocityLift=0), dict(k=2))
    add("fixed_depth", dict(useMedianDepth=0, initialSceneDepth=7.5, initialPointVariance=0.2), dict(measured=[i for i in range(12) if i not in (1, 6, 10)], new=3), "depth")
    add("median_depth", dict(useMedianDepth=1), dict(measured=[i for i in range(12) if i not in (1, 6, 10)], new=3), "depth")
    add("removeLostLandmarks", dict(removeLostLandmarks=0), dict(measured=bs.spread(12, 5)), "ids")
    add("euclidean", dict(coordinateChoice=COORD_EUCLIDEAN), dict(sigma_edit=None))
    add("unmodified_b", {}, {}, call=False, N=17)
    _cases = (base, out)
    return _cases


def oracle_frame(settings, sc):
    """the scenario through a full oracle with these settings; returns the oracle"""
    orc = OracleFilter(settings)
    orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    for u in sc.imus:
        orc.process_imu(u)
    orc.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
    return orc


def new_depth(orc, sc):
    """the depth the oracle gave the frame's first new landmark: |origin point| / |bearing|"""
    new = sc.plan["new"][0]
    _, _, ids, q0, _ = orc.get_eqf()
    i, j = list(ids).index(new), list(sc.mid).index(new)
    return float(np.linalg.norm(q0[i]) / np.linalg.norm(bs.oracle_cam_undistort(sc.cam, sc.y[2 * j:2 * j + 2])))
