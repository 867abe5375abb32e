"""50-digit truth for ONE planted frame of the filter batch at its size limit: N = 64 landmarks, all 64 measured (m = 128 rows of S, state dimension 213),
InvDepth chart, with the reference's *template* noise values (point variance 5000, pixel noise 0.003; tests/golden/make_truth_mp.py) that make cond(Sigma+) large.
Generator of tests/golden/truth_batch_N64.npz, the yardstick of tests/test_truth_batch_mp.py.

The frame is what one processVisionData call does with fast Riccati and no landmark turnover (thresholds 1e8): riccati_fast with the mean IMU sample, the k
discrete-lift observer steps, vision_update (equivariant output, discrete innovation lift). It is evaluated by the independent restatement
oracle/indep/eqvio_ref.py in mpmath at 50 digits, formulas as written (LU inverse, Sigma - K C Sigma). Every input is an fp64 number held by the fixture: the
planted state and the planted Sigma (see inputs(): ill-conditioned, exactly symmetric), the IMU samples and their stamps, the dts and the mean sample as the
filter's IMU selection computes them in fp64, and the pixels. Symmetric matrices are stored as lower triangles (tri_pack / tri_unpack).

Run (pure-Python mpmath, several minutes, CPU only):  python tests/golden/make_truth_batch_mp.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "indep"))

from make_truth_mp import CAM, TEMPLATE  # noqa: E402

N, OBS_STEPS, WARMUP = 64, 2, 1
T0, STAMP = 1.0, 1.05
PATH = os.path.join(HERE, "truth_batch_N64.npz")
GENERATOR = "oracle/indep/eqvio_ref.py, mpmath 50 digits, tests/golden/make_truth_batch_mp.py"


def tri_pack(S):
    return np.ascontiguousarray(S[np.tril_indices(S.shape[0])])


def tri_unpack(v):
    n = int(round((np.sqrt(8 * len(v) + 1) - 1) / 2))
    S = np.zeros((n, n))
    S[np.tril_indices(n)] = v
    return S + np.tril(S, -1).T


def template_settings():
    """the filter settings of the frame (tests/test_truth_batch_mp.py builds the same from the fixture)"""
    from eqvio_amd.capi import COORD_INVDEPTH
    from util import settings_for

    s = settings_for(COORD_INVDEPTH, fastRiccati=1, useDiscreteInnovationLift=1, useDiscreteVelocityLift=1, useEquivariantOutput=1, measurementNoise=TEMPLATE["meas_noise"])
    (s.biasOmegaProcessVariance, s.biasAccelProcessVariance, s.attitudeProcessVariance, s.positionProcessVariance, s.velocityProcessVariance,
     s.cameraAttitudeProcessVariance, s.cameraPositionProcessVariance, s.pointProcessVariance) = TEMPLATE["proc8"]
    s.velGyrNoise = s.velAccNoise = s.velGyrBiasWalk = s.velAccBiasWalk = float(np.sqrt(TEMPLATE["qin12"][0]))
    return s


def inputs():
    """fp64 inputs of the frame (numpy PRNG, seed fixed). The planted state and Sigma are where WARMUP frames of the same kind leave a filter that starts from
    the template's diagonal covariance (walked in fp64 by the CPU oracle's symmetric arithmetic): the landmark depths have begun to resolve, Sigma is
    ill-conditioned and its large entries still change in the frame, which is where fp64 evaluations part from the truth."""
    from eqvio_amd.capi import Camera
    from oracle_binding import ARITH_EFFICIENT, OracleFilter
    from util import estimate_landmarks, imu_selection, project, random_imu, reasonable_state

    rng = np.random.default_rng(6464)
    xi0, Xs, ids, q0, Q = reasonable_state(rng, N)
    i = TEMPLATE["init"]
    d = np.array([i["biasOmega"]] * 3 + [i["biasAccel"]] * 3 + [i["attitude"]] * 3 + [i["position"]] * 3 + [i["velocity"]] * 3 + [i["cameraAttitude"]] * 3 +
                 [i["cameraPosition"]] * 3 + [i["point"]] * (3 * N))
    scale, g = np.array([1] + [0.05] * 3 + [0.2] * 3 + [0] * 6), np.array([0] * 4 + [0, 0, 9.0] + [0] * 6)
    cam = Camera.pinhole(*CAM, 752, 480)
    orc = OracleFilter(template_settings())
    orc.set_arithmetic(ARITH_EFFICIENT)
    orc.set_eqf(xi0, Xs, ids, q0, Q, np.diag(d))

    def pixels():
        _, _, _, q0_, Q_ = orc.get_eqf()
        return (project(cam, estimate_landmarks(q0_, Q_)) + rng.normal(size=(N, 2)) * TEMPLATE["meas_noise"]).reshape(-1)  # ids ascend with the index

    for f in range(WARMUP):
        orc.integrate_riccati_fast(random_imu(rng) * scale + g, 0.05)
        for _ in range(OBS_STEPS):
            orc.integrate_observer(random_imu(rng) * scale + g, 0.025, True)
        orc.vision_update(cam, ids, pixels())
    xi0, Xs, ids, q0, Q = orc.get_eqf()
    S0 = orc.get_sigma()
    S0 = np.tril(S0) + np.tril(S0, -1).T
    imus = np.stack([random_imu(rng, stamp=T0 + 0.025 * s) * scale + g for s in range(OBS_STEPS)])
    dts, mean, total = imu_selection(imus, T0, STAMP)
    for u, dt in zip(imus, dts):  # the measurement is taken where the observer steps of the frame leave the estimate
        orc.integrate_observer(u, dt, True)
    return dict(xi0=xi0, Xs=Xs, ids=ids, q0=q0, Q=Q, Sigma0=S0, imus=imus, dts=dts, imu_mean=mean, dt_total=np.float64(total), t0=np.float64(T0),
                stamp=np.float64(STAMP), meas_ids=ids.copy(), meas_y=pixels())


def run_frame(r, inp):
    """The frame in r's arithmetic: Sigma+, Gamma and the group after the update (flat)."""
    from eqvio_ref import Camera

    o = r.o
    X = r.group_from_flat(inp["Xs"], inp["ids"], inp["Q"])
    xi0 = r.state_from_flat(inp["xi0"], inp["ids"], inp["q0"])
    S = o.arr(inp["Sigma0"])
    Qin, P = r.diag(TEMPLATE["qin12"]), r.state_gain(TEMPLATE["proc8"], N)
    S = r.riccati_fast("invdepth", X, xi0, S, r.imu_from_flat(inp["imu_mean"]), o.s(float(inp["dt_total"])), Qin, P)
    for k in range(len(inp["imus"])):
        X = r.integrate_observer(X, xi0, r.imu_from_flat(inp["imus"][k]), o.s(float(inp["dts"][k])), True)
    X, S, g = r.vision_update("invdepth", X, xi0, S, Camera(0, *CAM), r.meas_from_flat(inp["meas_ids"], inp["meas_y"]), o.s(TEMPLATE["meas_noise"]) ** 2, True, True)
    Xs, Q = r.group_to_flat(X)
    return dict(Sigma=o.tofloat(S), Gamma=o.tofloat(g), Xs=Xs, Q=Q)


if __name__ == "__main__":
    if os.path.exists(PATH) and "--force" not in sys.argv:
        print(PATH, "exists (use --force to regenerate)")
        sys.exit(0)
    from eqvio_ref import MP, EqVIORef

    inp = inputs()
    t0 = time.time()
    truth = run_frame(EqVIORef(MP(50)), inp)
    print(f"mp50 frame: {time.time() - t0:.0f} s")
    S = truth["Sigma"]
    asym = np.linalg.norm(S - S.T) / np.linalg.norm(S)
    assert asym < 1e-15, asym  # the exact answer is symmetric: only the rounding to fp64 of the two halves may differ
    out = {k: v for k, v in inp.items() if k != "Sigma0"}
    out.update(Sigma0_tril=tri_pack(inp["Sigma0"]), truth_Sigma_tril=tri_pack(S), truth_Gamma=truth["Gamma"], truth_Xs=truth["Xs"],
               truth_Q=truth["Q"], cam=np.array(CAM), proc8=np.array(TEMPLATE["proc8"]), qin12=np.array(TEMPLATE["qin12"]),
               meas_var=np.float64(TEMPLATE["meas_noise"] ** 2), generator=np.array(GENERATOR))
    assert np.array_equal(tri_unpack(out["Sigma0_tril"]), inp["Sigma0"])
    np.savez_compressed(PATH, **out)
    w = np.linalg.eigvalsh(tri_unpack(out["truth_Sigma_tril"]))
    print(PATH, os.path.getsize(PATH) // 1024, "KiB; cond(Sigma+) =", w[-1] / w[0])
