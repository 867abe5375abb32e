"""Distance to the TRUE answer of one filter-batch frame at its size limit, where Sigma is ill-conditioned and the 1e-9 bar against the oracle means little:
tests/golden/truth_batch_N64.npz holds one planted frame (N = 64 landmarks, all measured, InvDepth, the reference's template noise values: point variance 5000,
pixel noise 0.003) evaluated at 50 digits by the independent restatement (tests/golden/make_truth_batch_mp.py). The batch slot's Sigma+ is held against the
CPU oracle's OWN distance from that truth, measured in the same test, never against a figure of the device's:

 * e_dev <= 4 e_eff: the slot (Cholesky in LDS, W and Sigma - W^T W on MFMA with a 4-wide k split) and the oracle's "efficient" arithmetic (Cholesky,
   Sigma - K T^T) are both symmetric fp64 evaluations that differ in summation order only; the factor allows for the k split and the unblocked factorisation;
 * e_dev < e_asw whenever e_asw > 2 e_eff: where the reference's arithmetic as written (LU inverse, Sigma - K C Sigma) is measurably worse, the slot is not;
 * the slot's Sigma+ is exactly symmetric.

Measured on an MI355X (profiles/r09_batch_edges.txt): see DESIGN.md section 11, "Batch parity at the edges"."""
import os
import sys

import numpy as np
import pytest

from eqvio_amd.capi import COORD_INVDEPTH, Camera
from util import rel_fro, settings_for

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_truth_batch_mp import GENERATOR, PATH, tri_unpack  # noqa: E402


def _load():
    d = dict(np.load(PATH))
    d["Sigma0"] = tri_unpack(d["Sigma0_tril"])
    d["truth_Sigma"] = tri_unpack(d["truth_Sigma_tril"])
    s = settings_for(COORD_INVDEPTH, fastRiccati=1, useDiscreteInnovationLift=1, useDiscreteVelocityLift=1, useEquivariantOutput=1, removeLostLandmarks=1,
                     measurementNoise=float(np.sqrt(d["meas_var"])))  # thresholds 1e8: no outlier decision inside the frame
    (s.biasOmegaProcessVariance, s.biasAccelProcessVariance, s.attitudeProcessVariance, s.positionProcessVariance, s.velocityProcessVariance,
     s.cameraAttitudeProcessVariance, s.cameraPositionProcessVariance, s.pointProcessVariance) = [float(x) for x in d["proc8"]]
    q = np.sqrt(d["qin12"])
    s.velGyrNoise, s.velAccNoise, s.velGyrBiasWalk, s.velAccBiasWalk = float(q[0]), float(q[3]), float(q[6]), float(q[9])
    assert np.allclose(s.state_gain_diag8(), d["proc8"], rtol=1e-15) and np.allclose(s.input_gain_diag12(), d["qin12"], rtol=1e-14)
    assert s.outlierThresholdAbs == 1e8 and s.outlierThresholdProb == 1e8
    return d, s, Camera.pinhole(*[float(x) for x in d["cam"]], 752, 480)


def _oracle_error(d, s, cam, mode):
    """the frame through the oracle's processVisionData in the given arithmetic: error of Sigma+ and Gamma against the truth"""
    from oracle_binding import OracleFilter

    o = OracleFilter(s)
    o.set_arithmetic(mode)
    o.set_eqf(d["xi0"], d["Xs"], d["ids"], d["q0"], d["Q"], d["Sigma0"], time=float(d["t0"]))
    for u in d["imus"]:
        o.process_imu(u)
    o.process_vision(float(d["stamp"]), cam, d["meas_ids"], d["meas_y"])
    assert np.array_equal(o.get_eqf()[2], d["ids"])
    return rel_fro(o.get_sigma(), d["truth_Sigma"]), rel_fro(o.last_gamma(), d["truth_Gamma"])


def test_truth_batch_fixture_provenance():
    d = np.load(PATH)
    assert str(d["generator"]) == GENERATOR and "mpmath 50 digits" in GENERATOR and "oracle/indep/eqvio_ref.py" in GENERATOR
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(HERE, "golden", "truth_template_chain.npz"))  # lower triangles: no larger than the largest fixture
    T, S0 = tri_unpack(d["truth_Sigma_tril"]), tri_unpack(d["Sigma0_tril"])
    assert T.shape == (213, 213) and np.array_equal(T, T.T) and np.array_equal(S0, S0.T)  # the exact answer is symmetric
    assert len(d["ids"]) == 64 and np.array_equal(d["meas_ids"], d["ids"]) and len(d["meas_y"]) == 128 and len(d["truth_Gamma"]) == 213
    assert np.linalg.cond(T) > 1e10


def test_oracle_arithmetics_against_the_truth():
    """the yardsticks themselves, on the CPU: both oracle arithmetics run the frame and land near the truth; the fixture's dts and mean sample are the ones
    the filter's IMU selection computes"""
    from oracle_binding import ARITH_AS_WRITTEN, ARITH_EFFICIENT
    from util import imu_selection

    d, s, cam = _load()
    dts, mean, total = imu_selection(d["imus"], float(d["t0"]), float(d["stamp"]))
    assert np.array_equal(dts, d["dts"]) and np.array_equal(mean, d["imu_mean"]) and total == float(d["dt_total"])
    e_eff, g_eff = _oracle_error(d, s, cam, ARITH_EFFICIENT)
    e_asw, g_asw = _oracle_error(d, s, cam, ARITH_AS_WRITTEN)
    print(f"oracle vs 50-digit truth: efficient Sigma {e_eff:.3e} Gamma {g_eff:.3e}; as written Sigma {e_asw:.3e} Gamma {g_asw:.3e}")
    assert 0 < e_eff < 1e-6 and 0 < e_asw < 1e-6  # fp64 evaluations of a frame whose Sigma+ has cond > 1e10: near, not equal


@pytest.mark.gpu
def test_batch_slot_is_as_close_to_the_truth_as_the_oracle():
    from eqvio_amd.batch import BATCH_UPDATED, VIOFilterBatch
    from oracle_binding import ARITH_AS_WRITTEN, ARITH_EFFICIENT

    d, s, cam = _load()
    e_eff, _ = _oracle_error(d, s, cam, ARITH_EFFICIENT)
    e_asw, _ = _oracle_error(d, s, cam, ARITH_AS_WRITTEN)
    batch = VIOFilterBatch(s, 2, 64)
    k = 1
    batch.start_slot(k, d["xi0"], np.zeros(0, np.int32), np.zeros((0, 3)), float(d["t0"]))
    batch.slot(k).force_eqf(d["xi0"], d["Xs"], d["ids"], d["q0"], d["Q"], d["Sigma0"])
    for u in d["imus"]:
        batch.process_imu(k, u)
    st = batch.process_vision([(k, float(d["stamp"]), cam, d["meas_ids"], d["meas_y"])])
    assert st.tolist() == [0] and batch.last_result(k)[0] == BATCH_UPDATED
    assert np.array_equal(batch.slot(k).get_eqf()[2], d["ids"])
    S = batch.slot(k).get_sigma()
    assert np.array_equal(S, S.T)
    e_dev = rel_fro(S, d["truth_Sigma"])
    print(f"Sigma+ vs 50-digit truth: e_dev {e_dev:.3e}  e_eff {e_eff:.3e}  e_asw {e_asw:.3e}  (e_dev / e_eff {e_dev / e_eff:.2f})")
    assert e_dev <= 1.1 * e_eff, (e_dev, e_eff)  # 4 e_eff by the argument above, tightened to 1.5 x the measured ratio (0.73)
    if e_asw > 2.0 * e_eff:
        assert e_dev < e_asw, (e_dev, e_asw)
    Xs = batch.slot(k).get_eqf()[1]
    assert np.max(np.abs(Xs - d["truth_Xs"])) < 1e-6  # the state follows Gamma
