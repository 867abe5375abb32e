"""The planted frames of tests/riccati_cases.py for the filter batch's discrete-state-matrix mode (helper module, not a test): eqf_batch_step_discrete /
k_batch_discrete (eqvio_amd/csrc/eqf_batch.hpp). The cases are riccati_cases's as they are; what is added here is the oracle of the third propagation.

 * oracle_settings(s) is s with fastRiccati = 0 and useDiscreteStateMatrix = 1: what a discrete slot's oracle runs with. The batch's own settings keep
   fastRiccati = 1 and do not read useDiscreteStateMatrix.
 * walk(settings, sc, mode) takes a case through the oracle's VIO_eqf calls sample by sample - integrateUpToTime - with the Riccati step of `mode`.
 * TOL_SHORT / TOL_FRAME are the project's bounds for this mode (tests/test_gpu_parity.py::test_riccati_discrete, tests/test_gpu_filter.py::
   test_discrete_state_matrix_filter_run): A_d is a central difference with h = cbrt(eps) = 6e-6 in the reference itself, whose rounding noise eps / h per entry
   is the reference's own; tol(sc) picks the bound by the number of samples that move Sigma."""
import riccati_cases as rc
from oracle_binding import OracleFilter
from util import imu_selection

TOL_SHORT = 5e-9  # Sigma, relative, after a propagation of at most two samples
TOL_FRAME = 1e-8  # state and Sigma after a ten-sample walk or a whole frame, teacher forced


def oracle_settings(s):
    o = rc.oracle_settings(s)
    o.useDiscreteStateMatrix = 1
    return o


def tol(sc):
    return TOL_SHORT if rc.expected_samples(sc) <= 2 else TOL_FRAME


def walk(settings, sc, mode="discrete"):
    """integrateUpToTime by the oracle's VIO_eqf calls: mode "fast" (one Riccati step with the mean sample in front), "accurate" or "discrete" (one per
    sample with dt > 0, between the observer steps)."""
    orc = OracleFilter(settings)
    orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    dts, mean, total = imu_selection(sc.imus, sc.t0, sc.stamp)
    if mode == "fast":
        orc.integrate_riccati_fast(mean, total)
    for u, dt in zip(sc.imus, dts):
        if dt > 0 and mode == "accurate":
            orc.integrate_riccati_accurate(u, dt)
        elif dt > 0 and mode == "discrete":
            orc.integrate_riccati_discrete(u, dt)
        orc.integrate_observer(u, dt, bool(settings.useDiscreteVelocityLift))
    return orc


def whole_frame(settings, sc):
    """the case through the oracle's filter: processIMUData for every sample, then processVisionData"""
    orc = OracleFilter(settings)
    orc.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    for u in sc.imus:
        orc.process_imu(u)
    orc.process_vision(sc.stamp, sc.cam, sc.mid, sc.y)
    return orc
