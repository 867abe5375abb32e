"""EQF_OPT_CHECK_FINITE (include/eqf_hip.h) against the reference's assert(!Sigma.hasNaN()) behind its three Riccati integrations and its update
(VIO_eqf.cpp:71, 90, 102, 133), on the planted cases of tests/nonfinite_cases.py - every label there is the ORACLE's verdict behind the same call
(tests/test_nonfinite_cases.py shows that on the CPU). Checked here:

 * a reported case returns EQF_E_NONFINITE from THAT call with the option on, and 0 with the option off; a measured landmark's variance: never 0;
 * a clean twin returns 0 with the option on, state and Sigma bit-identical to the option off, and agrees with the oracle through the bounds the suite already
   has (test_gpu_parity.check_sigma / check_state at 1e-9; 5e-9 for the discrete mode's differencing, as test_riccati_discrete; 1e-4 on Sigma under the float
   stores, as test_gpu_fp32_sigma);
 * no verdict outlives its call: -1, repair with eqf_set_state + eqf_set_sigma, the same call again returns 0 - also where nothing but propagations runs in
   between, so that no measurement kernel clears the device's word, and across switching the option off and on;
 * after -1, eqf_set_state + eqf_set_sigma make the context equal to a fresh one: a propagation and an update bit for bit, and the same counters;
 * rows and columns beyond n that a removed landmark left behind are not scanned.
Every test is one or two frames at N <= 86."""
import numpy as np
import pytest

import nonfinite_cases as nc
from context_scenarios import CHART_NAMES, read_counters
from eqvio_amd.capi import OPT_CHECK_FINITE, OPT_FUSED_ASSEMBLY, OPT_RICCATI_DENSE, OPT_SIGMA_FP32, EqfError
from test_gpu_parity import check_sigma, check_state, make_pair
from util import rel_fro

pytestmark = pytest.mark.gpu

NONFINITE = -1  # EQF_E_NONFINITE
DISCRETE_TOL = 5e-9  # test_gpu_parity.test_riccati_discrete: the central differences' rounding noise
FP32_SIGMA_TOL = 1e-4  # test_gpu_fp32_sigma: Sigma under a float store against the fp64 oracle


def context(case, check, Sigma=None):
    """a context with the case's state, its options and Sigma (default: the clean one)"""
    inp = nc.inputs(case)
    _, _, _, core, data = make_pair(CHART_NAMES[case.chart], case.N, case.seed, useDiscreteInnovationLift=0)
    assert np.array_equal(data[5], inp.S) and np.array_equal(data[2], inp.state[2])  # the helper's state is make_pair's
    set_call_options(core, case.call)
    if case.fp32:
        core.set_option(OPT_SIGMA_FP32, case.fp32)
    core.set_option(OPT_CHECK_FINITE, check)
    if Sigma is not None or case.fp32:
        core.set_sigma(inp.S if Sigma is None else Sigma)
    return core


def set_call_options(core, call):
    core.set_option(OPT_FUSED_ASSEMBLY, 0 if call == "fast_unfused" else 1)
    core.set_option(OPT_RICCATI_DENSE, 1 if call == "fast_dense" else 0)


def run(core, case, call=None):
    """the case's call; returns its status"""
    inp, call = nc.inputs(case), call or case.call
    s = inp.settings
    Qd, Pd = s.input_gain_diag12(), s.state_gain_diag8()
    try:
        if call in ("fast", "fast_unfused", "fast_dense", "staged_propagate"):
            if call == "staged_propagate":
                core.stage_measurement(inp.mid, inp.y)
            core.propagate_fast(inp.imu, nc.DT, Qd, Pd, inp.imu[None, :], np.array([nc.DT]), True)
        elif call == "riccati_fast":
            core.integrate_riccati_fast(inp.imu, nc.DT, Qd, Pd)
        elif call == "accurate":
            core.integrate_riccati_accurate(inp.imu, nc.DT, Qd, Pd)
        elif call == "discrete":
            core.integrate_riccati_discrete(inp.imu, nc.DT, Qd, Pd)
        else:
            core.vision_update(inp.cam, inp.mid, inp.y, s.measurementNoise**2, True, False)
        core.synchronize()
    except EqfError as e:
        return e.code
    return 0


def restore(core, case):
    """what the header promises makes a context good again"""
    inp = nc.inputs(case)
    core.set_state(*inp.state)
    core.set_sigma(inp.S)


_oracles = {}


def oracle_behind(case):
    """the oracle behind the clean twin's call: computed once, shared, never modified"""
    t = case.twin()
    key = (t.chart, t.N, nc.ORACLE_OF[t.call], tuple(nc.measured(t)))
    if key not in _oracles:
        orc = nc.oracle_for(t)
        nc.apply_oracle(orc, t)
        _oracles[key] = orc
    return _oracles[key]


def check_against_oracle(core, case):
    orc = oracle_behind(case)
    if case.fp32:
        Sg, So = core.get_sigma(), orc.get_sigma()
        assert np.all(np.isfinite(Sg)) and rel_fro(Sg, So) <= FP32_SIGMA_TOL, rel_fro(Sg, So)
        if case.call not in nc.UPDATES:  # (a propagation's state does not depend on Sigma)
            check_state(core, orc)
        return
    check_sigma(core, orc, DISCRETE_TOL if case.call == "discrete" else 1e-9)
    check_state(core, orc)


def snapshot(core):
    return [core.get_sigma()] + list(core.get_state())


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("case", nc.REPORTED, ids=lambda c: c.id)
def test_planted_value_is_reported_by_the_call_that_meets_it(case):
    core = context(case, 1, nc.planted_sigma(case))
    rc = run(core, case)
    if nc.label(case) == "nonzero":
        assert rc in (NONFINITE, -2), rc  # the pivot test may see a measured landmark's variance first (EQF_E_NOT_SPD)
    else:
        assert rc == NONFINITE, rc
    # the option off: today's behaviour, kept - the call goes through
    core = context(case, 0, nc.planted_sigma(case))
    rc = run(core, case)
    if nc.label(case) == "nonzero":
        assert rc in (0, NONFINITE, -2)  # (Gamma's sensor entries and the pivots are looked at with the option on or off)
    else:
        assert rc == 0, rc


@pytest.mark.parametrize("case", nc.TWINS, ids=lambda c: c.id)
def test_clean_twin_passes_and_the_check_changes_nothing(case):
    on = context(case, 1)
    off = context(case, 0)
    assert run(on, case) == 0
    assert run(off, case) == 0
    assert same(snapshot(on), snapshot(off))
    check_against_oracle(on, case)


def representative(call, chart="invdepth"):
    return nc.Case(chart, 79, call, "nan", "last_diag")


@pytest.mark.parametrize("call", nc.CALLS)
def test_no_stale_verdict(call):
    """-1, repair, the same call: 0 and the oracle's numbers; a third call: 0"""
    case = representative(call)
    assert case in nc.REPORTED
    core = context(case, 1, nc.planted_sigma(case))
    assert run(core, case) == NONFINITE
    restore(core, case)
    assert run(core, case) == 0
    check_against_oracle(core, case)
    assert run(core, case) == 0
    assert np.all(np.isfinite(core.get_sigma()))


def test_no_stale_verdict_across_modes_with_only_propagations_in_between():
    """accurate on a planted Sigma, then the dense fast mode and the discrete mode on the repaired one: none of the three launches a kernel that clears the
    status words"""
    case = representative("accurate")
    core = context(case, 1, nc.planted_sigma(case))
    assert run(core, case) == NONFINITE
    core.set_sigma(nc.inputs(case).S)  # (the Riccati call has not moved X)
    set_call_options(core, "fast_dense")
    assert run(core, case, "fast_dense") == 0
    assert run(core, case, "discrete") == 0
    assert np.all(np.isfinite(core.get_sigma()))


def test_option_off_and_on_again_does_not_resurrect_a_verdict():
    case = representative("fast_dense")
    core = context(case, 1, nc.planted_sigma(case))
    assert run(core, case) == NONFINITE
    core.set_option(OPT_CHECK_FINITE, 0)
    restore(core, case)
    assert run(core, case) == 0
    core.set_option(OPT_CHECK_FINITE, 1)
    assert run(core, case) == 0
    assert run(core, case, "riccati_fast") == 0  # (still the dense mode: the option is the context's)
    assert np.all(np.isfinite(core.get_sigma()))


@pytest.mark.parametrize("call", nc.CALLS)
def test_context_is_as_new_after_set_state_and_set_sigma(call):
    """after EQF_E_NONFINITE Sigma and X are as the failed step left them; eqf_set_state + eqf_set_sigma make the context equal to one that never saw the bad
    matrix: the case's own call and then an update, bit for bit (Sigma, state, Gamma, estimate), and the same counters for those two calls"""
    case = representative(call)
    upd = representative("update_la")
    bad = context(case, 1, nc.planted_sigma(case))
    assert run(bad, case) == NONFINITE
    restore(bad, case)
    fresh = context(case, 1, nc.inputs(case).S)
    before = [read_counters(c) for c in (bad, fresh)]
    for c in (bad, fresh):
        assert run(c, case) == 0
        assert run(c, upd, "update_la") == 0
    assert same(snapshot(bad), snapshot(fresh))
    assert np.array_equal(bad.last_gamma(), fresh.last_gamma())
    assert same(bad.state_estimate(), fresh.state_estimate())
    deltas = [{k: v - b[k] for k, v in read_counters(c).items()} for c, b in zip((bad, fresh), before)]
    assert deltas[0] == deltas[1], deltas


@pytest.mark.parametrize("call", ["fast", "accurate", "update_la"])
def test_storage_a_removed_landmark_leaves_behind_is_not_scanned(call):
    """NaN in every row and column of the last landmark (its own block, its cross blocks with the sensor and with every other landmark); the landmark is removed:
    Sigma is 255 x 255 and clean, the NaN stay in the buffers beyond it. The oracle gets the same removal."""
    case = nc.Case("invdepth", 79, call, "none", "none")
    inp = nc.inputs(case)
    S = inp.S.copy()
    S[case.n - 3:, :] = np.nan
    S[:, case.n - 3:] = np.nan
    core = context(case, 1, S)
    orc = nc.oracle_for(case, S)
    core.remove_landmarks(np.array([case.N - 1], np.int32))
    orc.remove_landmark_by_index(case.N - 1)
    nc.apply_oracle(orc, case)
    assert np.all(np.isfinite(orc.get_sigma())) and orc.get_sigma().shape == (255, 255)
    assert run(core, case) == 0
    check_sigma(core, orc)
    check_state(core, orc)
