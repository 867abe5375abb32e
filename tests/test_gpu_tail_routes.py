"""The option-dependent branches of the vision update's tail - everything from the mapped measurement to the applied lift - one at a time and in the pairs that share
a rule, at the smallest sizes at which each form exists: 2 panels (launch chain), 3 panels (the smallest look-ahead instantiation; ZB = 2, then 3, on the staged
pair) and one 3-panel frame whose outlier decision is taken on the device (context_scenarios.py). For every (scenario, option set):

 (a) parity with the CPU oracle at the suite's flat 1e-9 (test_gpu_context_sizes.compare; the removed set and the statistics for the select scenario; SURVEY's
     bounds of test_gpu_fp32_sigma.py where Sigma is stored as float),
 (b) bit-identity with the default-options run of the same scenario, wherever the options only move work between launches (NOT_BIT_IDENTICAL names the rest
     and the arithmetic that differs),
 (c) the device's counters against COUNTERS below, which is derived from the rules in eqf_hip.hip (plan_tail; stats_then_update's routes) and not from a run.

The frames are driven through the public C-ABI the way a caller must: a statistics call that reports "not updated" is followed by eqf_vision_update (plain
statistics: EQF_OPT_SPECULATIVE = 0, EQF_OPT_CHECK_FINITE = 1), a cancelled speculative tail by the same call again (the back-off then takes the device-side
decision). Nothing here shortens a device-side wait or makes the look-ahead kernel give up: test_stalled_lookahead_* cover that route."""
import numpy as np
import pytest

import context_scenarios as cs
from eqvio_amd.capi import (OPT_CHECK_FINITE, OPT_DOORBELL, OPT_EARLY_DOORBELL, OPT_EARLY_LIFT, OPT_LIFT_WITH_SYRK, OPT_LIVE_COLUMNS_FIRST, OPT_LOOKAHEAD,
                            OPT_MEASURE_IN_PROPAGATE, OPT_SELECT_ONE_WORKGROUP, OPT_SIGMA_FP32, OPT_SPECULATIVE, OPT_TIMING, OPT_Z_IN_LOOKAHEAD, EqfCore)
from oracle_binding import se3_log_dist
from test_gpu_context_sizes import compare
from util import rel_fro

pytestmark = pytest.mark.gpu

SCENARIOS = {"update32": "update_inv_N32", "update33": "update_inv_N33", "staged32": "staged_inv_N32", "staged33": "staged_inv_N33", "select40": "select_inv_N40_M36"}

OPTIONS = {
    "defaults": (),
    "lookahead=0": ((OPT_LOOKAHEAD, 0),),
    "z_in_lookahead=0": ((OPT_Z_IN_LOOKAHEAD, 0),),
    "early_lift=0": ((OPT_EARLY_LIFT, 0),),
    "lift_with_syrk=0": ((OPT_LIFT_WITH_SYRK, 0),),
    "doorbell=0": ((OPT_DOORBELL, 0),),
    "early_doorbell=0": ((OPT_EARLY_DOORBELL, 0),),
    "measure_in_propagate=0": ((OPT_MEASURE_IN_PROPAGATE, 0),),
    "speculative=0": ((OPT_SPECULATIVE, 0),),
    "speculative=1": ((OPT_SPECULATIVE, 1),),  # (differs from the defaults on the select scenario only, which is driven with speculation off)
    "select_one_workgroup=0": ((OPT_SELECT_ONE_WORKGROUP, 0),),
    "live_columns_first=0": ((OPT_LIVE_COLUMNS_FIRST, 0),),
    "check_finite=1": ((OPT_CHECK_FINITE, 1),),
    "timing=1": ((OPT_TIMING, 1),),  # per-kernel timing
    "early_lift=0,lift_with_syrk=0": ((OPT_EARLY_LIFT, 0), (OPT_LIFT_WITH_SYRK, 0)),
    "lookahead=0,z_in_lookahead=0": ((OPT_LOOKAHEAD, 0), (OPT_Z_IN_LOOKAHEAD, 0)),
    "check_finite=1,early_doorbell=0": ((OPT_CHECK_FINITE, 1), (OPT_EARLY_DOORBELL, 0)),
    "sigma_fp32=2": ((OPT_SIGMA_FP32, 2),),
}

# ---------------------------------------------------------------------------------------------------------------------------------------------- (c) the counters
# Per scenario with default options; `early` is the number of updates the host takes from the look-ahead kernel's own doorbell: every tail that carries it. (The host
# takes whichever of the two doorbells it sees first; the lift's rings a kernel boundary and a lift later - microseconds - while the host polls both in a loop of
# nanoseconds, so the early one is seen first. Observed on the parent commit and on this one, in every run of all 90 cases: equal to this table.) `upd` is
# what the statistics calls report.
#  update: eqf_vision_update - no measurement fusion (ZB = 1 where the look-ahead kernel runs), no speculation, no early doorbell
#  staged: two speculative tails; frame 1 has no output blocks from the propagation kernel (no camera known yet: ZB = 2 up to 8 panels), frame 2 has (ZB = 3, me)
#  select: speculation off, one frame with the decision on the device (k_stats_select puts the live columns first: live)
ZERO = dict(la=0, zb=0, me=0, calls=0, queued=0, cancelled=0, sel=0, live=0, early=0)
DEFAULT = {
    "update32": dict(ZERO, upd=[]),
    "update33": dict(ZERO, la=1, zb=1, upd=[]),
    "staged32": dict(ZERO, me=1, calls=2, queued=2, upd=[1, 1]),
    "staged33": dict(ZERO, la=2, zb=2, me=1, calls=2, queued=2, early=2, upd=[1, 1]),
    "select40": dict(ZERO, la=1, zb=1, calls=1, sel=1, live=1, early=1, upd=[1]),
}
# What an option set changes, rule by rule:
#  la: EQF_OPT_LOOKAHEAD and 3 .. 32 panels. zb: la, EQF_OPT_Z_IN_LOOKAHEAD, fp64 Sigma; with measurement fusion ZB = 3 needs in_prop, ZB = 2 needs the staged
#  measurement and EQF_OPT_EARLY_LIFT. in_prop (me): fusion, EQF_OPT_MEASURE_IN_PROPAGATE, EQF_OPT_EARLY_LIFT, fp64 Sigma - and
#  output blocks from the propagation kernel, which evaluates them under the same options plus EQF_OPT_Z_IN_LOOKAHEAD and no finite check. Speculation: EQF_OPT_SPECULATIVE and
#  no finite check; without it the statistics call only computes statistics (upd 0) and eqf_vision_update takes the remembered output blocks (ZB = 1, no me).
#  early: la, a doorbell wait (EQF_OPT_DOORBELL, no finite check), EQF_OPT_EARLY_DOORBELL, the lift inside the covariance-update launch (EQF_OPT_EARLY_LIFT,
#  EQF_OPT_LIFT_WITH_SYRK, fp64 Sigma, no per-kernel timing), and a caller that can take it (not eqf_vision_update). live: la, k_stats_select (EQF_OPT_SELECT_ONE_WORKGROUP),
#  EQF_OPT_LIVE_COLUMNS_FIRST.
PLAIN32 = dict(me=0, queued=0, upd=[0, 0])
PLAIN33 = dict(me=0, queued=0, early=0, upd=[0, 0])
CHANGES = {
    "lookahead=0": {"update33": dict(la=0, zb=0), "staged33": dict(la=0, zb=0, early=0), "select40": dict(la=0, zb=0, live=0, early=0)},
    # (the propagation kernel evaluates output blocks for the update only where the look-ahead kernel may build Z from them: plan_stage (behind plan_propagation) asks for
    #  EQF_OPT_Z_IN_LOOKAHEAD, fp64 Sigma and no finite check as well - no me without them, whatever factorises)
    "z_in_lookahead=0": {"update33": dict(zb=0), "staged32": dict(me=0), "staged33": dict(zb=0, me=0), "select40": dict(zb=0)},
    "early_lift=0": {"staged32": dict(me=0), "staged33": dict(zb=0, me=0, early=0), "select40": dict(early=0)},
    "lift_with_syrk=0": {"staged33": dict(early=0), "select40": dict(early=0)},
    "doorbell=0": {"staged33": dict(early=0), "select40": dict(early=0)},
    "early_doorbell=0": {"staged33": dict(early=0), "select40": dict(early=0)},
    "measure_in_propagate=0": {"staged32": dict(me=0), "staged33": dict(me=0)},  # (ZB = 2 in both frames)
    "speculative=0": {"staged32": PLAIN32, "staged33": PLAIN33},
    # the speculative tail is cancelled by the planted outliers (la and ZB = 2 were launched), the back-off sends the repeated call to the device-side decision
    "speculative=1": {"select40": dict(la=2, zb=2, calls=2, queued=1, cancelled=1, upd=[0, 1])},
    "select_one_workgroup=0": {"select40": dict(live=0)},
    "live_columns_first=0": {"select40": dict(live=0)},
    "check_finite=1": {"staged32": PLAIN32, "staged33": PLAIN33, "select40": dict(early=0)},
    "timing=1": {"staged33": dict(early=0), "select40": dict(early=0)},
    "sigma_fp32=2": {"update33": dict(zb=0), "staged32": dict(me=0), "staged33": dict(zb=0, me=0, early=0), "select40": dict(zb=0, early=0)},
}
CHANGES["early_lift=0,lift_with_syrk=0"] = CHANGES["early_lift=0"]
CHANGES["lookahead=0,z_in_lookahead=0"] = dict(CHANGES["lookahead=0"], staged32=dict(me=0), staged33=dict(la=0, zb=0, me=0, early=0))
CHANGES["check_finite=1,early_doorbell=0"] = CHANGES["check_finite=1"]
COUNTERS = {(kind, opt): dict(DEFAULT[kind], **CHANGES.get(opt, {}).get(kind, {})) for kind in SCENARIOS for opt in OPTIONS}

# ---------------------------------------------------------------------------------------------------------------------------------------------- (b) bit-identity
# (kind, option set) -> the arithmetic that differs from the default-options run; everything else moves the same operations between launches and is held to
# bit-identity of every frame's state, estimates, Sigma and statistics.
#  GAMMA: Gamma = W z is summed in another order - the look-ahead kernel leaves it complete, the launch chain's last step leaves partial vectors for the lift to add
#  up, and with EQF_OPT_EARLY_LIFT = 0 on the chain it is a by-product of the covariance update's diagonal tiles. W and Sigma+ = Sigma - W W^T do not depend on it:
#  the first frame's Sigma is still bit-identical (the second frame's follows the first frame's lifted state).
#  ORDER: without k_stats_select's reordering the columns of Z are in measurement order, not live columns first: another elimination order.
#  FP32: Sigma is rounded to float on every store.
GAMMA, ORDER, FP32 = "gamma", "order", "fp32"
NOT_BIT_IDENTICAL = {}
for _kind in SCENARIOS:
    NOT_BIT_IDENTICAL[(_kind, "sigma_fp32=2")] = FP32
for _opt in ("early_lift=0", "early_lift=0,lift_with_syrk=0"):  # on the launch chain (2 panels) only: the look-ahead kernel computes Gamma wherever the lift runs
    NOT_BIT_IDENTICAL[("update32", _opt)] = NOT_BIT_IDENTICAL[("staged32", _opt)] = GAMMA
for _opt in ("lookahead=0", "lookahead=0,z_in_lookahead=0"):
    for _kind in ("update33", "staged33", "select40"):
        NOT_BIT_IDENTICAL[(_kind, _opt)] = GAMMA
for _opt in ("select_one_workgroup=0", "live_columns_first=0"):
    NOT_BIT_IDENTICAL[("select40", _opt)] = ORDER

CASES = [(kind, opt) for kind in SCENARIOS for opt in OPTIONS]


def drive(sc, orun, options):
    """context_scenarios.run_device with the caller's half of the statistics calls' contract (module docstring) and every counter read"""
    s = sc.settings()
    cam = cs.CAMERAS[sc.cam]
    Qd, Pd = s.input_gain_diag12(), s.state_gain_diag8()
    var = s.measurementNoise**2
    core = EqfCore(sc.N, cs.CHART_NAMES[sc.chart])
    try:
        if sc.route == "select":
            core.set_option(OPT_SPECULATIVE, 0)  # as run_device: straight to the device-side decision
        for opt, val in options:
            core.set_option(opt, val)
        core.set_state(*orun.state0)
        core.set_sigma(orun.Sigma0)
        out = cs.DeviceRun([], {}, updated=[])
        for fr in orun.frames:
            if sc.route == "update":
                core.integrate_riccati_fast(fr.mean, fr.total, Qd, Pd)
                core.vision_update(cam, fr.mid, fr.y, var, bool(sc.star), bool(sc.lift))
            else:
                core.stage_measurement(fr.mid, fr.y)
                core.propagate_fast(fr.mean, fr.total, Qd, Pd, fr.imus, fr.dts, bool(sc.vel_lift))
                if sc.route == "staged":
                    upd, *out.stats = core.stats_then_update(cam, fr.mid, fr.y, sc.thr_abs, sc.thr_prob, var, bool(sc.star), bool(sc.lift))
                    out.updated.append(upd)
                    if upd == 0:  # statistics only: the caller has no outlier to remove (the thresholds are out of reach) and updates
                        core.vision_update(cam, fr.mid, fr.y, var, bool(sc.star), bool(sc.lift))
                else:
                    for attempt in range(2):
                        upd, a, p, d, out.removed = core.stats_select_update(cam, fr.mid, fr.y, sc.thr_abs, sc.thr_prob, sc.cap, var, bool(sc.star), bool(sc.lift))
                        out.stats = [a, p, d]
                        out.updated.append(upd)
                        if upd != 0:
                            break
            out.after.append((core.get_state(), core.state_estimate(), core.get_sigma()))
        out.counters = cs.read_counters(core, every=True)
        return out
    finally:
        core.close()


_runs = {}


def device_run(kind, opt):
    if (kind, opt) not in _runs:
        sc = cs.BY_NAME[SCENARIOS[kind]]
        _runs[(kind, opt)] = drive(sc, cs.oracle_run(sc), OPTIONS[opt])
    return _runs[(kind, opt)]


def bit_identical(a, b):
    same = len(a.after) == len(b.after)
    for (sa, ea, Sa), (sb, eb, Sb) in zip(a.after, b.after):
        same = same and np.array_equal(Sa, Sb) and all(np.array_equal(u, v) for u, v in zip(tuple(sa) + tuple(ea), tuple(sb) + tuple(eb)))
    if a.stats is not None:
        same = same and all(np.array_equal(u, v) for u, v in zip(a.stats, b.stats))
    return bool(same)


def fp32_errors(sc, dev, orun):
    """test_gpu_fp32_sigma.py's quantities against the oracle: Sigma (relative Frobenius), pose, worst landmark (relative)"""
    worst = dict(sigma=0.0, pose=0.0, landmarks=0.0)
    for (st_g, (b, ib, pb), S_g), (st_o, (a, ia, pa), S_o) in zip(dev.after, orun.after):
        assert np.array_equal(ia, ib) and np.all(np.isfinite(S_g)) and np.array_equal(S_g, S_g.astype(np.float32).astype(np.float64))
        worst["sigma"] = max(worst["sigma"], rel_fro(S_g, S_o))
        worst["pose"] = max(worst["pose"], se3_log_dist(b[6:13], a[6:13]) / max(1.0, np.linalg.norm(a[10:13])))
        worst["landmarks"] = max(worst["landmarks"], float(np.max(np.linalg.norm(pb - pa, axis=1) / np.maximum(1.0, np.linalg.norm(pa, axis=1)))))
    return worst


@pytest.mark.parametrize("kind,opt", CASES, ids=[f"{k}-{o}" for k, o in CASES])
def test_tail_route(kind, opt):
    sc = cs.BY_NAME[SCENARIOS[kind]]
    orun = cs.oracle_run(sc)
    dev = device_run(kind, opt)
    c, want = dev.counters, COUNTERS[(kind, opt)]
    fp32 = (OPT_SIGMA_FP32, 2) in OPTIONS[opt]
    same = bit_identical(dev, device_run(kind, "defaults"))
    print(f"{kind} {opt}: N {sc.N} M {sc.M} NJ {sc.NJ} updated {dev.updated} counters {c} bit-identical to the defaults: {same}")
    # (c)
    assert dev.updated == want["upd"], (dev.updated, want)
    assert c["la_fallbacks"] == 0
    for k in ("la", "zb", "me", "calls", "queued", "cancelled", "sel", "live", "early"):
        assert c[k] == want[k], (kind, opt, k, c, want)
    # (a)
    if sc.route == "select":
        ab, pr, disc = orun.candidates
        assert list(dev.removed) == disc and c["discarded"] == len(disc) == sc.cap
        a_o, p_o = orun.stats
        a_g, p_g, _ = dev.stats
        np.testing.assert_allclose(a_g, a_o, rtol=1e-11, atol=1e-11)  # test_outlier_stats' bounds
        # (probErr is a function of S = C Sigma C^T + R: with Sigma stored as float it is held to SURVEY's bound on Sigma itself; absErr does not depend on Sigma)
        np.testing.assert_allclose(p_g, p_o, rtol=1e-4 if fp32 else 1e-9, atol=1e-11)
    if fp32:
        worst = fp32_errors(sc, dev, orun)
        print(f"{kind} {opt}: against the oracle {worst}")
        assert worst["sigma"] <= 1e-4 and worst["pose"] <= 1e-5 and worst["landmarks"] <= 1e-5  # SURVEY's bounds, as test_gpu_fp32_sigma.py holds them up to 60 landmarks
    else:
        compare(sc, dev, orun)
    # (b)
    differs = NOT_BIT_IDENTICAL.get((kind, opt))
    if differs is None:
        assert same, (kind, opt)
    elif differs == GAMMA:
        assert np.array_equal(dev.after[0][2], device_run(kind, "defaults").after[0][2]), (kind, opt)
