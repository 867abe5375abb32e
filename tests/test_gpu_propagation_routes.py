"""The option-dependent branches of the propagation half of the context path - the three Riccati entry points and eqf_propagate_fast with its observer chunks, staged
measurement, removal record and held landmarks - one option at a time and in the pairs that share a rule, at the smallest sizes at which each form of the launch
exists: N = 17 (two 16-landmark tiles, the second holding one landmark; the full square of tiles), N = 257 (17 tiles a side: the smallest mirrored launch, one tile per
workgroup on 256 compute units) and, for the dense modes, N = 0 and 1. The counterpart of test_gpu_tail_routes.py; for every (route, place, option set):

 (a) parity with the CPU oracle at the suite's flat 1e-9 (test_gpu_context_sizes.compare; SURVEY's bounds as test_gpu_fp32_sigma.py holds them where Sigma is stored
     as float; test_riccati_discrete's 5e-9 for the discrete mode in the normal chart, where the reference differentiates numerically in other coordinates),
 (b) bit-identity with the default-options run of the same route and place, wherever the options only move work between launches (not_bit_identical names the rest
     and the arithmetic that differs),
 (c) the device's counters against COUNTERS below, which is derived from the rules in eqf_hip.hip (plan_propagation, eqf_hold_supported) and not from a run.

The routes are driven through the public C-ABI the way a caller must: a refused eqf_add_landmarks_held is followed by eqf_add_landmarks behind the propagation (the
reference's order), a statistics call that reports "not updated" by eqf_vision_update. The oracle's order is always remove, propagate, append. What the code refuses
is in REFUSED: each call returns EQF_E_UNSUPPORTED and leaves the context as it was."""
import os
import re
from dataclasses import dataclass

import numpy as np
import pytest

import context_scenarios as cs
from batch_scenarios import frame_imus
from eqvio_amd.capi import (OPT_CHECK_FINITE, OPT_FUSED_ASSEMBLY, OPT_GATHER_IN_PROPAGATE, OPT_HOLD_NEW_LANDMARKS, OPT_MEASURE_IN_PROPAGATE, OPT_RICCATI_DENSE, OPT_SIGMA_FP32,
                            OPT_TILES_PER_WORKGROUP, OPT_TIMING, OPT_Z_IN_LOOKAHEAD, EqfCore, EqfError)
from oracle_binding import OracleFilter
from test_gpu_context_sizes import _Snapshot, compare
from test_gpu_parity import TOL, check_state
from test_gpu_tail_routes import bit_identical, fp32_errors
from util import imu_selection, random_imu, rel_fro

pytestmark = pytest.mark.gpu

_KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "eqvio_amd", "csrc", "eqf_kernels.hpp")
OBS_CHUNK = int(re.search(r"constexpr int kObsChunk = (\d+);", open(_KERNELS).read()).group(1))  # observer steps one launch carries
E_UNSUPPORTED = -6

# ---------------------------------------------------------------------------------------------------------------------------------------------- routes and places
PLACES = {"inv0": ("invdepth", 0), "inv1": ("invdepth", 1), "inv17": ("invdepth", 17), "euc17": ("euclid", 17), "nrm17": ("normal", 17), "inv257": ("invdepth", 257),
          "nrm257": ("normal", 257)}
SMALL, FAST = ("inv17", "euc17", "nrm17", "inv257"), ("inv17", "euc17", "nrm17", "inv257", "nrm257")
DENSE_MODES = ("inv0", "inv1") + SMALL
# route -> its places. riccati_fast at N = 0 and 1 exists for the option sets with EQF_OPT_RICCATI_DENSE only (applicable)
ROUTES = {
    "riccati_fast": ("inv0", "inv1") + FAST,
    "riccati_accurate": DENSE_MODES,
    "riccati_discrete": DENSE_MODES,
    "propagate_k3": FAST,
    "propagate_chunks": SMALL,   # k = kObsChunk + 1: the last step is a k_observer launch of its own
    "propagate_k0": SMALL,
    "staged_fresh": SMALL,       # eqf_stage_measurement first, on a context that has not seen an update: the observer blocks know no camera
    "staged_seen": SMALL,        # ... the same for a second frame: they evaluate the output blocks with the camera of the first frame's update
    "gather": SMALL,             # eqf_remove_landmarks of three landmarks in front (no held route in the normal chart: eqf_hold_supported)
    "held": ("inv17", "euc17", "inv257"),
    "held_gather": ("inv17", "euc17", "inv257"),
}
STEPS = {"propagate_k3": 3, "propagate_chunks": OBS_CHUNK + 1, "propagate_k0": 0, "gather": 3, "held": 3, "held_gather": 3}
HELD_VAR = 1.7

OPTIONS = {
    "defaults": (),
    "fused_assembly=0": ((OPT_FUSED_ASSEMBLY, 0),),
    "riccati_dense=1": ((OPT_RICCATI_DENSE, 1),),
    "sigma_fp32=2": ((OPT_SIGMA_FP32, 2),),
    "tiles_per_workgroup=0": ((OPT_TILES_PER_WORKGROUP, 0),),
    "tiles_per_workgroup=2": ((OPT_TILES_PER_WORKGROUP, 2),),
    "tiles_per_workgroup=8": ((OPT_TILES_PER_WORKGROUP, 8),),
    "gather_in_propagate=0": ((OPT_GATHER_IN_PROPAGATE, 0),),
    "hold_new_landmarks=0": ((OPT_HOLD_NEW_LANDMARKS, 0),),
    "measure_in_propagate=0": ((OPT_MEASURE_IN_PROPAGATE, 0),),
    "z_in_lookahead=0": ((OPT_Z_IN_LOOKAHEAD, 0),),
    "check_finite=1": ((OPT_CHECK_FINITE, 1),),
    "timing=1": ((OPT_TIMING, 1),),  # per-kernel timing
    "riccati_dense=1,fused_assembly=0": ((OPT_RICCATI_DENSE, 1), (OPT_FUSED_ASSEMBLY, 0)),
    "sigma_fp32=2,gather_in_propagate=0": ((OPT_SIGMA_FP32, 2), (OPT_GATHER_IN_PROPAGATE, 0)),
    "check_finite=1,hold_new_landmarks=0": ((OPT_CHECK_FINITE, 1), (OPT_HOLD_NEW_LANDMARKS, 0)),
}
# (pairs of an option and a route that share a rule - the float store on the gather route, the finite check on the held route - are cases of the cross product)


def has(opt, option, value):
    return (option, value) in OPTIONS[opt]


def applicable(route, place, opt):
    """The combinations the code accepts and in which the option can act (REFUSED holds the others)"""
    N = PLACES[place][1]
    if any(o == OPT_TILES_PER_WORKGROUP for o, _ in OPTIONS[opt]) and N != 257:
        return False  # acts on the mirrored form only
    if has(opt, OPT_SIGMA_FP32, 2) and route in ("riccati_accurate", "riccati_discrete"):
        return False  # refused: the float store exists for the structured fast path only
    if route == "riccati_fast" and N <= 1:
        return has(opt, OPT_RICCATI_DENSE, 1)
    return True


CASES = [(route, place, opt) for route, places in ROUTES.items() for place in places for opt in OPTIONS if applicable(route, place, opt)]

# ---------------------------------------------------------------------------------------------------------------------------------------------- (c) the counters
# gather: propagation launches that applied the removal record themselves; hold: ... that created the held landmarks themselves; me: updates that took the output
# blocks the propagation kernel's observer blocks evaluated. Per route with default options, outside the normal chart:
ZERO = dict(gather=0, hold=0, me=0)
DEFAULT = {route: dict(ZERO) for route in ROUTES}
DEFAULT["gather"] = dict(ZERO, gather=1)
DEFAULT["held"] = dict(ZERO, hold=1)
DEFAULT["held_gather"] = dict(ZERO, gather=1, hold=1)
DEFAULT["staged_seen"] = dict(ZERO, me=1)  # the second frame's update; the first has no camera to evaluate with (staged_fresh: 0)
# What an option set changes, rule by rule (plan_propagation; eqf_hold_supported for `hold`):
#  the fused kernel is available: EQF_OPT_FUSED_ASSEMBLY, no EQF_OPT_RICCATI_DENSE, fp64 Sigma, not the normal chart - and for this call: observer steps, N > 0.
#  gather: the fused kernel, EQF_OPT_GATHER_IN_PROPAGATE, a record of removals only (up to GATHER_MAXN = 512 landmarks in the buffers).
#  hold: eqf_add_landmarks_held accepts where the fused kernel is available, with EQF_OPT_HOLD_NEW_LANDMARKS, EQF_OPT_GATHER_IN_PROPAGATE and no finite check; the
#  propagation then creates them on the gather route. Refused there, the caller appends them behind the propagation: no launch counted.
#  me: the observer blocks evaluate output blocks with fused assembly (any chart), a staged measurement, a camera from an earlier update, all steps in one chunk,
#  EQF_OPT_MEASURE_IN_PROPAGATE, EQF_OPT_Z_IN_LOOKAHEAD, fp64 Sigma and no finite check; the speculative tail of the update then takes them (plan_tail).
NO_FUSED_KERNEL = {"gather": dict(gather=0), "held": dict(hold=0), "held_gather": dict(gather=0, hold=0), "staged_seen": dict(me=0)}
NO_HOLD = {"held": dict(hold=0), "held_gather": dict(hold=0)}
CHANGES = {
    "fused_assembly=0": NO_FUSED_KERNEL,
    "riccati_dense=1": NO_FUSED_KERNEL,
    "sigma_fp32=2": NO_FUSED_KERNEL,
    "gather_in_propagate=0": {"gather": dict(gather=0), "held": dict(hold=0), "held_gather": dict(gather=0, hold=0)},
    "hold_new_landmarks=0": NO_HOLD,
    "measure_in_propagate=0": {"staged_seen": dict(me=0)},
    "z_in_lookahead=0": {"staged_seen": dict(me=0)},
    "check_finite=1": dict(NO_HOLD, staged_seen=dict(me=0)),  # (the removal record is still applied inside the launch)
    "riccati_dense=1,fused_assembly=0": NO_FUSED_KERNEL,
    "sigma_fp32=2,gather_in_propagate=0": NO_FUSED_KERNEL,
}
CHANGES["check_finite=1,hold_new_landmarks=0"] = CHANGES["check_finite=1"]
NORMAL_CHART = {"gather": dict(gather=0)}  # no fused kernel for the gather route; fused ASSEMBLY, and with it `me`, exists in every chart
COUNTERS = {(route, place, opt): {**DEFAULT[route], **CHANGES.get(opt, {}).get(route, {}), **(NORMAL_CHART.get(route, {}) if PLACES[place][0] == "normal" else {})}
            for route, place, opt in CASES}

# ---------------------------------------------------------------------------------------------------------------------------------------------- (b) bit-identity
#  FP32: Sigma is rounded to float on every store.
#  DENSE: EQF_OPT_RICCATI_DENSE forms F and sums F Sigma F^T in two GEMMs (k_gemm_nt: 32 x 32 tiles over the whole row) where the arrow form (k_propagate_main) sums the
#  sensor strip and one 3 x 3 landmark block per element. The accurate and the discrete mode are dense whatever the option says: bit-identical with it.
#  Everything else - who assembles A and B (fused assembly evaluates the same expressions from the same Q and sensor terms inside the propagation kernel), tiles per
#  workgroup, who compacts the removed landmarks or writes the new ones, whether a measurement is staged or evaluated along, the finite check, the timing events -
#  moves the same operations between launches.
#  TAIL: not the propagation but the update behind it, at 17 panels of S (N = M = 257). With output blocks from the propagation kernel (me) the look-ahead kernel builds
#  its rows of Z in registers (ZB = 3, la_build_rows2); without them k_build_Z builds Z in memory in front of it (plan_tail: ZB = 2 ends at 8 panels) and sums
#  C Sigma C^T in its own order. Everything up to and including the second frame's propagation (Run.mid) is still bit-identical; only its update is not.
FP32, DENSE, TAIL = "fp32", "dense", "tail"


def not_bit_identical(route, place, opt):
    if has(opt, OPT_SIGMA_FP32, 2):
        return FP32
    if has(opt, OPT_RICCATI_DENSE, 1) and route not in ("riccati_accurate", "riccati_discrete"):
        return DENSE
    if (route, place) == ("staged_seen", "inv257") and COUNTERS[(route, place, opt)]["me"] == 0:
        return TAIL
    return None


# ---------------------------------------------------------------------------------------------------------------------------------------------- the frames
@dataclass
class Run:
    after: list           # per frame: (state, state estimate, Sigma)
    mid: list = None      # staged routes: the same behind each frame's propagation, in front of its update
    counters: dict = None
    stats: tuple = None   # (bit_identical's interface)
    frames: int = 1
    name: str = ""


def scenario(route, place):
    chart, N = PLACES[place]
    staged = route.startswith("staged")
    # (continuous velocity lift where the steps span two launches, the discrete one everywhere else)
    return cs._sc(f"prop_{route}_{place}", "staged" if staged else "update", chart, N, seed=7000 + 31 * list(ROUTES).index(route) + N + len(chart), k=3, shuffled=True,
                  vel_lift=0 if route == "propagate_chunks" else 1)


def removed(N):
    return [0, N // 2, N - 1]  # first, the middle of a tile (8 of 16 | 128 = 8 tiles), last


@dataclass
class Plant:
    sc: object
    state0: tuple
    Sigma0: np.ndarray
    imu: np.ndarray = None     # the Riccati modes
    dt: float = 0.0
    frame: object = None       # eqf_propagate_fast: cs.Frame (no measurement)
    new_ids: np.ndarray = None
    new_p: np.ndarray = None
    staged: object = None      # cs.OracleRun of the staged routes


_plants = {}


def plant(route, place):
    """The route's inputs and its oracle run, once per process"""
    if (route, place) in _plants:
        return _plants[(route, place)]
    sc = scenario(route, place)
    if route.startswith("staged"):
        orun = cs.oracle_run(sc)
        frames = 1 if route == "staged_fresh" else 2
        p = Plant(sc, orun.state0, orun.Sigma0, staged=orun)
        out = Run(orun.after[:frames], frames=frames, name=sc.name)
        _plants[(route, place)] = (p, out)
        return p, out
    rng, s, st, Sigma = cs.planted(sc)
    orc = OracleFilter(s)
    orc.set_eqf(*st, Sigma, time=0.0)
    p = Plant(sc, st, Sigma)
    if route.startswith("riccati"):
        p.imu, p.dt = random_imu(rng, bias_vel=True), 0.02
        getattr(orc, "integrate_" + route)(p.imu, p.dt)
    else:
        k = STEPS[route]
        if k:
            imus = frame_imus(rng, 0.0, cs.FRAME_DT, k)
            dts, mean, total = imu_selection(imus, 0.0, cs.FRAME_DT)
        else:
            imus, dts, mean, total = np.zeros((0, 13)), np.zeros(0), random_imu(rng), cs.FRAME_DT
        p.frame = cs.Frame(mean, total, imus, dts, None, None)
        if "held" in route:
            p.new_ids = (np.arange(2) * 13 + int(np.max(st[2])) + 5).astype(np.int32)
            p.new_p = rng.uniform(-1, 1, (2, 3)) + np.array([0, 0, 5.0])
        if "gather" in route:
            for i in sorted(removed(sc.N), reverse=True):
                orc.remove_landmark_by_index(i)
        orc.integrate_riccati_fast(mean, total)
        for u, dt in zip(imus, dts):
            orc.integrate_observer(u, dt, bool(sc.vel_lift))
        if "held" in route:
            orc.add_landmarks(p.new_ids, p.new_p, HELD_VAR)
    out = Run([(orc.get_eqf(), orc.state_estimate(), orc.get_sigma())], name=sc.name)
    _plants[(route, place)] = (p, out)
    return p, out


def fresh_core(p, options):
    core = EqfCore(p.sc.N + 8, cs.CHART_NAMES[p.sc.chart])
    for opt, val in options:
        core.set_option(opt, val)
    core.set_state(*p.state0)
    core.set_sigma(p.Sigma0)
    return core


def snapshot(core):
    return core.get_state(), core.state_estimate(), core.get_sigma()


def propagate(core, p):
    s, fr = p.sc.settings(), p.frame
    core.propagate_fast(fr.mean, fr.total, s.input_gain_diag12(), s.state_gain_diag8(), fr.imus, fr.dts, bool(p.sc.vel_lift))


def drive(route, p, options):
    sc = p.sc
    s = sc.settings()
    Qd, Pd = s.input_gain_diag12(), s.state_gain_diag8()
    core = fresh_core(p, options)
    try:
        out = Run([], name=sc.name)
        if route.startswith("riccati"):
            getattr(core, "integrate_" + route)(p.imu, p.dt, Qd, Pd)
            out.after.append(snapshot(core))
        elif route.startswith("staged"):
            cam, var = cs.CAMERAS[sc.cam], s.measurementNoise**2
            out.frames, out.mid = 1 if route == "staged_fresh" else 2, []
            for fr in p.staged.frames[:out.frames]:
                core.stage_measurement(fr.mid, fr.y)
                core.propagate_fast(fr.mean, fr.total, Qd, Pd, fr.imus, fr.dts, bool(sc.vel_lift))
                out.mid.append(snapshot(core))
                upd, *_ = core.stats_then_update(cam, fr.mid, fr.y, sc.thr_abs, sc.thr_prob, var, bool(sc.star), bool(sc.lift))
                if upd == 0:  # statistics only (EQF_OPT_CHECK_FINITE): the thresholds are out of reach, the caller updates
                    core.vision_update(cam, fr.mid, fr.y, var, bool(sc.star), bool(sc.lift))
                out.after.append(snapshot(core))
        else:
            if "gather" in route:
                core.remove_landmarks(np.array(removed(sc.N), np.int32))
            held = "held" in route and core.add_landmarks_held(p.new_ids, p.new_p, HELD_VAR)
            propagate(core, p)
            if "held" in route and not held:
                core.add_landmarks(p.new_ids, p.new_p, HELD_VAR)
            out.after.append(snapshot(core))
        out.counters = cs.read_counters(core, every=True)
        return out
    finally:
        core.close()


_runs = {}


def device_run(route, place, opt):
    if (route, place, opt) not in _runs:
        _runs[(route, place, opt)] = drive(route, plant(route, place)[0], OPTIONS[opt])
    return _runs[(route, place, opt)]


def same_bits(a, b, but_last_update=False):
    """bit_identical over every snapshot of the two runs (but_last_update: all but the one behind the last update)"""
    upto = len(a.after) - (1 if but_last_update else 0)
    return bit_identical(Run((a.mid or []) + a.after[:upto]), Run((b.mid or []) + b.after[:upto]))


@pytest.mark.parametrize("route,place,opt", CASES, ids=[f"{r}-{p}-{o}" for r, p, o in CASES])
def test_propagation_route(route, place, opt):
    p, orun = plant(route, place)
    dev = device_run(route, place, opt)
    c, want = dev.counters, COUNTERS[(route, place, opt)]
    differs = not_bit_identical(route, place, opt)
    has_default = (route, place, "defaults") in COUNTERS
    same = same_bits(dev, device_run(route, place, "defaults"), differs == TAIL) if has_default else None
    print(f"{route} {place} {opt}: counters { {k: c[k] for k in want} } bit-identical to the defaults: {same}")
    # (c)
    assert c["la_fallbacks"] == 0
    for k, v in want.items():
        assert c[k] == v, (route, place, opt, k, c, want)
    # (a)
    if differs == FP32:
        worst = fp32_errors(p.sc, dev, orun)
        print(f"{route} {place} {opt}: against the oracle {worst}")
        # SURVEY's bounds as test_gpu_fp32_sigma.py holds them: every landmark within 1e-5 up to 60 landmarks, within 1e-3 above
        assert worst["sigma"] <= 1e-4 and worst["pose"] <= 1e-5 and worst["landmarks"] <= (1e-5 if p.sc.N <= 60 else 1e-3)
    elif route == "riccati_discrete" and p.sc.chart == "normal":
        (st_g, est_g, S_g), (st_o, est_o, S_o) = dev.after[0], orun.after[0]
        e = rel_fro(S_g, S_o)
        print(f"{route} {place} {opt}: Sigma {e:.2e}")
        assert np.all(np.isfinite(S_g)) and e <= 5e-9, e  # test_riccati_discrete's bound
        check_state(_Snapshot(st_g, est_g), _Snapshot(st_o, est_o))
    else:
        assert TOL == 1e-9
        compare(orun, dev, orun)  # (a Run carries the name and the frame count compare reads of a scenario)
    # (b)
    if differs in (None, TAIL) and has_default:
        assert same, (route, place, opt)


# ---------------------------------------------------------------------------------------------------------------------------------------------- what is refused
# name -> (route that plants the context, option set in front, options changed behind eqf_add_landmarks_held, the call that must be refused)
REFUSED = {
    "float store, accurate": ("riccati_accurate", "sigma_fp32=2", (), "riccati_accurate"),
    "float store, discrete": ("riccati_discrete", "sigma_fp32=2", (), "riccati_discrete"),
    "held, fused assembly switched off": ("held", "defaults", ((OPT_FUSED_ASSEMBLY, 0),), "propagate"),
    "held, dense switched on": ("held", "defaults", ((OPT_RICCATI_DENSE, 1),), "propagate"),
    "held, no observer steps": ("held", "defaults", (), "propagate_k0"),
    "held, eqf_integrate_riccati_fast": ("held", "defaults", (), "riccati_fast"),
    "held, eqf_integrate_riccati_accurate": ("held", "defaults", (), "riccati_accurate"),
    "held, eqf_integrate_riccati_discrete": ("held", "defaults", (), "riccati_discrete"),
    "held, eqf_integrate_observer": ("held", "defaults", (), "observer"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_call_leaves_the_context_as_it_was(name):
    route, opt, behind, call = REFUSED[name]
    p, _ = plant(route, "inv17")
    s = p.sc.settings()
    Qd, Pd = s.input_gain_diag12(), s.state_gain_diag8()
    imu = random_imu(np.random.default_rng(1), bias_vel=True)
    a, b = fresh_core(p, OPTIONS[opt]), fresh_core(p, OPTIONS[opt])
    try:
        if route == "held":
            assert a.add_landmarks_held(p.new_ids, p.new_p, HELD_VAR) and b.add_landmarks_held(p.new_ids, p.new_p, HELD_VAR)
        for o, v in behind:
            a.set_option(o, v)
        with pytest.raises(EqfError) as e:
            if call == "propagate":
                propagate(a, p)
            elif call == "propagate_k0":
                a.propagate_fast(imu, 0.05, Qd, Pd, np.zeros((0, 13)), np.zeros(0), True)
            elif call == "observer":
                a.integrate_observer(imu[None, :], np.array([0.02]), True)
            else:
                getattr(a, "integrate_" + call)(imu, 0.02, Qd, Pd)
        assert e.value.code == E_UNSUPPORTED
        for o, v in behind:
            a.set_option(o, 1 - v)
        before = (snapshot(a), snapshot(b))
        assert bit_identical(Run([before[0]]), Run([before[1]]))
        if route != "held":  # a propagation the option set accepts
            p = plant("propagate_k3", "inv17")[0]
        propagate(a, p), propagate(b, p)
        assert bit_identical(Run([snapshot(a)]), Run([snapshot(b)]))
        ca, cb = cs.read_counters(a, every=True), cs.read_counters(b, every=True)
        assert all(ca[k] == cb[k] for k in ZERO), (ca, cb)
    finally:
        a.close(), b.close()
