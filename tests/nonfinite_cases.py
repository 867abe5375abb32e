"""Planted cases for EQF_OPT_CHECK_FINITE (helper module, not a test), after the pattern of riccati_cases.py: one Case is one call of the context path
(include/eqf_hip.h) on a Sigma with a NaN / +Inf / -Inf planted at a named position - or its clean twin, the same seed with nothing planted.

The option stands in for the reference's assert(!Sigma.hasNaN()) behind its three Riccati integrations and its update (VIO_eqf.cpp:71, 90, 102, 133). A case's
label - "reported" or "clean" - is therefore never written by hand: label(case) is "reported" exactly where something is planted, and
tests/test_nonfinite_cases.py shows on the CPU that this equals oracle_verdict(case) = not np.all(np.isfinite(Sigma)) of the ORACLE's Sigma after the same call
on the same planted Sigma, for every case. tests/test_gpu_nonfinite.py then compares the device with the reference's verdict and not with itself.

Sizes, the smallest at which the scan (k_check_finite: 256-row blocks over n = 21 + 3 N rows, one block row per column) can still go wrong: N = 1 (n = 24),
N = 78 (n = 255, one block not full), N = 79 (n = 258: the second row block holds two rows), N = 86 (n = 279: row 257 is not the last row).

Calls (CALLS): the propagation modes by the entry point and options that select them - "fast", "fast_unfused" (EQF_OPT_FUSED_ASSEMBLY = 0), "fast_dense"
(EQF_OPT_RICCATI_DENSE = 1) and "staged_propagate" (eqf_stage_measurement in front) are eqf_propagate_fast with one observer step, "riccati_fast", "accurate" and
"discrete" the three eqf_integrate_riccati_* calls - and the update (eqf_vision_update) with the look-ahead kernel eligible (M = 40 of 79: 3 panels)
and as the launch chain (M = 12). An update only ever reads the columns of Sigma that belong to a MEASURED landmark (C_i is 2 x 3 on the landmark's own block), so
its cases plant where the factorisation does not read - the sensor block's diagonal, the last two landmarks, which no update case measures - and the NaN survives
Sigma -= W W^T for the check to find. The one exception is the position "measured_diag": there the pivot test may see the value first, and the expectation is
"nonzero" (EQF_E_NOT_SPD or EQF_E_NONFINITE, never 0)."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from context_scenarios import CHART_NAMES, lookahead_fits
from oracle_binding import OracleFilter
from util import default_camera, random_imu, random_spd, reasonable_state, settings_for, synth_measurement

VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
SIZES = (1, 78, 79, 86)
DT = 0.01
ROW_EDGES = ("row_255", "row_256", "row_257")
POSITIONS = ("sensor_diag", "sensor_offdiag", "first_lm", "last_diag", "last_row_first_col", "cross_unmeasured") + ROW_EDGES
PROPAGATIONS = ("fast", "fast_unfused", "fast_dense", "riccati_fast", "accurate", "discrete", "staged_propagate")
UPDATES = ("update_la", "update_chain")
CALLS = PROPAGATIONS + UPDATES
# what the oracle runs for a call: integrateRiccatiStateFast (+ one observer step where the device call is eqf_propagate_fast), ...Accurate, ...Discrete, performVisionUpdate
ORACLE_OF = {"fast": "fast+observer", "fast_unfused": "fast+observer", "fast_dense": "fast+observer", "staged_propagate": "fast+observer", "riccati_fast": "fast",
             "accurate": "accurate", "discrete": "discrete", "update_la": "update", "update_chain": "update"}
UPDATE_M = {"update_la": 40, "update_chain": 12}  # at N >= 78; at N = 1 the one landmark is measured (and both names are the chain)
FP32_MODES = (1, 2, 3)  # EQF_OPT_SIGMA_FP32: float model on the fp64 store, float store, mixed-store model


@dataclass(frozen=True)
class Case:
    chart: str      # "invdepth" | "euclid" | "normal"
    N: int
    call: str       # one of CALLS
    value: str      # a key of VALUES, or "none": the clean twin
    position: str   # one of POSITIONS or "measured_diag"; "none" for the twin
    fp32: int = 0   # EQF_OPT_SIGMA_FP32

    @property
    def n(self):
        return 21 + 3 * self.N

    @property
    def seed(self):  # of the state and the frame: a case and its twin share it
        return 7000 + 10 * self.N + list(CHART_NAMES).index(self.chart)

    @property
    def id(self):
        return f"{self.call}-{self.chart}-N{self.N}-{self.position}-{self.value}" + (f"-fp32_{self.fp32}" if self.fp32 else "")

    def twin(self):
        return Case(self.chart, self.N, self.call, "none", "none", self.fp32)


def label(case):
    """what the case says of itself"""
    if case.value == "none":
        return "clean"
    return "nonzero" if case.position == "measured_diag" else "reported"


def unmeasured(N):
    """the two landmarks (state indices) that no update case measures, and between which "cross_unmeasured" lies"""
    return (N - 2, N - 1)


def measured(case):
    """state indices an update case measures: the first M, never the last two"""
    if case.call not in UPDATES:
        return []
    M = 1 if case.N == 1 else UPDATE_M[case.call]
    assert case.N == 1 or M <= case.N - 2
    return list(range(M))


def entries(case):
    """(row, column) pairs of Sigma that hold the planted value (a symmetric set)"""
    n, N, p = case.n, case.N, case.position
    if p == "none":
        return []
    if p == "sensor_diag":
        out = [(3, 3)]
    elif p == "sensor_offdiag":
        out = [(2, 17)]
    elif p == "first_lm":
        out = [(21, 21)]
    elif p == "last_diag":
        out = [(n - 1, n - 1)]
    elif p == "last_row_first_col":
        out = [(n - 1, 0)]
    elif p == "cross_unmeasured":
        a, b = unmeasured(N)
        out = [(21 + 3 * a + i, 21 + 3 * b + j) for i in range(3) for j in range(3)]
    elif p in ROW_EDGES:
        r = int(p[4:])
        out = [(r, r)]
    elif p == "measured_diag":
        l = 21 + 3 * measured(case)[0]
        out = [(l, l)]
    else:
        raise KeyError(p)
    assert all(0 <= r < n and 0 <= c < n for r, c in out), (case.id, out)
    return sorted(set(out) | {(c, r) for r, c in out})


def allowed(N, position):
    """does the position exist at this size"""
    n = 21 + 3 * N
    if position in ROW_EDGES:
        return int(position[4:]) < n
    if position == "cross_unmeasured":
        return N >= 2
    return True


@dataclass
class Inputs:
    settings: object
    state: tuple      # xi0, Xs, ids, q0, Q
    S: np.ndarray     # the clean Sigma
    imu: np.ndarray
    cam: object
    mid: np.ndarray
    y: np.ndarray


@lru_cache(maxsize=None)
def _inputs(chart, N, seed, meas):
    # the first lines are test_gpu_parity.make_pair's, so that make_pair(CHART_NAMES[chart], N, seed, useDiscreteInnovationLift=0) yields this state and Sigma
    rng = np.random.default_rng(seed)
    settings = settings_for(CHART_NAMES[chart], useDiscreteInnovationLift=0)
    xi0, Xs, ids, q0, Q = reasonable_state(rng, N, shuffle_ids=True)
    S = random_spd(rng, 21 + 3 * N)
    frame = np.random.default_rng(seed + 50000)  # the frame's own stream: the same IMU sample and pixels whatever make_pair drew
    imu = random_imu(frame, bias_vel=True)
    cam = default_camera()
    sub = list(meas) if meas else list(range(min(N, 8)))  # (propagations: what staged_propagate stages)
    mid, y = synth_measurement(frame, cam, ids, q0, Q, noise_px=1.0, subset=np.array(sub, dtype=int))
    return Inputs(settings, (xi0, Xs, ids, q0, Q), S, imu, cam, mid, y)


def inputs(case):
    """settings, state, clean Sigma, IMU sample and measurement of a case; shared (and left unchanged) by every case of the same chart, size and measured set"""
    return _inputs(case.chart, case.N, case.seed, tuple(measured(case)))


def planted_sigma(case):
    S = inputs(case).S.copy()
    for r, c in entries(case):
        S[r, c] = VALUES[case.value]
    return S


def apply_oracle(orc, case):
    """the reference's step for the case's call"""
    inp, kind = inputs(case), ORACLE_OF[case.call]
    if kind in ("fast", "fast+observer"):
        orc.integrate_riccati_fast(inp.imu, DT)
        if kind == "fast+observer":
            orc.integrate_observer(inp.imu, DT, True)
    elif kind == "accurate":
        orc.integrate_riccati_accurate(inp.imu, DT)
    elif kind == "discrete":
        orc.integrate_riccati_discrete(inp.imu, DT)
    else:
        orc.vision_update(inp.cam, inp.mid, inp.y)


def oracle_for(case, Sigma=None):
    """an oracle holding the case's state and (planted) Sigma, the call not yet made"""
    inp = inputs(case)
    orc = OracleFilter(inp.settings)
    orc.set_eqf(*inp.state, planted_sigma(case) if Sigma is None else Sigma)
    return orc


def oracle_verdict(case):
    """the reference's hasNaN() behind the call, widened to Inf as the option is: "reported" | "clean" """
    orc = oracle_for(case)
    apply_oracle(orc, case)
    return "clean" if np.all(np.isfinite(orc.get_sigma())) else "reported"


def _reported():
    out = []

    def add(chart, N, call, value, position, fp32=0):
        if not allowed(N, position):
            return
        c = Case(chart, N, call, value, position, fp32)
        if c not in out:
            out.append(c)

    # every call x NaN x three positions at N = 79, both charts; the normal chart for the propagation modes
    for chart in ("invdepth", "euclid", "normal"):
        for call in (PROPAGATIONS if chart == "normal" else CALLS):
            for pos in ("sensor_diag", "last_diag", "last_row_first_col"):
                add(chart, 79, call, "nan", pos)
    # every position x every value for the fast and the accurate mode at N = 79
    for call in ("fast", "accurate"):
        for pos in POSITIONS:
            for value in VALUES:
                add("invdepth", 79, call, value, pos)
    # the row edges of the scan's 256-row blocks, either side: n = 255 has none of the three rows (its last row and column stand in), 258 ends at 257, 279 goes past
    for N in (78, 79, 86):
        for pos in ROW_EDGES + (("last_diag", "last_row_first_col") if N == 78 else ()):
            add("euclid", N, "fast", "nan", pos)
    # the smallest state, every call (its one landmark is measured by the update: the sensor block is where the factorisation does not read)
    for call in CALLS:
        add("invdepth", 1, call, "nan", "sensor_diag")
        if call in PROPAGATIONS:
            add("invdepth", 1, call, "nan", "last_diag")
    # the update where it may read: two unmeasured landmarks' cross block, and a measured landmark's own variance
    for call in UPDATES:
        add("invdepth", 79, call, "nan", "cross_unmeasured")
        add("invdepth", 79, call, "nan", "measured_diag")
        add("invdepth", 79, call, "+inf", "last_diag")
    # the float stores: the kernel reads float (2) or doubles that hold floats (1, 3)
    for mode in FP32_MODES:
        for call in ("fast",) + UPDATES:
            add("invdepth", 79, call, "nan", "last_diag", mode)
    return out


REPORTED = _reported()  # (the measured_diag cases among them: label "nonzero")
TWINS = list(dict.fromkeys(c.twin() for c in REPORTED))
CASES = REPORTED + TWINS


def update_form(case):
    """"lookahead" | "chain": what context_scenarios.lookahead_fits says of an update case"""
    return "lookahead" if lookahead_fits(case.N, len(measured(case))) else "chain"
