"""Planted single frames for the single-filter context path (EqfCore, include/eqf_hip.h; helper module, not a test), after the pattern of batch_scenarios.py.
The context path picks its kernels by size in about a dozen places (THRESHOLDS below, read from eqvio_amd/csrc/eqf_hip.hip and eqf_kernels.hpp); a Scenario is
one planted frame on one side of such a threshold: chart, N, which landmarks are measured, id order, camera, IMU samples, lifts, output, Sigma, and the ROUTE
by which the device is driven:

 * "update": set_state / set_sigma, integrate_riccati_fast, vision_update (the stand-alone route: k_measure in front of the update tail);
 * "staged": stage_measurement + propagate_fast + stats_then_update for TWO consecutive frames (the second takes its output blocks from the propagation kernel);
 * "select": the staged calls with eqf_stats_select_update and thresholds under which planted measurements are absolute outliers, others probabilistic-only
   ones, and the cap binds: the decision is taken on the device.

run_oracle(sc) builds the frames (each measurement is projected from the ORACLE's propagated estimate) and runs them through the CPU oracle alone;
run_device(sc, oracle_run) replays the same frames on the device and reads its counters. tests/test_context_scenarios.py checks on the CPU that every
scenario is what its label says, tests/test_gpu_context_sizes.py compares."""
import ctypes as C
import time
from dataclasses import dataclass, field

import numpy as np

from batch_scenarios import CAMERAS as _BATCH_CAMERAS
from batch_scenarios import PINHOLE, SMALL, frame_imus, ranked_discards
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL
from oracle_binding import OracleFilter
from util import estimate_landmarks, imu_selection, project, random_spd, reasonable_state, settings_for

CAMERAS = {"pinhole": PINHOLE, "radtan": _BATCH_CAMERAS["radtan"], "equidistant": _BATCH_CAMERAS["equidistant"]}
CHART_NAMES = {"invdepth": COORD_INVDEPTH, "euclid": COORD_EUCLIDEAN, "normal": COORD_NORMAL}
FRAME_DT = 0.05
CU_COUNT = 256  # compute units of one MI355X: lookahead_eligible compares the launch's workgroups with it

# Size thresholds of the context path, as read from the code (left value | right value take different forms). NJ = ceil(2 M / 32) panels of S.
THRESHOLDS = {
    "NJ 2|3": "launch chain below the smallest look-ahead instantiation (lookahead_eligible: NJ >= 3)",
    "NJ 8|9": "ZB = 2 (the look-ahead kernel evaluates the output blocks itself) in the speculative tail up to 8 panels (plan_tail)",
    "NJ 16|17": "la_row2 / la_build_rows2, HOME placement, live_cols and live_first up to 16 panels (launch_lookahead, plan_tail, stats_select_route)",
    "NJ 32|33": "look-ahead kernel up to 32 panels (la_njcap), one launch per panel above",
    "N 256|257": "propagation: nT = ceil(N / 16) > 16 takes the mirrored lower triangle with several tiles per workgroup (plan_propagation)",
    "N 249|250": "k_syrk_lift walks the lower triangle row by row up to SYRK_ARITH_TILES = 24 tile rows of 32 (21 + 3 N <= 768)",
    "N 512|513": "SEL_ONE_WG = 512: k_stats_select up to it, k_outlier_stats -> k_select_outliers above",
    "N 16k": "16-landmark tiles of the propagation kernel (PT): 255, 257, 271, 273, 511, 513",
    "N 64k": "64-landmark blocks of the lift (k_syrk_lift: nlift = ceil(N / 64)): 255, 257, 511, 513, 640",
    "co-residency": "(2 NJ - 1) + ceil((22 + 3 N) / 16) + 1 > 256 compute units: lookahead_eligible refuses, the update takes k_build_Z + the launch chain",
    "NEES 32|33": "launch chain over 21 + 3 N + 1 columns: 32 panels up to N = 334, 33 from N = 335",
}


def panels(M):
    return (2 * M + 31) // 32


def lookahead_fits(N, M):
    """lookahead_eligible (eqf_hip.hip) restated: 3 .. 32 panels, and every workgroup of the launch resident at once"""
    NJ = panels(M)
    return 3 <= NJ <= 32 and (2 * NJ - 1) + (21 + 3 * N + 1 + 15) // 16 + 1 <= CU_COUNT


@dataclass
class Scenario:
    name: str
    route: str                 # "update" | "staged" | "select"
    chart: str
    N: int
    measured: list             # state indices the frame measures
    seed: int
    shuffled: bool = False
    cam: str = "pinhole"
    k: int = 4                 # IMU samples of the frame
    lift: int = 0              # useDiscreteInnovationLift
    vel_lift: int = 1          # useDiscreteVelocityLift
    star: int = 1              # useEquivariantOutput
    sigma: str = "spd"         # "spd": util.random_spd; "init": the settings' initial diagonal
    abs_out: tuple = ()        # select: (state index, pixel offset)
    prob_out: tuple = ()
    cap: int = -1              # select: max_outliers
    thr_abs: float = 1e9
    thr_prob: float = 1e9
    pins: tuple = ()           # the THRESHOLDS keys this scenario sits next to
    noise_px: float = 0.4
    meas_noise: float = 1.5
    extra: dict = field(default_factory=dict)

    @property
    def M(self):
        return len(self.measured)

    @property
    def NJ(self):
        return panels(self.M)

    @property
    def frames(self):
        return 2 if self.route == "staged" else 1

    def settings(self):
        kw = dict(fastRiccati=1, useDiscreteInnovationLift=self.lift, useDiscreteVelocityLift=self.vel_lift, useEquivariantOutput=self.star, measurementNoise=self.meas_noise,
                  initialPointVariance=4.0)
        if self.route == "select":
            kw.update(pointProcessVariance=1e-8)  # so that the planted-small landmark blocks stay small through the propagation
        return settings_for(CHART_NAMES[self.chart], **kw)

    def expected(self):
        """What the device's counters must read after the scenario (see plan_tail / stats_then_update and its three routes): look-ahead launches, launches that built Z
        inside, updates that used the propagation kernel's output blocks, speculative tails queued, frames with the device-side decision."""
        la = lookahead_fits(self.N, self.M)
        if self.route == "update":
            return dict(la=int(la), zb=int(la), me=0, calls=0, queued=0, sel=0)
        if self.route == "select":
            return dict(la=int(la), zb=int(la), me=0, calls=1, queued=0, sel=1)
        # staged: the first frame has no camera yet (ZB = 2 up to 8 panels, k_build_Z above), the second reads the propagation kernel's output blocks (ZB = 3)
        return dict(la=2 * int(la), zb=(2 if self.NJ <= 8 else 1) * int(la), me=1, calls=2, queued=2, sel=0)

    def form(self):
        la = lookahead_fits(self.N, self.M)
        fact = "chain" if not la else ("lookahead<=16" if self.NJ <= 16 else "lookahead17..32")
        prop = "full" if (self.N + 15) // 16 <= 16 else "mirrored"
        return f"{fact}/{prop}" + ("/select1wg" if self.route == "select" and self.N <= 512 else "/select2" if self.route == "select" else "")


def spread_out(N, M):
    """M of N indices that leave unmeasured landmarks at both ends and in the middle"""
    if M >= N:
        return list(range(N))
    gap = N - M
    lo, mid = gap // 3, gap // 3
    hi = gap - lo - mid
    cut = lo + (M // 2)
    idx = list(range(lo, cut)) + list(range(cut + mid, N - hi))
    assert len(idx) == M and idx[0] >= (1 if gap >= 3 else 0)
    return idx


# ------------------------------------------------------------------------------------------------ the frames, through the oracle alone
@dataclass
class Frame:
    mean: np.ndarray
    total: float
    imus: np.ndarray
    dts: np.ndarray
    mid: np.ndarray
    y: np.ndarray


@dataclass
class OracleRun:
    state0: tuple
    Sigma0: np.ndarray
    frames: list
    after: list                # per frame: (get_eqf() tuple, state_estimate() tuple, Sigma)
    stats: tuple = None        # select: (absErr, probErr) of the oracle after the propagation
    candidates: tuple = None   # select: (absolute, probabilistic-only, discarded) state indices
    seconds: float = 0.0
    orc: object = None


def planted(sc):
    rng = np.random.default_rng(sc.seed)
    st = reasonable_state(rng, sc.N, shuffle_ids=sc.shuffled)
    n = 21 + 3 * sc.N
    s = sc.settings()
    Sigma = random_spd(rng, n) if sc.sigma == "spd" else np.diag(s.initial_cov_diag(sc.N))
    if sc.prob_out:
        d = np.ones(n)
        d[:21] = SMALL
        for i, _ in sc.prob_out:
            d[21 + 3 * i:24 + 3 * i] = SMALL
        Sigma = d[:, None] * Sigma * d[None, :]
    return rng, s, st, Sigma


def run_oracle(sc, arithmetic=None):
    """The scenario through the CPU oracle: VIO_eqf calls in the order of VIOFilter::processVisionData (Riccati step at the old X, observer steps, [outlier
    removal,] update). The update route propagates Sigma only, as its device calls do."""
    rng, s, st, Sigma = planted(sc)
    cam = CAMERAS[sc.cam]
    orc = OracleFilter(s)
    if arithmetic is not None:
        orc.set_arithmetic(arithmetic)
    orc.set_eqf(*st, Sigma, time=0.0)
    out = OracleRun(st, Sigma, [], [])
    t0 = 0.0
    t_start = time.perf_counter()
    for f in range(sc.frames):
        stamp = t0 + FRAME_DT
        imus = frame_imus(rng, t0, stamp, sc.k)
        dts, mean, total = imu_selection(imus, t0, stamp)
        orc.integrate_riccati_fast(mean, total)
        if sc.route != "update":
            for u, dt in zip(imus, dts):
                orc.integrate_observer(u, dt, bool(s.useDiscreteVelocityLift))
        _, _, ids, q0, Q = orc.get_eqf()
        pix = project(cam, estimate_landmarks(q0, Q)) + rng.normal(size=(sc.N, 2)) * sc.noise_px
        for i, off in list(sc.abs_out) + list(sc.prob_out):
            ang = rng.uniform(0, 2 * np.pi)
            pix[i] += off * np.array([np.cos(ang), np.sin(ang)])
        sel = np.asarray(sc.measured)
        order = np.argsort(ids[sel])
        sel = sel[order]
        mid, y = ids[sel].astype(np.int32), pix[sel].reshape(-1)
        out.frames.append(Frame(mean, total, imus, dts, mid, y))
        if sc.route == "select":
            absE, probE = orc.outlier_stats(cam, mid, y)
            a, p, disc = ranked_discards(absE, probE, sc.thr_abs, sc.thr_prob, sc.cap)
            out.stats, out.candidates = (absE, probE), (a, p, sorted(disc))
            for i in sorted(disc, reverse=True):
                orc.remove_landmark_by_index(i)
            gone = set(int(ids[i]) for i in disc)
            keep = np.array([int(v) not in gone for v in mid])
            mid, y = mid[keep], y.reshape(-1, 2)[keep].reshape(-1)
        orc.vision_update(cam, mid, y)
        out.after.append((orc.get_eqf(), orc.state_estimate(), orc.get_sigma()))
        t0 = stamp
    out.seconds = time.perf_counter() - t_start
    out.orc = orc
    return out


_oracle_runs = {}


def oracle_run(sc):
    """run_oracle in the oracle's default arithmetic, once per process and scenario"""
    if sc.name not in _oracle_runs:
        _oracle_runs[sc.name] = run_oracle(sc)
    return _oracle_runs[sc.name]


# ------------------------------------------------------------------------------------------------ the device
@dataclass
class DeviceRun:
    after: list                # per frame: (get_state(), state_estimate(), Sigma)
    counters: dict
    stats: tuple = None        # last frame: (absErr, probErr, depth2)
    removed: np.ndarray = None
    updated: list = None


def read_counters(core, every=False):
    """The counters that name the route a frame took (what a repeated run must reproduce). every=True: also the ones that depend on the host's timing or are not
    about routes - every other *_stats getter, eqf_nees_lu_fallbacks and the wait count of eqf_host_wait_stats. Nothing is reset."""
    v = [C.c_long() for _ in range(14)]
    lib, h = core.lib, core.h
    assert lib.eqf_lookahead_stats(h, C.byref(v[0]), C.byref(v[1]), 0) == 0
    assert lib.eqf_z_in_lookahead_stats(h, C.byref(v[2]), 0) == 0
    assert lib.eqf_measure_in_propagate_stats(h, C.byref(v[3]), 0) == 0
    assert lib.eqf_speculation_stats(h, C.byref(v[4]), C.byref(v[5]), C.byref(v[6]), 0) == 0
    assert lib.eqf_selection_stats(h, C.byref(v[7]), C.byref(v[8]), 0) == 0
    names = ("la", "la_fallbacks", "zb", "me", "calls", "queued", "cancelled", "sel", "discarded")
    if every:
        assert lib.eqf_hold_stats(h, C.byref(v[9]), 0) == 0
        assert lib.eqf_gather_stats(h, C.byref(v[10]), 0) == 0
        assert lib.eqf_live_columns_stats(h, C.byref(v[11]), 0) == 0
        assert lib.eqf_early_doorbell_stats(h, C.byref(v[12]), 0) == 0
        assert lib.eqf_nees_lu_fallbacks(h, C.byref(v[13])) == 0
        names += ("hold", "gather", "live", "early", "nees_lu")
    out = {k: x.value for k, x in zip(names, v)}
    if every:
        calls, seconds = (C.c_long * 2)(), (C.c_double * 2)()
        assert lib.eqf_host_wait_stats(h, calls, seconds, 0) == 0
        out["wait_calls"] = calls[0]
    return out


def run_device(sc, orun, options=()):
    """The frames of orun on a fresh context of exactly N landmarks, by sc.route; the context is closed before returning."""
    from eqvio_amd.capi import OPT_SPECULATIVE, EqfCore

    s = sc.settings()
    cam = CAMERAS[sc.cam]
    Qd, Pd = s.input_gain_diag12(), s.state_gain_diag8()
    var = s.measurementNoise**2
    core = EqfCore(sc.N, CHART_NAMES[sc.chart])
    try:
        for opt, val in options:
            core.set_option(opt, val)
        if sc.route == "select":
            core.set_option(OPT_SPECULATIVE, 0)  # straight to the device-side decision (what the back-off reaches after a cancelled tail)
        core.set_state(*orun.state0)
        core.set_sigma(orun.Sigma0)
        out = DeviceRun([], {}, updated=[])
        for fr in orun.frames:
            if sc.route == "update":
                core.integrate_riccati_fast(fr.mean, fr.total, Qd, Pd)
                core.vision_update(cam, fr.mid, fr.y, var, bool(sc.star), bool(sc.lift))
            else:
                core.stage_measurement(fr.mid, fr.y)
                core.propagate_fast(fr.mean, fr.total, Qd, Pd, fr.imus, fr.dts, bool(sc.vel_lift))
                if sc.route == "staged":
                    upd, *out.stats = core.stats_then_update(cam, fr.mid, fr.y, sc.thr_abs, sc.thr_prob, var, bool(sc.star), bool(sc.lift))
                else:
                    upd, a, p, d, out.removed = core.stats_select_update(cam, fr.mid, fr.y, sc.thr_abs, sc.thr_prob, sc.cap, var, bool(sc.star), bool(sc.lift))
                    out.stats = [a, p, d]
                out.updated.append(upd)
            out.after.append((core.get_state(), core.state_estimate(), core.get_sigma()))
        out.counters = read_counters(core)
        return out
    finally:
        core.close()


# ------------------------------------------------------------------------------------------------ the scenarios
def _sc(name, route, chart, N, M=None, seed=0, **kw):
    measured = kw.pop("measured", None)
    if measured is None:
        measured = spread_out(N, N if M is None else M)
    return Scenario(name, route, chart, N, measured, seed, **kw)


ABS_OFFS = (30.0, 12.0, 15.0, 18.0, 21.0)
PROB_OFFS = (2.5, 2.9, 3.3, 3.7, 4.1, 4.5)


def _select(name, N, M, seed, chart="invdepth", **kw):
    """5 absolute and 6 probabilistic-only outliers among the measured landmarks (first and last measured index among them), the cap at 8"""
    measured = spread_out(N, M)
    pick = [measured[int(round(v))] for v in np.linspace(0, M - 1, 11)]
    abs_out = tuple(zip(pick[0::2][:5], ABS_OFFS))
    prob_out = tuple(zip([i for i in pick if i not in pick[0::2][:5]], PROB_OFFS))
    return Scenario(name, "select", chart, N, measured, seed, abs_out=abs_out, prob_out=prob_out, cap=8, thr_abs=6.0, thr_prob=4.0, noise_px=0.2, **kw)


def build_scenarios():
    s = []
    # panels of S on both sides of every boundary, stand-alone route and staged route (M = N unless said)
    for M, pins in ((32, ("NJ 2|3",)), (33, ("NJ 2|3",)), (128, ("NJ 8|9",)), (129, ("NJ 8|9",)), (256, ("NJ 16|17", "N 256|257")), (257, ("NJ 16|17", "N 256|257", "N 16k", "N 64k")),
                    (512, ("NJ 32|33", "N 512|513")), (513, ("NJ 32|33", "N 512|513", "N 16k", "N 64k"))):
        s.append(_sc(f"update_inv_N{M}", "update", "invdepth", M, seed=100 + M, pins=pins, shuffled=M % 2 == 1, lift=M % 2))
        s.append(_sc(f"staged_inv_N{M}", "staged", "invdepth", M, seed=200 + M, pins=pins, shuffled=M % 2 == 0, lift=(M + 1) % 2, star=1 if M != 129 else 0, k=3 + M % 5))
    # SYRK_ARITH_TILES and the 16 / 64 landmark tiles; ragged last panels (M not a multiple of 16), M < N with the gaps at both ends and in the middle
    s.append(_sc("update_inv_N249", "update", "invdepth", 249, seed=301, pins=("N 249|250",), sigma="init"))
    s.append(_sc("update_inv_N250", "update", "invdepth", 250, seed=302, pins=("N 249|250",), sigma="init"))
    s.append(_sc("staged_inv_N255_M250", "staged", "invdepth", 255, 250, seed=303, pins=("N 16k", "N 64k"), cam="radtan", vel_lift=0))
    s.append(_sc("staged_inv_N271_M257", "staged", "invdepth", 271, 257, seed=304, pins=("N 16k", "NJ 16|17"), shuffled=True))
    s.append(_sc("staged_inv_N273_M256", "staged", "invdepth", 273, 256, seed=305, pins=("N 16k", "NJ 16|17"), cam="equidistant", star=0))
    s.append(_sc("update_inv_N511_M33", "update", "invdepth", 511, 33, seed=306, pins=("N 16k", "N 64k", "NJ 2|3"), shuffled=True))
    s.append(_sc("staged_inv_N300_M32", "staged", "invdepth", 300, 32, seed=307, pins=("NJ 2|3", "N 256|257")))
    # Euclidean on both sides of N = 256 | 257 and M = 512 | 513
    for M in (256, 257, 512, 513):
        s.append(_sc(f"staged_euc_N{M}", "staged", "euclid", M, seed=400 + M, pins=("N 256|257",) if M < 300 else ("NJ 32|33", "N 512|513"), shuffled=M % 2 == 1, lift=M % 2))
    s.append(_sc("update_euc_N513", "update", "euclid", 513, seed=420, pins=("NJ 32|33",), lift=1))
    # Normal chart above 256 (k_congruence_normal)
    s.append(_sc("update_nrm_N260_M250", "update", "normal", 260, 250, seed=430, pins=("N 256|257",), shuffled=True))
    # above every threshold
    s.append(_sc("staged_inv_N640_M600", "staged", "invdepth", 640, 600, seed=500, pins=("NJ 32|33", "N 64k"), k=6))
    # (continuous lift: with the discrete one this frame pair flings landmarks to scales of 3e-5, and the oracle's own two arithmetics differ by 9e-9 on such a scale)
    s.append(_sc("staged_inv_N1000_M520", "staged", "invdepth", 1000, 520, seed=501, pins=("NJ 32|33",), shuffled=True))
    # look-ahead kernel refused on co-residency although M is small
    s.append(_sc("staged_inv_N1300_M100", "staged", "invdepth", 1300, 100, seed=502, pins=("co-residency",)))
    # the device-side outlier decision on both sides of SEL_ONE_WG, of 16 panels and above 32 panels
    s.append(_select("select_inv_N512_M256", 512, 256, 600, pins=("N 512|513", "NJ 16|17")))
    s.append(_select("select_inv_N513_M257", 513, 257, 601, pins=("N 512|513", "NJ 16|17"), shuffled=True))
    s.append(_select("select_euc_N540_M530", 540, 530, 602, chart="euclid", pins=("NJ 32|33",)))
    s.append(_select("select_inv_N200_M190", 200, 190, 603, pins=()))
    # the smallest look-ahead instantiation (3 panels) behind the device-side decision (tests/test_gpu_tail_routes.py crosses the options over it)
    s.append(_select("select_inv_N40_M36", 40, 36, 604, pins=("NJ 2|3",)))
    return s


SCENARIOS = build_scenarios()
BY_NAME = {sc.name: sc for sc in SCENARIOS}
assert len(BY_NAME) == len(SCENARIOS)
LARGEST = ["staged_inv_N1000_M520", "staged_inv_N640_M600", "select_inv_N513_M257"]  # run twice in fresh contexts: bit-identical
