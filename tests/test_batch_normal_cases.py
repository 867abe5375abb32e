"""The planted frames of tests/batch_scenarios.py and tests/riccati_cases.py under the Normal chart, through the CPU oracle ALONE, so that
tests/test_gpu_batch_normal.py cannot pass vacuously: a Normal frame is told apart from its Euclidean and InvDepth twins and the three propagations from each
other by far more than the parity bounds, every scenario is the edge its name claims under this chart as well, and every oracle result is finite with a positive
definite Sigma. No GPU is needed."""
import numpy as np
import pytest

import batch_normal_cases as bn
import batch_scenarios as bs
import discrete_cases as dc
import riccati_cases as rc
from batch_scenarios import ADDED, EMPTY, REMOVED_INVALID, REMOVED_OLD, REMOVED_OUTLIERS, UPDATED
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL
from oracle_binding import OracleFilter
from util import rel_fro


def healthy(orc, name):
    """finite, and Sigma positive definite"""
    S = orc.get_sigma()
    assert all(np.all(np.isfinite(a)) for a in orc.get_eqf()) and np.all(np.isfinite(S)), name
    assert np.linalg.eigvalsh(0.5 * (S + S.T))[0] > 0.0, name


# ------------------------------------------------------------------------------------------------ a wrong chart or a wrong mode is far from the bounds
def test_normal_frames_differ_from_their_twins():
    sn, scs = bn.build_group("sizes_lift0_out1")
    seen = []
    for sc in scs:
        frames = {c: dc.whole_frame(bn.with_chart(sn, c), sc) for c in (COORD_NORMAL, COORD_EUCLIDEAN, COORD_INVDEPTH)}
        healthy(frames[COORD_NORMAL], sc.name)
        for c in (COORD_EUCLIDEAN, COORD_INVDEPTH):
            assert np.array_equal(frames[c].get_eqf()[2], frames[COORD_NORMAL].get_eqf()[2]), sc.name
            d = rel_fro(frames[c].get_sigma(), frames[COORD_NORMAL].get_sigma())
            seen.append(d)
            assert d > 1e-3, (sc.name, c, d)
    print(f"Normal against its twins, Sigma after the frame: {min(seen):.2f} .. {max(seen):.2f} relative")


def test_three_propagations_differ_under_normal():
    sn, so, sd, cases = bn.riccati()
    assert sn.coordinateChoice == so.coordinateChoice == sd.coordinateChoice == COORD_NORMAL and (so.fastRiccati, sd.useDiscreteStateMatrix) == (0, 1)
    seen = []
    for sc in cases:
        walks = {m: dc.walk(st, sc, m) for m, st in (("fast", sn), ("accurate", so), ("discrete", sd))}
        full = {m: dc.whole_frame(st, sc) for m, st in (("fast", sn), ("accurate", so), ("discrete", sd))}
        for m in walks:
            healthy(walks[m], (sc.name, m))
            healthy(full[m], (sc.name, m))
        for a, b in (("fast", "accurate"), ("fast", "discrete"), ("accurate", "discrete")):
            d = rel_fro(walks[a].get_sigma(), walks[b].get_sigma())
            print(f"{sc.name}: {a} against {b}: {d:.2e}")
            seen.append(d)
            if (a, b) != ("accurate", "discrete"):  # the issue's statement: fast against the two per-sample modes
                assert d > 1e-6, (sc.name, a, b, d)
            elif sc.N > 0:  # tests/test_batch_discrete_cases.py's statement, wherever there is a landmark
                assert d > 1e-6, (sc.name, a, b, d)
    print(f"the three propagations under Normal: at least {min(seen):.2e} apart")
    # the filter on the propagation-only form of a case is the walk by VIO_eqf calls, bit for bit (the oracle of the GPU file's propagation test)
    keep_a, keep_d = rc.oracle_settings(bn.normal(removeLostLandmarks=0)), dc.oracle_settings(bn.normal(removeLostLandmarks=0))
    for sc in cases:
        for st, m in ((keep_a, "accurate"), (keep_d, "discrete")):
            assert np.array_equal(dc.whole_frame(st, rc.propagation_only(sc)).get_sigma(), dc.walk(st, sc, m).get_sigma()), (sc.name, m)


# ------------------------------------------------------------------------------------------------ every scenario is the edge it claims, under Normal too
def described(group):
    s, scs = bn.build_group(group)
    assert s.coordinateChoice == COORD_NORMAL
    out = {}
    for sc in scs:
        d = bs.describe(s, sc)
        if sc.oracle == "full":
            healthy(dc.whole_frame(s, sc), sc.name)
        out[sc.name] = (sc, d)
    return s, out


def check_common(sc, d):
    """tests/test_batch_scenarios.py's: the oracle's bookkeeping is the planted one, its statistics predict what it did, no ambiguous order"""
    ids = sc.state[2]
    assert d["lost"] == [int(ids[i]) for i in sc.plan["lost"]] or not d["lost"] and sc.plan["lost"]
    assert d["new"] == sc.plan["new"]
    assert d["distinct"]
    if sc.oracle != "none":
        assert d["ids_after"] == d["ids_predicted"], sc.name
        assert d["invalid"] == [int(ids[i]) for i in sc.plan["invalid"]], sc.name
        if d["flags"] & UPDATED:
            assert d["min_eig_S"] > 0.0, (sc.name, d["min_eig_S"])


@pytest.mark.parametrize("group", bn.SIZE_GROUPS)
def test_size_grid(group):
    s, ds = described(group)
    assert len(bn.SIZE_GROUPS) == 4 and [ds[f"size{N}"][0].N for N in bs.SIZES] == bs.SIZES
    for name, (sc, d) in ds.items():
        check_common(sc, d)
        assert d["flags"] == UPDATED and len(d["ids_after"]) == sc.N == len(sc.mid), name
        assert d["n_abs"] == d["n_prob"] == 0
    assert ds["size64_radtan"][0].cam.model == 1


def test_partial_measurement_keeps_lost_landmarks():
    s, ds = described("partial")
    assert s.removeLostLandmarks == 0
    for M in (0, 1, 8, 33, 63):
        sc, d = ds[f"partial{M}"]
        check_common(sc, d)
        assert len(sc.mid) == M and len(d["ids_after"]) == 64 and not d["lost"]
        assert d["flags"] == (EMPTY if M == 0 else UPDATED)
        assert np.count_nonzero(d["stats"][0] >= 0) == M


@pytest.mark.parametrize("group", ["turnover_fixed", "turnover_median"])
def test_turnover_at_capacity(group):
    s, ds = described(group)
    median = "median" in group
    assert bool(s.useMedianDepth) == median and s.removeLostLandmarks == 1
    for r in (1, 16, 63, 64):
        sc, d = ds[f"turnover{r}"]
        check_common(sc, d)
        assert len(d["lost"]) == r and len(d["new"]) == r and len(d["ids_after"]) == 64 and d["flags"] == REMOVED_OLD | ADDED | UPDATED
        d2, nk = np.sort(d["kept_depth2"]), 64 - r
        expect = np.sqrt(d2[nk // 2]) if median and nk > 0 else s.initialSceneDepth
        assert abs(d["median"] - expect) <= 1e-12 * expect, (r, d["median"], expect)
    if median:
        sc, d = ds["turnover16_tie"]
        check_common(sc, d)
        d2 = np.sort(d["kept_depth2"])
        assert d2[24] == d2[25] and d2[23] < d2[24] and abs(d["median"] - np.sqrt(d2[24])) <= 1e-12 * d["median"]
    sc, d = ds["over_capacity"]
    assert sc.N == 64 and not d["lost"] and len(d["new"]) == 1 and len(sc.mid) == 65


def test_outlier_ranking_under_the_cap():
    s, ds = described("rank")
    sc, d = ds["rank64"]
    check_common(sc, d)
    assert sc.N == len(sc.mid) == 64 and d["max_outliers"] == bn.RANK_CAP
    assert d["n_abs"] == bs.C_ABS and d["n_prob"] == bs.C_PROB
    absE, probE = d["stats"]
    assert sorted(np.flatnonzero(absE > s.outlierThresholdAbs).tolist()) == sorted(sc.plan["abs"]) and 63 in sc.plan["abs"]
    for i in sc.plan["prob"]:
        assert absE[i] < s.outlierThresholdAbs and probE[i] > s.outlierThresholdProb
    ids = sc.state[2]
    by_abs = [int(ids[i]) for i in sorted(sc.plan["abs"], key=lambda i: -absE[i])]
    by_prob = [int(ids[i]) for i in sorted(sc.plan["prob"], key=lambda i: -probE[i])]
    assert d["discarded"] == (by_abs + by_prob)[: bn.RANK_CAP] and by_abs[0] == int(ids[63])
    assert d["flags"] == REMOVED_OUTLIERS | UPDATED
    sc, d = ds["rank12"]
    check_common(sc, d)
    assert d["n_abs"] == 2 and d["n_prob"] == 2 and len(d["discarded"]) == min(d["max_outliers"], 4)


def test_invalid_landmarks_at_the_ends():
    s, ds = described("invalid_ends")
    for name, idx in (("invalid0", [0]), ("invalid63", [63]), ("invalid0_31_63", [0, 31, 63])):
        sc, d = ds[name]
        check_common(sc, d)
        assert d["invalid"] == [int(sc.state[2][i]) for i in idx] and d["flags"] == UPDATED | REMOVED_INVALID
    for name in ("neighbour64", "neighbour33"):
        sc, d = ds[name]
        check_common(sc, d)
        assert d["flags"] == UPDATED and not d["invalid"]


def test_failure_scenarios():
    s, ds = described("failures")
    for name in ("not_spd", "nonfinite"):
        sc, d = ds[name]
        assert sc.N == 64 and sc.oracle == "no_update" and d["n_abs"] == d["n_prob"] == 0
        assert len(d["lost"]) == 2 and len(d["new"]) == 2 and d["flags"] == REMOVED_OLD | ADDED
        assert d["ids_after"] == d["ids_predicted"] and len(d["ids_after"]) == 64
    assert ds["not_spd"][1]["min_eig_S"] < 0.0
    # Under Normal the planted cross term (position row, one landmark) does not stay out of S: M^-1 carries the position rows into the camera-offset rows,
    # which a landmark's rows of A read. The planted Sigma and the oracle's frame without the update are finite; the update itself cannot be applied, one way
    # (a pivot of S) or the other (T = Sigma C^T) - tests/test_gpu_batch_normal.py takes either failure code for this slot.
    sc, d = ds["nonfinite"]
    assert np.all(np.isfinite(sc.Sigma)) and not (d["min_eig_S"] > 0.0 and d["T_finite"])
    full = OracleFilter(s)
    full.set_eqf(*sc.state, sc.Sigma, time=sc.t0)
    for u in sc.imus:
        full.process_imu(u)
    bs.oracle_without_update(full, s, sc)
    assert np.all(np.isfinite(full.get_sigma()))
    for name in ("good_a", "good_b", "good_c"):
        sc, d = ds[name]
        check_common(sc, d)
        assert d["flags"] & UPDATED


def test_unequal_imu_counts():
    s, ds = described("unequal_imu")
    assert sorted((len(sc.imus), sc.N) for sc, _ in ds.values()) == sorted((k, N) for k in (1, 2, 10, 45) for N in (5, 40, 64))
    for sc, d in ds.values():
        check_common(sc, d)
        assert d["flags"] == UPDATED


def test_every_group_is_checked_here():
    assert set(bn.GROUPS) == set(bn.SIZE_GROUPS) | {"partial", "turnover_fixed", "turnover_median", "rank", "invalid_ends", "failures", "unequal_imu"}
