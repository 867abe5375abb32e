"""Every planted frame of tests/batch_scenarios.py through the CPU oracle ALONE: each scenario really is the edge of k_batch_frame it claims to be (sizes after
the frame, how many outliers were candidates and how many were discarded, which landmark became invalid, an SPD innovation covariance where an update is
expected), so that tests/test_gpu_batch_edges.py cannot pass vacuously. No GPU is needed."""
import numpy as np
import pytest

import batch_scenarios as bs
from batch_scenarios import ADDED, EMPTY, REMOVED_INVALID, REMOVED_OLD, REMOVED_OUTLIERS, UPDATED


def described(group):
    s, scs = bs.build_group(group)
    return s, {sc.name: (sc, bs.describe(s, sc)) for sc in scs}


def check_common(sc, d):
    """what holds for every scenario the oracle runs: its bookkeeping is the planted one, the prediction from its statistics is what it did, no ambiguous order"""
    ids = sc.state[2]
    assert d["lost"] == [int(ids[i]) for i in sc.plan["lost"]] or not d["lost"] and sc.plan["lost"]  # the latter: removeLostLandmarks = 0
    assert d["new"] == sc.plan["new"]
    assert d["distinct"], "two candidate errors are equal: the oracle's unstable sort could order them either way"
    if sc.oracle != "none":
        assert d["ids_after"] == d["ids_predicted"], sc.name
        assert d["invalid"] == [int(ids[i]) for i in sc.plan["invalid"]], sc.name
        if d["flags"] & UPDATED:
            assert d["min_eig_S"] > 0.0, (sc.name, d["min_eig_S"])


SIZE_GROUPS = [g for g in bs.GROUPS if g.startswith("sizes_")]


@pytest.mark.parametrize("group", SIZE_GROUPS)
def test_size_grid(group):
    s, ds = described(group)
    assert len(SIZE_GROUPS) == 8 and [ds[f"size{N}"][0].N for N in bs.SIZES] == bs.SIZES
    # the tile shapes of the blocked solve: m == m16 (no column padding), n2 + 1 a multiple of 16 (no row padding), the 14th row tile, M2 = 64
    assert {8, 16, 32, 48, 56, 64} <= set(bs.SIZES) and {14, 30, 46, 62} <= set(bs.SIZES) and {63, 64} <= set(bs.SIZES)
    for name, (sc, d) in ds.items():
        check_common(sc, d)
        assert d["flags"] == UPDATED and len(d["ids_after"]) == sc.N == len(sc.mid), name  # all measured, no turnover, no outlier
        assert d["n_abs"] == d["n_prob"] == 0
    assert ds["size64_radtan"][0].cam.model == 1


@pytest.mark.parametrize("chart", ["euclid", "invdepth"])
def test_partial_measurement_keeps_lost_landmarks(chart):
    s, ds = described(f"partial_{chart}")
    assert s.removeLostLandmarks == 0
    for M in (0, 1, 8, 33, 63):
        sc, d = ds[f"partial{M}"]
        check_common(sc, d)
        assert len(sc.mid) == M and len(d["ids_after"]) == 64 and not d["lost"]
        assert d["flags"] == (EMPTY if M == 0 else UPDATED)
        absE = d["stats"][0]
        assert np.count_nonzero(absE >= 0) == M and np.count_nonzero(absE < 0) == 64 - M  # the unmeasured ones stay, with statistics -1
        if M >= 8:
            assert 0 in sc.plan["measured"] and 63 in sc.plan["measured"]
    assert ds["partial1"][0].plan["measured"] == [63]


@pytest.mark.parametrize("group", ["turnover_fixed_euclid", "turnover_fixed_invdepth", "turnover_median_euclid", "turnover_median_invdepth"])
def test_turnover_at_capacity(group):
    s, ds = described(group)
    median = "median" in group
    assert bool(s.useMedianDepth) == median and s.removeLostLandmarks == 1
    for r in (1, 16, 63, 64):
        sc, d = ds[f"turnover{r}"]
        check_common(sc, d)
        assert len(d["lost"]) == r and len(d["new"]) == r and len(d["ids_after"]) == 64
        assert d["flags"] == REMOVED_OLD | ADDED | UPDATED
        ids_new = np.array(d["new"])
        if r > 1:
            assert ids_new.min() < max(d["ids_after"][: 64 - r], default=10 ** 9) or r == 64  # new ids interleaved with the old ones in id order
        nk = 64 - r
        d2 = np.sort(d["kept_depth2"])
        assert len(d2) == nk
        expect = np.sqrt(d2[nk // 2]) if median and nk > 0 else s.initialSceneDepth  # nk = 63 (odd), 48 (even), 1, 0 (falls back to initialSceneDepth)
        assert abs(d["median"] - expect) <= 1e-12 * expect, (r, d["median"], expect)
        if median and nk == 48:
            assert d2[nk // 2] != d2[(nk - 1) // 2]  # an even count: the upper of the two middle elements is the median, and it differs from the lower
    if median:
        sc, d = ds["turnover16_tie"]
        check_common(sc, d)
        d2 = np.sort(d["kept_depth2"])
        assert len(d2) == 48 and d2[24] == d2[25] and d2[23] < d2[24]  # two kept landmarks of exactly equal depth at the median position
        assert abs(d["median"] - np.sqrt(d2[24])) <= 1e-12 * d["median"]
    sc, d = ds["over_capacity"]
    assert sc.N == 64 and not d["lost"] and len(d["new"]) == 1 and len(sc.mid) == 65  # 64 stay + 1 new


@pytest.mark.parametrize("cap", bs.RANK_CAPS)
def test_outlier_ranking_under_the_cap(cap):
    s, ds = described(f"rank_cap{cap}")
    sc, d = ds["rank64"]
    check_common(sc, d)
    assert sc.N == len(sc.mid) == 64 and d["max_outliers"] == cap
    assert d["n_abs"] == bs.C_ABS == 5 and d["n_prob"] == bs.C_PROB == 6
    absE, probE = d["stats"]
    assert sorted(np.flatnonzero(absE > s.outlierThresholdAbs).tolist()) == sorted(sc.plan["abs"]) and 63 in sc.plan["abs"]
    for i in sc.plan["prob"]:  # probabilistic-only: the pixel error is under the absolute threshold, only the chi^2 statistic fires
        assert absE[i] < s.outlierThresholdAbs and probE[i] > s.outlierThresholdProb
    n_disc = min(cap, bs.C_ABS + bs.C_PROB)
    assert len(d["discarded"]) == n_disc and len(d["ids_after"]) == 64 - n_disc
    ids = sc.state[2]
    by_abs = [int(ids[i]) for i in sorted(sc.plan["abs"], key=lambda i: -absE[i])]
    by_prob = [int(ids[i]) for i in sorted(sc.plan["prob"], key=lambda i: -probE[i])]
    assert d["discarded"] == (by_abs + by_prob)[:n_disc]
    assert by_abs[0] == int(ids[63])  # bit 63 of the drop mask is set whenever anything is discarded
    assert d["flags"] == (REMOVED_OUTLIERS if n_disc else 0) | UPDATED
    sc, d = ds["rank12"]
    check_common(sc, d)
    assert d["n_abs"] == 2 and d["n_prob"] == 2 and len(d["discarded"]) == min(d["max_outliers"], 4)


def test_max_outliers_truncation():
    s, ds = described("rank_truncation")
    sc, d = ds["trunc10"]
    check_common(sc, d)
    assert s.featureRetention == 0.9 and len(sc.mid) == 10 and (1.0 - 0.9) * 10 < 1.0  # 0.9999999999999998 -> 0
    assert d["max_outliers"] == 0 and d["n_abs"] == 1 and d["discarded"] == [] and len(d["ids_after"]) == 10


def test_invalid_landmarks_at_the_ends():
    s, ds = described("invalid_ends")
    for name, idx in (("invalid0", [0]), ("invalid63", [63]), ("invalid0_31_63", [0, 31, 63])):
        sc, d = ds[name]
        check_common(sc, d)
        assert d["invalid"] == [int(sc.state[2][i]) for i in idx] and len(d["ids_after"]) == 64 - len(idx)
        assert d["flags"] == UPDATED | REMOVED_INVALID
    for name in ("neighbour64", "neighbour33"):
        sc, d = ds[name]
        check_common(sc, d)
        assert d["flags"] == UPDATED and not d["invalid"]


@pytest.mark.parametrize("group", ["failures", "failures_euclid"])
def test_failure_scenarios(group):
    s, ds = described(group)
    assert len(ds) >= 3
    for name in ("not_spd", "nonfinite"):
        sc, d = ds[name]
        assert sc.N == 64 and sc.oracle == "no_update" and d["n_abs"] == d["n_prob"] == 0
        assert len(d["lost"]) == 2 and len(d["new"]) == 2 and d["flags"] == REMOVED_OLD | ADDED  # bookkeeping, no update
        assert d["ids_after"] == d["ids_predicted"] and len(d["ids_after"]) == 64
    assert ds["not_spd"][1]["min_eig_S"] < 0.0
    d = ds["nonfinite"][1]
    assert d["min_eig_S"] > 0.0 and not d["T_finite"]  # every pivot of S is positive and finite; T = Sigma C^T overflows, so Gamma cannot be finite
    assert np.all(np.isfinite(ds["nonfinite"][0].Sigma))
    for name in ("good_a", "good_b", "good_c"):
        sc, d = ds[name]
        check_common(sc, d)
        assert d["flags"] & UPDATED


@pytest.mark.parametrize("chart", ["euclid", "invdepth"])
def test_unequal_imu_counts(chart):
    s, ds = described(f"unequal_imu_{chart}")
    seen = [(len(sc.imus), sc.N) for sc, _ in ds.values()]
    assert sorted(seen) == sorted((k, N) for k in (1, 2, 10, 45) for N in (5, 40, 64)) and seen != sorted(seen)  # every combination, in shuffled slot order
    for sc, d in ds.values():
        check_common(sc, d)
        assert d["flags"] == UPDATED
        assert np.all(np.diff(sc.imus[:, 0]) > 0) and sc.imus[0, 0] == sc.t0 and sc.imus[-1, 0] < sc.stamp


def test_every_group_is_checked_here():
    covered = set(SIZE_GROUPS) | {f"partial_{c}" for c in ("euclid", "invdepth")} | {f"turnover_{d}_{c}" for d in ("fixed", "median") for c in ("euclid", "invdepth")}
    covered |= {f"rank_cap{c}" for c in bs.RANK_CAPS} | {"rank_truncation", "invalid_ends", "failures", "failures_euclid"} | {f"unequal_imu_{c}" for c in ("euclid", "invdepth")}
    assert covered == set(bs.GROUPS)
    assert bs.RANK_CAPS[:6] == [0, 1, 4, 5, 6, 10] and bs.RANK_CAPS[6] >= 11
