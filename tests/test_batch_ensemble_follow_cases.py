"""The planted cases of eqf_bens_follow (tests/batch_ensemble_follow_cases.py) proved on the CPU with numpy alone: every shape is the edge its label claims,
every case of the table is admitted (the fp64 restatement agrees with the same arithmetic at higher precision to 1e-11), the draw is the conditional law it is
said to be, the regeneration identity holds, and the statistical case's mean NEES is the reference's. Nothing here calls the product. Seen values are printed
(run with -s); profiles/r31_batch_ensemble_follow_parity.txt lists such a run."""
import numpy as np
import pytest

from batch_ensemble_follow_cases import (ADMIT, FIVE, OTHERS, REGEN, SHAPES, SIZES_P, TABLE, StatCase, admission, get_case, key, regenerated)
from ensemble_cases import STAT_BANDS

IDS = [key(*t) for t in TABLE]


def test_every_shape_is_the_edge_its_label_claims():
    n = lambda N: 21 + 3 * N  # noqa: E731
    assert len(TABLE) == 31 and len(set(TABLE)) == 31 and len(set(IDS)) == 31
    assert n(6) % 2 == 1  # 5 -> 6: n = 39 is odd, the factor is padded
    assert n(9) % 16 == 0 and n(25) % 16 == 0  # 9 -> 10, 9 -> 12, 25 -> 26: the split falls on a tile edge ...
    assert all(n(k) % 16 for k in (0, 1, 5, 7, 15, 16, 60, 63))  # ... and inside a tile everywhere else
    assert n(12) - n(9) == 9 and n(12) > n(9) + 4  # 9 -> 12: more than one row block of normals behind the edge
    assert n(15) // 16 == n(16) // 16 == 4 and n(17) // 16 == 4 and n(15) % 4 == 2 and n(16) % 4 == 1 and n(5) % 4 == 0  # partly and wholly used row blocks of four
    assert n(64) == 213 and n(64) % 2 == 1 and (n(64) + 3) // 4 * 4 == 216  # the capacity: padded factor, 216 rows of normals in a 224-row tile
    assert n(60) // 16 < n(64) // 16 and n(63) // 16 == n(64) // 16  # 60 -> 64 crosses a tile edge, 63 -> 64 stays inside the last tile
    assert {t[3] for t in TABLE} == set(SIZES_P) and {15, 16, 17} <= set(SIZES_P) and 257 in SIZES_P  # a wave's 16 particles, more than one workgroup of 256
    for t in TABLE:
        fc = get_case(*t)
        ids, sens, p = fc.cloud
        assert len(set(ids.tolist())) == len(ids) == fc.nK + fc.nf and sens.shape == (fc.P, 23) and p.shape == (fc.P, fc.nK + fc.nf, 3)
        kept = [i for i in ids if i in set(fc.c.ids.tolist())]
        assert sorted(kept) == sorted(fc.c.ids[:fc.nK].tolist())  # the cloud lacks a suffix of the slot's order: the rule holds
        assert fc.counts == (fc.nf, fc.N - fc.nK)
        if fc.variant == "order":
            assert not fc.moves
        elif fc.nK > 1 or (fc.nK == 1 and fc.nf):
            assert fc.moves or fc.nK <= 1
        for i, gid in enumerate(fc.c.ids[:fc.nK]):  # the kept points sit where the cloud's id says
            assert p[:, list(ids).index(gid)].tobytes() == np.ascontiguousarray(fc.kept_p[:, i]).tobytes()
    reorder = [get_case(*t) for t in TABLE if t[1:3] == (3, 3)]
    assert reorder and all(fc.moves and fc.counts == (0, 0) for fc in reorder)  # 3 -> 3: nothing leaves or arrives, only the order changes
    drops = [get_case(*t) for t in TABLE if t[1:3] == (2, 2)]
    assert [fc.counts for fc in drops] == [(2, 0), (2, 0)] and [fc.moves for fc in drops] == [False, True]  # 4 -> 2: with and without a move
    assert any(get_case(*t).moves for t in TABLE if t[1] < t[2]) and any(not get_case(*t).moves for t in TABLE if t[1] < t[2])
    assert len({s for s, _ in FIVE + OTHERS}) == 7 and len({c[0] for _, c in FIVE}) == 3


@pytest.mark.parametrize("case", TABLE, ids=IDS)
def test_case_is_admitted(case):
    fc = get_case(*case)
    ee, ep = admission(fc)
    how = "mpmath 50 digits" if fc.N <= 26 else "np.longdouble linear algebra, charts at 50 digits"
    print(f"[follow admission] {key(*case)} n_K = {fc.nk} n = {fc.n}: eps_A {ee:.2e} points {ep:.2e} ({how}; cond Sigma {np.linalg.cond(fc.c.Sigma):.0f})")
    assert ee <= ADMIT and ep <= ADMIT
    if fc.N > fc.nK:
        assert np.all(np.isfinite(fc.added_p)) and fc.added_p.shape == (fc.P, fc.N - fc.nK, 3)
        assert np.all(np.isfinite(fc.nees)) and np.all(fc.nees > 0)


@pytest.mark.parametrize("case", [t for t in TABLE if 0 < t[1] < t[2] and t[2] <= 26], ids=[key(*t) for t in TABLE if 0 < t[1] < t[2] and t[2] <= 26])
def test_the_draw_is_the_conditional_law(case):
    """L_AK z_K = Sigma_AK Sigma_KK^-1 eps_K and L_AA L_AA^T = the Schur complement: eps_A | eps_K ~ N(mean, Schur) without forming either"""
    fc = get_case(*case)
    S, L, nk = fc.c.Sigma, fc.c.L, fc.nk
    mean = S[nk:, :nk] @ np.linalg.solve(S[:nk, :nk], fc.epsK)
    schur = S[nk:, nk:] - S[nk:, :nk] @ np.linalg.solve(S[:nk, :nk], S[:nk, nk:])
    got_mean = fc.eps[nk:] - L[nk:, nk:] @ fc.xi[nk:]
    scale = np.sqrt(np.diag(S)[nk:])[:, None]
    em = float(np.max(np.abs(got_mean - mean) / scale))
    es = float(np.max(np.abs(L[nk:, nk:] @ L[nk:, nk:].T - schur) / (scale * scale.T)))
    print(f"[follow law] {key(*case)}: mean {em:.2e} Schur {es:.2e} (relative to the standard deviations)")
    assert em <= 1e-9 and es <= 1e-9


@pytest.mark.parametrize("case", REGEN, ids=[key(*t) for t in REGEN])
def test_regeneration_identity(case):
    fc = get_case(*case)
    again, first = regenerated(fc)
    err = float(np.max(np.abs(again - first) / np.maximum(1.0, np.abs(first))))
    print(f"[follow regeneration] {key(*case)}: {err:.2e}")
    assert err <= 1e-11


def test_statistical_case_in_the_restatement():
    sc = StatCase()
    print(f"[follow statistics] N = 2 -> 3 (one id leaves, two arrive), n = {sc.n}, P = {sc.P}: mean NEES {sc.mean_nees:.6f} (band {STAT_BANDS['initial']}, "
          f"spread to expect {np.sqrt(2.0 / (sc.n * sc.P)):.4f})")
    assert abs(sc.mean_nees - 1.0) <= STAT_BANDS["initial"] == 0.1
    assert sc.eps.shape == (30, 1000)
