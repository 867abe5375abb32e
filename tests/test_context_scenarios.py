"""The planted frames of context_scenarios.py through the CPU oracle ALONE: every scenario is the size it claims to be, the select scenarios produce the
claimed candidates with a binding cap, both sides of every threshold of THRESHOLDS are present, and - condition, not measurement - the oracle's two dense
arithmetics (as written: LU inverse, K evaluated twice; efficient: Cholesky, symmetric) agree on Sigma+ to 1e-10 relative Frobenius on every frame, so that
the flat 1e-9 of tests/test_gpu_context_sizes.py is attainable by the reference alone on these inputs."""
import numpy as np
import pytest

import context_scenarios as cs
from oracle_binding import ARITH_AS_WRITTEN, ARITH_EFFICIENT
from util import rel_fro

CONDITION = 1e-10


@pytest.mark.parametrize("name", [sc.name for sc in cs.SCENARIOS])
def test_scenario_is_what_it_claims(name):
    sc = cs.BY_NAME[name]
    a = cs.run_oracle(sc, ARITH_AS_WRITTEN)
    b = cs.run_oracle(sc, ARITH_EFFICIENT)
    assert len(a.frames) == sc.frames == len(a.after)
    ids0 = a.state0[2]
    assert len(ids0) == sc.N and sc.shuffled == bool(np.any(np.diff(ids0) < 0))
    for fa, fb in zip(a.frames, b.frames):
        assert len(fa.mid) == sc.M and len(fa.y) == 2 * sc.M and np.all(np.diff(fa.mid) > 0)
        assert np.array_equal(fa.mid, fb.mid) and np.allclose(fa.y, fb.y, rtol=0, atol=1e-6)  # (the second frame's pixels follow each oracle's own first update)
        assert set(fa.mid.tolist()) == set(int(ids0[i]) for i in sc.measured)
    assert sc.NJ == (2 * sc.M + 31) // 32
    if sc.M < sc.N:  # unmeasured landmarks at both ends and in the middle
        un = sorted(set(range(sc.N)) - set(sc.measured))
        assert un[0] == 0 and un[-1] == sc.N - 1 and any(sc.measured[0] < i < sc.measured[-1] for i in un)
    if sc.route == "select":
        ab, pr, disc = a.candidates
        assert sorted(ab) == sorted(i for i, _ in sc.abs_out) and sorted(pr) == sorted(i for i, _ in sc.prob_out)
        assert len(ab) == 5 and len(pr) == 6 and len(disc) == sc.cap < len(ab) + len(pr)  # the cap binds, inside the probabilistic-only candidates
        assert set(ab) <= set(disc) and b.candidates == a.candidates
        vals = [a.stats[0][i] for i in ab] + [a.stats[1][i] for i in pr]
        assert len(set(vals)) == len(vals)
        # no decision hangs on the last bits: every statistic is well away from its threshold
        absE, probE = a.stats
        seen = absE >= 0
        assert np.min(np.abs(absE[seen] - sc.thr_abs)) > 0.5 and np.min(np.abs(probE[seen] / sc.thr_prob - 1.0)) > 1e-3
        assert len(a.after[0][0][2]) == sc.N - sc.cap
    for f, (ra, rb) in enumerate(zip(a.after, b.after)):
        assert np.array_equal(ra[0][2], rb[0][2])
        e = rel_fro(ra[2], rb[2])
        assert np.all(np.isfinite(ra[2])) and e <= CONDITION, (name, f, e)


def test_both_sides_of_every_threshold():
    S = cs.SCENARIOS
    NJs = {(sc.route, sc.NJ) for sc in S}
    for lo, hi in ((2, 3), (8, 9), (16, 17), (32, 33)):
        for route in ("update", "staged"):
            assert (route, lo) in NJs and (route, hi) in NJs, (route, lo, hi)
    Ns = {sc.N for sc in S}
    assert {249, 250, 255, 256, 257, 271, 273, 511, 512, 513} <= Ns
    assert {sc.N for sc in S if sc.route == "select"} >= {512, 513}
    for key in cs.THRESHOLDS:
        assert key == "NEES 32|33" or any(key in sc.pins for sc in S), key
    big = [sc for sc in S if sc.N > 512 and sc.route == "staged"]
    assert len({sc.N for sc in big}) >= 4 and any(sc.N > 512 and sc.route == "select" for sc in S)
    # the look-ahead kernel refused on co-residency alone: few panels, too many T half-rows
    co = [sc for sc in S if "co-residency" in sc.pins]
    assert co and all(3 <= sc.NJ <= 32 and not cs.lookahead_fits(sc.N, sc.M) for sc in co)
    # more than 3 tiles per workgroup in the propagation: the smallest tpw with which sum_r ceil((r + 1) / tpw) + 2 + observer blocks fit 256 compute units
    def tpw(N):
        nT = (N + 15) // 16
        t = 1
        while t < 8 and sum((r + t) // t for r in range(nT)) + 2 + (N + 767) // 768 > cs.CU_COUNT:
            t += 1
        return t
    assert tpw(512) == 3 and tpw(640) == 4 and tpw(1000) == 8
    assert {"euclid", "invdepth", "normal"} == {sc.chart for sc in S}
    for N in (256, 257, 512, 513):
        assert any(sc.chart == "euclid" and sc.N == N for sc in S)
    assert any(sc.chart == "normal" and sc.N > 256 for sc in S)
    assert {sc.cam for sc in S} == {"pinhole", "radtan", "equidistant"} and {sc.lift for sc in S} == {0, 1} and {sc.star for sc in S} == {0, 1} and {sc.vel_lift for sc in S} == {0, 1}
    assert any(sc.sigma == "init" for sc in S) and any(sc.M % 16 for sc in S) and any(sc.M == sc.N for sc in S)
