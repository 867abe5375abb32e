"""The changes of coordinates of tests/rechart_cases.py through the CPU oracle and oracle/indep ALONE, so that tests/test_gpu_batch_rechart.py compares the
device against a T that is the reference's own: block diagonal, carrying the oracle's A, B and C from one chart to the other, commuting with the Riccati step
up to the process noise and with the innovation covariance when the equivariant output is off - and against cases on which a conversion that only relabels
the slot is far from the bound. No GPU is needed."""
import numpy as np
import pytest

import rechart_cases as rcs
from batch_scenarios import reference_defaults
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL
from oracle_binding import OracleFilter
from util import random_imu, rel_fro

PAIR_IDS = [rcs.pair_name(p) for p in rcs.PAIRS]
PROCESS = ["biasOmegaProcessVariance", "biasAccelProcessVariance", "attitudeProcessVariance", "positionProcessVariance", "velocityProcessVariance",
           "cameraAttitudeProcessVariance", "cameraPositionProcessVariance", "pointProcessVariance"]


def oracle(chart, N, Sigma=None, **kw):
    state, S = rcs.case(N)
    orc = OracleFilter(reference_defaults(coordinateChoice=chart, **kw))
    orc.set_eqf(*state, S if Sigma is None else Sigma)
    return orc


def innovation_cov(orc, N, star):
    cam, mid, y = rcs.frame(N)
    C = orc.output_matrix_C(cam, mid, y, star)
    return C @ orc.get_sigma() @ C.T + orc.settings.measurementNoise**2 * np.eye(C.shape[0])


def on_blocks(N):
    m = np.zeros((21 + 3 * N, 21 + 3 * N), bool)
    m[:21, :21] = True
    for i in range(N):
        m[21 + 3 * i:24 + 3 * i, 21 + 3 * i:24 + 3 * i] = True
    return m


def test_T_is_block_diagonal():
    """the differential of the whole state map has no entry off the blocks the helper builds T from, and equals it on them"""
    for N in (1, 2, 5):
        for kind, chart in (("invdepth", COORD_INVDEPTH), ("normal", COORD_NORMAL)):
            for D, Tm in ((rcs.full_differential(N, "euclid", kind), rcs.T(N, COORD_EUCLIDEAN, chart)), (rcs.full_differential(N, kind, "euclid"), rcs.T(N, chart, COORD_EUCLIDEAN))):
                assert not np.any(D[~on_blocks(N)]), (N, kind)  # exactly 0 off the blocks
                assert np.abs(D - Tm).max() <= 1e-15 * np.abs(Tm).max(), (N, kind, np.abs(D - Tm).max())
    for N in rcs.NS:
        for a, b in rcs.PAIRS:
            Tm = rcs.T(N, a, b)
            assert not np.any(Tm[~on_blocks(N)])
            if COORD_NORMAL not in (a, b):
                assert np.array_equal(Tm[:21, :21], np.eye(21))  # exactly the identity
            else:
                assert np.abs(Tm[:21, :21] - np.eye(21)).max() > 1e-2
            assert np.abs(Tm @ rcs.T(N, b, a) - np.eye(len(Tm))).max() <= 1e-13


@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_T_carries_the_oracles_matrices(pair):
    """A_to = T A_from T^-1, B_to = T B_from and, without the equivariant output, C_to = C_from T^-1 at 1e-9: a closed-form T that misses that is a wrong T"""
    a, b = pair
    N = 5
    imu = random_imu(np.random.default_rng(3), bias_vel=True)
    Tm, Ti = rcs.T(N, a, b), rcs.T(N, b, a)
    oa, ob = oracle(a, N), oracle(b, N)
    cam, mid, y = rcs.frame(N)
    dA = rel_fro(Tm @ oa.state_matrix_A(imu) @ Ti, ob.state_matrix_A(imu))
    dB = rel_fro(Tm @ oa.input_matrix_B(), ob.input_matrix_B())
    dC = rel_fro(oa.output_matrix_C(cam, mid, y, False) @ Ti, ob.output_matrix_C(cam, mid, y, False))
    print(f"{rcs.pair_name(pair)}: A {dA:.1e}  B {dB:.1e}  C {dC:.1e}  cond T {np.linalg.cond(Tm):.0f}")
    assert dA <= 1e-9 and dB <= 1e-9 and dC <= 1e-9, (dA, dB, dC)


@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_riccati_commutes_without_process_noise(pair):
    """with every process variance 0, one integrate_riccati_accurate under each chart: Sigma'_to = T Sigma'_from T^T at 1e-9"""
    a, b = pair
    N = 5
    imu = random_imu(np.random.default_rng(4), bias_vel=True)
    zero = {k: 0.0 for k in PROCESS}
    oa = oracle(a, N, **zero)
    ob = oracle(b, N, Sigma=rcs.expected(N, a, b), **zero)
    oa.integrate_riccati_accurate(imu, 0.05)
    ob.integrate_riccati_accurate(imu, 0.05)
    d = rel_fro(rcs.congruence(rcs.T(N, a, b), oa.get_sigma()), ob.get_sigma())
    moved = rel_fro(ob.get_sigma(), rcs.expected(N, a, b))
    print(f"{rcs.pair_name(pair)}: Riccati step commutes to {d:.1e} (the step moved Sigma by {moved:.1e})")
    assert d <= 1e-9 and moved > 1e-6, (d, moved)


def test_cases_tell_the_charts_apart():
    """a call that only relabels the slot cannot pass: T Sigma T^T is far from Sigma wherever T is not the identity"""
    seen = []
    for N in rcs.NS:
        for a, b in rcs.PAIRS:
            d = rel_fro(rcs.expected(N, a, b), rcs.case(N)[1])
            if N >= 1 or COORD_NORMAL in (a, b):
                seen.append(d)
                assert d > 1e-3, (N, rcs.pair_name((a, b)), d)
            else:
                assert d == 0.0  # no landmark, neither chart Normal: T is the identity
    print(f"T Sigma T^T against Sigma: at least {min(seen):.2e} relative")


def test_fp64_reference_is_good_to_1e10():
    """numpy's T Sigma T^T is within 1e-10 of the 50-digit product on every case: a factor 10 under the device bound"""
    worst = 0.0
    for N in rcs.NS:
        for a, b in rcs.PAIRS:
            d = rel_fro(rcs.expected(N, a, b), rcs.expected_mp(N, a, b))
            worst = max(worst, d)
            assert d <= 1e-10, (N, rcs.pair_name((a, b)), d)
    print(f"numpy against 50 digits: {worst:.1e}")


@pytest.mark.parametrize("pair", rcs.PAIRS, ids=PAIR_IDS)
def test_innovation_covariance_is_invariant_without_the_equivariant_output(pair):
    """on the frames the GPU invariance test uses: S = C Sigma C^T + R under one chart and under the other with T Sigma T^T, within 1e-10"""
    a, b = pair
    worst = 0.0
    for N in [n for n in rcs.NS if n > 0]:
        Sa = innovation_cov(oracle(a, N, useEquivariantOutput=0), N, False)
        Sb = innovation_cov(oracle(b, N, Sigma=rcs.expected(N, a, b), useEquivariantOutput=0), N, False)
        d = rel_fro(Sb, Sa)
        worst = max(worst, d)
        assert d <= 1e-10, (N, d)
    print(f"{rcs.pair_name(pair)}: S under the two charts {worst:.1e}")


def test_normal_equivariant_output_is_not_the_transported_one():
    """under Normal with the equivariant output on the two innovation covariances differ by more than 1e-6 (DESIGN.md section 11.13 says so); InvDepth's agree"""
    N = 5
    for other in (COORD_EUCLIDEAN, COORD_INVDEPTH):
        Sa = innovation_cov(oracle(other, N, useEquivariantOutput=1), N, True)
        Sb = innovation_cov(oracle(COORD_NORMAL, N, Sigma=rcs.expected(N, other, COORD_NORMAL), useEquivariantOutput=1), N, True)
        d = rel_fro(Sb, Sa)
        print(f"equivariant output, {rcs.KIND[other]} against normal: S differs by {d:.1e}")
        assert d > 1e-6, d
    Sa = innovation_cov(oracle(COORD_EUCLIDEAN, N, useEquivariantOutput=1), N, True)
    Sb = innovation_cov(oracle(COORD_INVDEPTH, N, Sigma=rcs.expected(N, COORD_EUCLIDEAN, COORD_INVDEPTH), useEquivariantOutput=1), N, True)
    print(f"equivariant output, euclid against invdepth: S differs by {rel_fro(Sb, Sa):.1e}")
    assert rel_fro(Sb, Sa) <= 1e-10
