"""Changing a slot's chart under landmarks (helper module, not a test): eqf_batch_convert_chart, k_batch_rechart (eqvio_amd/csrc/eqf_batch.hpp).

The change of coordinates T between two charts is built here WITHOUT the product's code, from oracle/indep/eqvio_ref.py on its 50-digit back-end:
 * Euclidean <-> InvDepth: the closed forms conv_euc2ind(q0_i) / conv_ind2euc(q0_i), identity on the sensor coordinates;
 * Euclidean <-> Normal: the differential at 0 of state_chart("normal", state_chart_inv("euclid", .)) and of the map the other way round, by central
   differences with h = 1e-20 at 50 digits (truncation ~1e-40, rounding ~1e-30): block by block - the 21 sensor coordinates, then each landmark's 3 - which
   full_differential() checks against the differential of the whole state map at small N (tests/test_rechart_cases.py);
 * InvDepth <-> Normal: the product of the two through Euclidean.
T_ab = M_b M_a^-1 with M_euclid = I. Everything is cached per process: a reference is computed once and shared.

 * case(N): the planted state and Sigma of tests/test_gpu_batch_nees.py's plant / spd (eigenvalues in [1e-3, 10]) at N landmarks, N in NS.
 * T(N, a, b): T_ab of case(N) in fp64, dense. T_mp(N, a, b): its blocks at 50 digits. expected(N, a, b): numpy's T Sigma T^T, symmetrised.
   expected_mp(N, a, b): the same product at 50 digits, rounded to fp64.
 * frame(N): a measurement of every landmark of case(N) (no IMU sample, no propagation) for the innovation-invariance tests."""
import os
import sys
from functools import lru_cache

import numpy as np

from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL
from test_gpu_batch_nees import plant, spd
from util import default_camera, synth_measurement

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "indep"))
from eqvio_ref import MP, EqVIORef, State  # noqa: E402

CHARTS = [COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL]
KIND = {COORD_EUCLIDEAN: "euclid", COORD_INVDEPTH: "invdepth", COORD_NORMAL: "normal"}
PAIRS = [(a, b) for a in CHARTS for b in CHARTS if a != b]
NS = [0, 1, 2, 5, 21, 64]
H = "1e-20"


def pair_name(p):
    return f"{KIND[p[0]]}-{KIND[p[1]]}"


@lru_cache(maxsize=None)
def case(N):
    rng = np.random.default_rng(9100 + N)
    state, V, lam = plant(rng, N, COORD_EUCLIDEAN)
    return state, spd(V, lam)


def _ref():
    return EqVIORef(MP(50))


def _differential(r, f, n):
    h = r.o.s(H)
    return r.numerical_differential(f, r.o.zeros(n), h)


@lru_cache(maxsize=None)
def _blocks(N):
    """per chart kind: (sensor block of M, landmark blocks of M, sensor block of M^-1, landmark blocks of M^-1), object arrays at 50 digits"""
    r = _ref()
    (xi0, _, ids, q0, _), _ = case(N)
    s0 = r.sensor_from_flat(xi0)
    q0m = r.o.arr(q0)
    I21, I3 = r.o.eye(21), r.o.eye(3)
    out = {"euclid": (I21, [I3] * N, I21, [I3] * N)}
    out["invdepth"] = (I21, [r.conv_euc2ind(q0m[i]) for i in range(N)], I21, [r.conv_ind2euc(q0m[i]) for i in range(N)])
    Ms = _differential(r, lambda e: r.sensor_chart_normal(r.sensor_chart_std_inv(e, s0), s0), 21)
    Msi = _differential(r, lambda e: r.sensor_chart_std(r.sensor_chart_normal_inv(e, s0), s0), 21)
    Ml = [_differential(r, lambda e, q=q0m[i]: r.point_chart("normal", r.point_chart_inv("euclid", e, q), q), 3) for i in range(N)]
    Mli = [_differential(r, lambda e, q=q0m[i]: r.point_chart("euclid", r.point_chart_inv("normal", e, q), q), 3) for i in range(N)]
    out["normal"] = (Ms, Ml, Msi, Mli)
    return out


@lru_cache(maxsize=None)
def T_mp(N, a, b):
    """(sensor block, landmark blocks) of T_ab = M_b M_a^-1 at 50 digits"""
    _ref()
    bl = _blocks(N)
    _, _, Asi, Ali = bl[KIND[a]]
    Bs, Bl, _, _ = bl[KIND[b]]
    return Bs @ Asi, [Bl[i] @ Ali[i] for i in range(N)]


def _dense(Ts, Tl):
    n = 21 + 3 * len(Tl)
    T = np.zeros((n, n))
    f = _ref().o.tofloat
    T[:21, :21] = f(Ts)
    for i, t in enumerate(Tl):
        T[21 + 3 * i:24 + 3 * i, 21 + 3 * i:24 + 3 * i] = f(t)
    return T


@lru_cache(maxsize=None)
def T(N, a, b):
    return _dense(*T_mp(N, a, b))


def congruence(Tm, S):
    """numpy's T S T^T in fp64, symmetrised"""
    E = Tm @ S @ Tm.T
    return 0.5 * (E + E.T)


@lru_cache(maxsize=None)
def expected(N, a, b):
    return congruence(T(N, a, b), case(N)[1])


@lru_cache(maxsize=None)
def expected_mp(N, a, b):
    """T Sigma T^T at 50 digits, block by block (T is block diagonal), rounded to fp64"""
    r = _ref()
    Ts, Tl = T_mp(N, a, b)
    S = r.o.arr(case(N)[1])
    blocks = [(0, 21, Ts)] + [(21 + 3 * i, 24 + 3 * i, Tl[i]) for i in range(N)]
    n = 21 + 3 * N
    out = np.zeros((n, n))
    for bi, (a0, a1, Ta) in enumerate(blocks):
        TaS = {}
        for b0, b1, Tb in blocks[: bi + 1]:
            key = (b0, b1)
            TaS[key] = Ta @ S[a0:a1, b0:b1]
            v = r.o.tofloat(TaS[key] @ Tb.T)
            out[a0:a1, b0:b1] = v
            out[b0:b1, a0:a1] = v.T
    return out


def full_differential(N, kind_from, kind_to):
    """the differential at 0 of state_chart(kind_to, state_chart_inv(kind_from, .)) of the WHOLE state of case(N), at 50 digits, as floats"""
    r = _ref()
    (xi0, _, ids, q0, _), _ = case(N)
    st = State(r.sensor_from_flat(xi0), [int(i) for i in ids], r.o.arr(q0))
    D = _differential(r, lambda e: r.state_chart(kind_to, r.state_chart_inv(kind_from, e, st), st), 21 + 3 * N)
    return r.o.tofloat(D)


@lru_cache(maxsize=None)
def frame(N):
    """(camera, ids ascending, pixels) measuring every landmark of case(N)"""
    (xi0, Xs, ids, q0, Q), _ = case(N)
    cam = default_camera()
    mid, y = synth_measurement(np.random.default_rng(9200 + N), cam, ids, q0, Q, noise_px=1.0)
    return cam, mid, y
