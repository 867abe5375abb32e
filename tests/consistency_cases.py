"""Helper of the filter batch's consistency record tests (tests/test_batch_consistency_api.py, tests/test_gpu_batch_consistency.py), not a test.

A numpy restatement of what eqf_batch_consistency (include/eqf_batch.h) reports for one slot:
  eps          stateGroupAction(X^-1, truth truncated to the slot's ids, state order) (VIOGroup.cpp:24-55, 108-120), then the oracle's state_chart against xi0
               - the eps of VIO_eqf::computeNEES (VIO_eqf.cpp:153-170);
  block forms  x @ numpy.linalg.solve(M, x) on the rows of the oracle's Sigma, M the block's principal sub-matrix;
  lm_quad      the same for every landmark's 3 x 3 diagonal block;
  lm_err       |p_hat - p_true| with p_hat from OracleFilter.state_estimate.
and the planted cases: test_gpu_batch_nees.py's plant / spd recipe, Sigma with eigenvalues in [1e-3, 10]. Every principal sub-matrix of such a Sigma has its
eigenvalues in the same interval (Cauchy interlacing), so its condition number is <= 1e4 and a double-precision solve keeps about 1e4 * 2.2e-16 * n ~ 1e-12
relative, below the tests' 1e-9.
"""
import functools

import numpy as np

from batch_scenarios import reference_defaults
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH
from oracle_binding import OracleFilter
from test_gpu_batch_nees import plant, spd
from util import quat_mul, quat_rot, so3_exp

TOL = 1e-9
# EQF_BLOCK_* (include/eqf_batch.h): first row and size in eps / Sigma
BLOCKS = [("bias", 0, 6), ("attitude", 6, 3), ("position", 9, 3), ("pose", 6, 6), ("velocity", 12, 3), ("camera", 15, 6), ("sensor", 0, 21)]
# landmark counts: n = 21 (odd, padded), 24, 27 (odd), 36 (two full panels and a short one), 84, 213 (the maximum)
CASE_N = [0, 1, 2, 5, 21, 64]
CHARTS = [COORD_EUCLIDEAN, COORD_INVDEPTH]


def _conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _se3_mul(a, b):  # (qw, qx, qy, qz, x, y, z)
    return np.concatenate([quat_mul(a[:4], b[:4]), a[4:] + quat_rot(a[:4], b[4:])])


def _se3_inv(a):
    qi = _conj(a[:4])
    return np.concatenate([qi, -quat_rot(qi, a[4:])])


def state_error(Xs, Q, true_sensor, true_p):
    """stateGroupAction(X^-1, (true_sensor, true_p)): true_p in the state's landmark order. Returns the packed sensor state and the points."""
    beta, A, w, B = Xs[0:6], Xs[6:13], Xs[13:16], Xs[16:23]
    Ai, Bi = _se3_inv(A), _se3_inv(B)
    wi = -quat_rot(_conj(A[:4]), w)
    out = np.zeros(23)
    out[0:6] = true_sensor[0:6] - beta
    out[6:13] = _se3_mul(true_sensor[6:13], Ai)
    out[13:16] = quat_rot(_conj(Ai[:4]), true_sensor[13:16] - wi)
    out[16:23] = _se3_mul(_se3_mul(_se3_inv(Ai), true_sensor[16:23]), Bi)
    p = np.array([Q[i, 4] * quat_rot(Q[i, :4], true_p[i]) for i in range(len(Q))]).reshape(len(Q), 3)  # (Q_i^-1)^-1 p = a R p
    return out, p


def in_state_order(ids, true_ids, true_p):
    """The true points of the state's ids, state order (computeNEES's truncated state: the first true landmark of an id)."""
    true_ids = np.asarray(true_ids)
    return np.array([true_p[int(np.nonzero(true_ids == i)[0][0])] for i in ids]).reshape(len(ids), 3)


def eps_of(orc, state, truth):
    """The eps computeNEES forms. orc holds the state (set_eqf); state = (xi0, Xs, ids, q0, Q); truth = (sensor, ids, p)."""
    _, Xs, ids, _, Q = state
    es, ep = state_error(Xs, Q, truth[0], in_state_order(ids, truth[1], truth[2]))
    return orc.state_chart(es, ids, ep)


def quad(M, x):
    return float(x @ np.linalg.solve(M, x))


def expected_record(orc, state, truth):
    """The record of a slot that holds orc's EqF state, against truth: dict with the keys of VIOFilterBatch.consistency's records (without lu)."""
    ids = state[2]
    N, n = len(ids), 21 + 3 * len(ids)
    S = orc.get_sigma()
    eps = eps_of(orc, state, truth)
    _, eids, ep = orc.state_estimate()
    assert np.array_equal(eids, ids)
    tp = in_state_order(ids, truth[1], truth[2])
    return {
        "N": N,
        "nees": float(eps @ np.linalg.solve(S, eps)) / n,
        "block": np.array([quad(S[r:r + k, r:r + k], eps[r:r + k]) for _, r, k in BLOCKS]),
        "eps": eps,
        "sigma_diag": np.diag(S).copy(),
        "ids": np.asarray(ids, np.int32),
        "lm_quad": np.array([quad(S[21 + 3 * i:24 + 3 * i, 21 + 3 * i:24 + 3 * i], eps[21 + 3 * i:24 + 3 * i]) for i in range(N)]),
        "lm_err": np.linalg.norm(ep - tp, axis=1) if N else np.zeros(0),
    }


def rel(a, b):
    """test_gpu_batch_nees.py's measure, entry by entry."""
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)


def eps_floor(state, chart):
    """The size below which an entry of eps cannot be asked for to 1e-9 of itself. Every entry is a difference (or the logarithm of a quotient) of numbers of
    the size of the state - a Euclidean landmark entry is a R p - q0 with |q0| about 20, an InvDepth one is formed from unit vectors and 1 / |q0|, the pose
    entries from positions of a few metres - so it carries an absolute error of a few units in the last place of THAT size, however small it is itself. The
    floor is 8 such units over 1e-9: 1.8e-6 for sizes up to 1, 2.8e-5 at |q0| = 20 in the Euclidean chart. The planted cases keep every entry above it
    (planted_cases asserts that); an entry of a simulated filter's eps below it is measured against the floor (deviations)."""
    xi0, _, _, q0, _ = state
    size = max(1.0, float(np.max(np.abs(np.concatenate([xi0[10:16], xi0[20:23]])))))
    if chart == COORD_EUCLIDEAN and len(q0):
        size = max(size, float(np.max(np.abs(q0))))
    return 8.0 * float(np.spacing(size)) / TOL


def deviations(rec, exp, floor=0.0):
    """Per quantity, the largest deviation of a record from the helper's, entry by entry in the project's flat measure |a - b| / max(|b|, 1e-300). With a
    floor (eps_floor, for eps that is not planted; 0 for the planted cases), an entry of eps smaller than it is measured against the floor: |a - b| / max(|b|, floor)."""
    out = {key: float(np.max(rel(rec[key], exp[key]))) for key in ("block", "lm_quad", "lm_err") if len(exp[key])}
    out["eps"] = float(np.max(np.abs(rec["eps"] - exp["eps"]) / np.maximum(np.abs(exp["eps"]), max(floor, 1e-300))))
    return out


def worst_deviation(rec, exp, show=None, floor=0.0):
    d = deviations(rec, exp, floor)
    if show is not None:
        print(show, {k: f"{v:.2e}" for k, v in d.items()}, f"smallest |eps| {float(np.min(np.abs(exp['eps']))):.2e} floor {floor:.2e}")
    return max(d.values())


def away_from_zero(rng, size, scale):
    """offsets of either sign with magnitude in [0.5, 1.5] * scale"""
    return rng.choice([-1.0, 1.0], size=size) * rng.uniform(0.5, 1.5, size=size) * scale


def moved_sensor(sensor, rng):
    """The packed sensor state moved in every component by an offset bounded away from 0: biases about 1e-3, velocity, attitudes and positions of pose and
    camera offset about 1e-2."""
    ts = np.array(sensor, dtype=np.float64)
    ts[0:6] += away_from_zero(rng, 6, 1e-3)
    ts[13:16] += away_from_zero(rng, 3, 1e-2)
    for q, x in ((6, 10), (16, 20)):  # pose, camera offset
        ts[q:q + 4] = quat_mul(ts[q:q + 4], so3_exp(away_from_zero(rng, 3, 1e-2)))
        ts[x:x + 3] += away_from_zero(rng, 3, 1e-2)
    return ts


def truth_with_extras(orc, rng, extras=3):
    """A true state near the estimate, off it in every component (test_gpu_batch_nees.py's true_of moves the biases, the velocity and the points only, which
    leaves the pose and camera entries of eps at exactly 0) by offsets bounded away from 0, its ids shuffled among `extras` ids the slot does not hold."""
    es, eids, ep = orc.state_estimate()
    ts = moved_sensor(es, rng)
    tids = np.concatenate([eids, 10 ** 6 + np.arange(extras, dtype=np.int32)]).astype(np.int32)
    tp = np.concatenate([ep + away_from_zero(rng, ep.shape, 1e-1), rng.uniform(-1, 1, (extras, 3)) * 5.0 + np.array([0, 0, 20.0])])
    perm = rng.permutation(len(tids))
    return ts, tids[perm], tp[perm]


@functools.lru_cache(maxsize=None)
def planted_cases():
    """Every chart x landmark count: dicts with chart, N, settings, state, S, truth, orc (holding state and S) and exp (expected_record). Built once."""
    cases = []
    for chart in CHARTS:
        rng = np.random.default_rng(1300 + chart)
        s = reference_defaults(coordinateChoice=chart)
        for N in CASE_N:
            state, V, lam = plant(rng, N, chart)
            S = spd(V, lam)
            orc = OracleFilter(s)
            orc.set_eqf(*state, S)
            truth = truth_with_extras(orc, rng)
            exp = expected_record(orc, state, truth)
            assert np.min(np.abs(exp["eps"])) >= eps_floor(state, chart), (chart, N, np.min(np.abs(exp["eps"])), eps_floor(state, chart))
            cases.append({"chart": chart, "N": N, "settings": s, "state": state, "S": S, "truth": truth, "orc": orc, "exp": exp})
    return cases
