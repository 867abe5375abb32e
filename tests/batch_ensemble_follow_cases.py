"""Planted cases of eqf_bens_follow (eqvio_amd/csrc/eqf_batch_ensemble_follow.h): tests/test_batch_ensemble_follow_cases.py proves them on the CPU,
tests/test_gpu_batch_ensemble_follow.py runs them on the device.

A case is (chart, |K|, N, P, variant, foreign): the planted filter ensemble_cases.Case(chart, N, P) over N landmarks, and a cloud of P particles that holds
the filter's first |K| landmarks and `foreign` ids the filter does not know - "order": the kept ones in the slot's order with the foreign ones behind them;
"shuffled" and "foreign": in another order. The particles are the case's own draw eps = L Xi with Xi = cached_normals(SEED, 0, n, P) through the exact chart
inverse (Case.sampled), cut back to the kept landmarks; the foreign landmarks' points are arbitrary.

Truth, with numpy alone: L = numpy's cholesky(Sigma); eps_K the rows of the case's restated error (Case.restated_errors) over the sensor and the kept landmarks;
z_K = L_KK^-1 eps_K by a triangular solve; eps_A = L_AK z_K + L_AA Xi_A with Xi = cached_normals(SEED, stream, n, P), rows n_K .. n - 1; the added points by the
restated inverse chart and group action (oracle/indep/eqvio_ref.py). Nothing here calls the product. A reference is computed once per case and shared.

Admission. A case enters the table only if this fp64 restatement agrees to 1e-11 with the same arithmetic at higher precision (admission()): mpmath at 50
digits for the factor, the solve, eps_A and - for the first, middle and last particle - the charts (EqVIORef(MP(50)), as oracle/indep does); at N = 64 the
factor of a 213 x 213 matrix in mpmath takes minutes, so there the linear algebra is repeated in np.longdouble (64-bit mantissa) and the charts stay at 50
digits."""
import functools

import numpy as np

from ensemble_cases import CHART_NAMES, Case, R, flat_sensor, planted_sigma  # noqa: F401  (planted_sigma: the Sigma every Case plants)
from ensemble_random_cases import cached_normals

SEED = 2026
STREAM_0 = 0  # the stream of the clouds' own draw
STREAM_F = 5  # the stream of the parity cases' follow
ADMIT = 1e-11
MP_MAX_N = 26  # mpmath linear algebra up to n = 99; np.longdouble above

# (|K|, N): 0 -> 1 and 1 -> 2 the smallest; 5 -> 6 n odd (39); 7 -> 8; 9 -> 10 and 9 -> 12 the split n_K = 48 on a tile edge; 15 -> 17 and 16 -> 17 on either
# side of n_K = 69 (n_K mod 4 = 2 and 1: a partly used row block of normals); 25 -> 26 the split n_K = 96 on a tile edge; 60 -> 64, 63 -> 64 and 0 -> 64 the
# capacity (n = 213, padded); 3 -> 3 a pure reorder; "4 -> 2" a cloud of 4 over a slot of 2: drops only.
SHAPES = ((0, 1), (1, 2), (5, 6), (7, 8), (9, 10), (9, 12), (15, 17), (16, 17), (25, 26), (60, 64), (63, 64), (0, 64), (3, 3), (2, 2))
SIZES_P = (1, 2, 15, 16, 17, 33, 257)
VARIANTS = ("order", "shuffled", "foreign")

# chart, |K|, N, P, variant, foreign ids
TABLE = [
    (0, 0, 1, 1, "order", 0), (1, 0, 1, 17, "foreign", 3), (2, 0, 1, 257, "foreign", 1),
    (1, 1, 2, 2, "order", 0), (2, 1, 2, 33, "foreign", 2),
    (2, 5, 6, 15, "order", 0), (0, 5, 6, 257, "shuffled", 0), (1, 5, 6, 16, "foreign", 3),
    (0, 7, 8, 16, "shuffled", 0), (1, 7, 8, 1, "foreign", 1),
    (1, 9, 10, 17, "order", 0), (2, 9, 10, 33, "shuffled", 0), (0, 9, 10, 2, "foreign", 2),
    (2, 9, 12, 257, "order", 0), (0, 9, 12, 15, "foreign", 3),
    (0, 15, 17, 33, "shuffled", 0), (1, 15, 17, 2, "foreign", 1),
    (1, 16, 17, 15, "order", 0), (2, 16, 17, 16, "shuffled", 0),
    (2, 25, 26, 17, "shuffled", 0), (0, 25, 26, 33, "foreign", 2),
    (0, 60, 64, 16, "order", 0), (1, 60, 64, 33, "foreign", 3),
    (1, 63, 64, 2, "shuffled", 0), (2, 63, 64, 17, "foreign", 1),
    (2, 0, 64, 15, "order", 0), (0, 0, 64, 33, "foreign", 3),
    (0, 3, 3, 257, "shuffled", 0), (1, 3, 3, 16, "shuffled", 0),
    (1, 2, 2, 33, "order", 2), (2, 2, 2, 1, "foreign", 2),
]
assert {(t[1], t[2]) for t in TABLE} == set(SHAPES) and {t[3] for t in TABLE} == set(SIZES_P) and {t[0] for t in TABLE} == {0, 1, 2}
assert all({t[4] for t in TABLE if (t[1], t[2]) == s} - {"order"} for s in SHAPES)  # every shape also with a cloud that is not in the slot's order


def key(chart, nK, N, P, variant, nf):
    return f"{CHART_NAMES[chart]}-{nK + nf if nK == N else nK}to{N}-P{P}-{variant}{nf or ''}"


@functools.lru_cache(maxsize=None)
def seeded_case(chart, N, P):
    c = Case(chart, N, P)
    c.xi = np.array(cached_normals(SEED, STREAM_0, c.n, P))
    return c


def conditional_eps(L, epsK, xi):
    """[eps_K ; eps_A] with z_K = L_KK^-1 eps_K and eps_A = L_AK z_K + L_AA Xi_A, and z_K itself"""
    from scipy.linalg import solve_triangular

    nk = epsK.shape[0]
    zK = solve_triangular(L[:nk, :nk], epsK, lower=True) if nk else epsK
    epsA = L[nk:, :nk] @ zK + L[nk:, nk:] @ xi[nk:]
    return np.vstack([epsK, epsA]), zK


def points_of(c, eps, lo):
    """the points of landmarks lo .. N - 1 of state_action(X, state_chart_inv(eps_k ; xi0)) for every column of eps: (P, N - lo, 3)"""
    out = np.zeros((eps.shape[1], c.N - lo, 3))
    for k in range(eps.shape[1]):
        for i in range(lo, c.N):  # a landmark's point depends on its own three rows alone (state_chart_inv, state_action)
            out[k, i - lo] = (c.X.QR[i].T @ R.point_chart_inv(c.kind, eps[21 + 3 * i:24 + 3 * i, k], c.xi0.p[i])) / c.X.Qa[i]
    return out


class FollowCase:
    def __init__(self, chart, nK, N, P, variant, nf, stream=STREAM_F):
        c = self.c = seeded_case(chart, N, P)
        self.chart, self.nK, self.N, self.P, self.variant, self.nf, self.stream = chart, nK, N, P, variant, nf, stream
        self.n, self.nk = c.n, 21 + 3 * nK
        rng = np.random.default_rng([77, chart, nK, N, P, VARIANTS.index(variant), nf])
        sens, pts = c.sampled
        self.sensor = np.ascontiguousarray(sens)
        self.kept_p = np.ascontiguousarray(pts[:, :nK])
        ids = np.concatenate([c.ids[:nK], 200001 + np.arange(nf)]).astype(np.int32)
        p = np.concatenate([self.kept_p, rng.uniform(-1, 1, (P, nf, 3)) + np.array([0, 0, 12.0])], axis=1)
        self.perm = np.arange(nK + nf)
        if variant != "order" and nK + nf > 1:
            while np.array_equal(self.perm, np.arange(nK + nf)):
                self.perm = rng.permutation(nK + nf)
        self.cloud = (ids[self.perm], self.sensor, np.ascontiguousarray(p[:, self.perm]))  # what eqf_bens_set is handed
        self.xi = cached_normals(SEED, stream, c.n, P)

    @functools.cached_property
    def epsK(self):
        """the restated error over the sensor rows and the kept landmarks (a landmark's rows depend on that landmark alone)"""
        return self.c.restated_errors(self.c.ids, *self.c.sampled)[:self.nk]

    @functools.cached_property
    def eps(self):
        return conditional_eps(self.c.L, self.epsK, self.xi)[0]

    @functools.cached_property
    def added_p(self):
        return points_of(self.c, self.eps, self.nK)

    @functools.cached_property
    def nees(self):
        from scipy.linalg import solve_triangular

        y = solve_triangular(self.c.L, self.eps, lower=True)
        return np.einsum("ik,ik->k", y, y) / self.n

    # what the plan of the entry must be
    @property
    def moves(self):
        return not np.array_equal(self.cloud[0][:self.nK], self.c.ids[:self.nK])

    @property
    def counts(self):
        return self.nf, self.N - self.nK  # (dropped, added)


@functools.lru_cache(maxsize=None)
def get_case(*k):
    return FollowCase(*k)


def admission(fc):
    """(eps_A, points): the largest deviation of the fp64 restatement from the same arithmetic at higher precision, eps_A relative to its largest entry, the added
    points relative to max(1, |value|). The charts run at 50 digits for the first, middle and last particle."""
    import mpmath as mp
    from eqvio_ref import MP, EqVIORef, State

    c, nk, n = fc.c, fc.nk, fc.n
    if fc.N == fc.nK:
        return 0.0, 0.0
    RM = EqVIORef(MP(50))
    picks = sorted({0, fc.P // 2, fc.P - 1})
    xi0 = RM.state_from_flat(c.xi0f, c.ids, c.q0.reshape(c.N, 3))
    X = RM.group_from_flat(c.Xsf, c.ids, c.Q.reshape(c.N, 5))
    Xinv = RM.group_inv(X)
    sens, pts = c.sampled
    epsK = np.empty((nk, len(picks)), dtype=object)
    for col, k in enumerate(picks):
        st = State(RM.sensor_from_flat(sens[k]), X.ids, RM.o.arr(pts[k]))
        epsK[:, col] = RM.state_chart(c.kind, RM.state_action(Xinv, st), xi0)[:nk]
    if fc.N <= MP_MAX_N:
        S = RM.o.arr(c.Sigma)
        L = RM.o.zeros(n, n)
        for j in range(n):
            L[j, j] = mp.sqrt(S[j, j] - sum((L[j, t] * L[j, t] for t in range(j)), mp.mpf(0)))
            for i in range(j + 1, n):
                L[i, j] = (S[i, j] - sum((L[i, t] * L[j, t] for t in range(j)), mp.mpf(0))) / L[j, j]
        one = mp.mpf(1)
    else:  # np.longdouble: 64-bit mantissa
        S = np.asarray(c.Sigma, np.longdouble)
        L = np.zeros((n, n), np.longdouble)
        for j in range(n):
            L[j, j] = np.sqrt(S[j, j] - L[j, :j] @ L[j, :j])
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        one = np.longdouble(1)
    worst_e = worst_p = 0.0
    for col, k in enumerate(picks):
        y = [one * 0] * n  # [z_K ; Xi_A]
        rhs = [v if fc.N <= MP_MAX_N else np.longdouble(float(v)) for v in epsK[:, col]]
        for i in range(nk):
            y[i] = (rhs[i] - sum((L[i, t] * y[t] for t in range(i)), one * 0)) / L[i, i]
        for i in range(nk, n):
            y[i] = one * float(fc.xi[i, k])
        epsA = [sum((L[i, t] * y[t] for t in range(i + 1)), one * 0) for i in range(nk, n)]
        ref_e = np.array([float(v) for v in epsA])
        worst_e = max(worst_e, float(np.max(np.abs(fc.eps[nk:, k] - ref_e)) / np.max(np.abs(ref_e))))
        eA = RM.o.arr([mp.mpf(float(v)) if fc.N > MP_MAX_N else v for v in epsA])
        ref_p = np.array([RM.o.tofloat((X.QR[i].T @ RM.point_chart_inv(c.kind, eA[3 * (i - fc.nK):3 * (i - fc.nK) + 3], xi0.p[i])) / X.Qa[i]) for i in range(fc.nK, c.N)])
        worst_p = max(worst_p, float(np.max(np.abs(fc.added_p[k] - ref_p) / np.maximum(1.0, np.abs(ref_p)))))
    return worst_e, worst_p


# ---- the regeneration identity: a cloud drawn as eps = L Xi(SEED, STREAM_0), cut back to its first |K| landmarks and followed with the same (seed, stream)
def regenerated(fc):
    """(added points of the follow with the cloud's own stream, the cloud's original points of those landmarks)"""
    eps = conditional_eps(fc.c.L, fc.epsK, cached_normals(SEED, STREAM_0, fc.n, fc.P))[0]
    return points_of(fc.c, eps, fc.nK), fc.c.sampled[1][:, fc.nK:]


REGEN = [(1, 5, 6, 16, "foreign", 3), (2, 9, 12, 257, "order", 0), (0, 15, 17, 33, "shuffled", 0), (1, 60, 64, 33, "foreign", 3), (2, 0, 64, 15, "order", 0)]
assert all(t in TABLE for t in REGEN)

# ---- five entries over a 7-slot batch, in the call's order, and the two slots the call does not list: (slot, case)
FIVE = [(6, (1, 5, 6, 16, "foreign", 3)), (0, (0, 0, 1, 1, "order", 0)), (3, (2, 9, 12, 257, "order", 0)), (5, (0, 3, 3, 257, "shuffled", 0)), (1, (0, 25, 26, 33, "foreign", 2))]
OTHERS = [(2, (1, 2, 2, 33, "order", 2)), (4, (2, 16, 17, 16, "shuffled", 0))]
assert all(c in TABLE for _, c in FIVE + OTHERS)
MAXP = 257


# ---- the statistical case: StatFixture's N = 2, P = 1000 (InvDepth there; here one slot per chart). One id leaves and two arrive by augment: n = 30.
class StatCase:
    """The slot after the turnover in the restatement: landmark ids (1, 7, 8) - id 0 has left, 7 and 8 are new with Sigma_AK = 0 and the initial point variance -
    and the followed cloud's eps: the kept rows of the first draw (sensor and landmark 1: eps = L0 Xi0 restricted, L0 diagonal) and fresh normals for the new block."""

    def __init__(self, seed=1, P=1000, stream=11):
        from ensemble_cases import StatFixture

        f = self.f = StatFixture(2, P, seed)
        self.P, self.n, self.stream = P, 30, stream
        d0 = np.diag(f.sigma0)
        keep = np.r_[0:21, 24:27]  # the sensor rows and landmark id 1
        new_var = d0[21:24]  # a new landmark's block is the initial one (eqf_batch_augment)
        self.sigma = np.diag(np.concatenate([d0[keep], new_var, new_var]))
        L = np.linalg.cholesky(self.sigma)
        xi0 = cached_normals(SEED, STREAM_0, 27, P)
        epsK = (np.sqrt(d0)[:, None] * xi0)[keep]
        self.eps = conditional_eps(L, epsK, cached_normals(SEED, stream, 30, P))[0]
        y = np.linalg.solve(L, self.eps)
        self.mean_nees = float(np.mean(np.einsum("ik,ik->k", y, y) / 30.0))
