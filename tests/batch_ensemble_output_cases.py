"""Planted cases of the measurement side of the particle ensembles against batch slots (include/eqf_batch_ensemble_output.h):
tests/test_batch_ensemble_output_cases.py proves them on the CPU, tests/test_gpu_batch_ensemble_output.py runs them on the device.

A likelihood case is tests/ensemble_output_cases.OutputCase(cam, M, P): P particles over N = M + 2 landmarks (two more than are measured, in another order), so
M <= 62 fits a slot's 64 landmarks. A resampling case adds the measurement variance, P_new and the stream of its uniforms, cached_uniforms(SEED, stream,
P_new) - the draw eqf_bens_resample_weighted_seeded is defined by. A covariance case is tests/ensemble_cases.Case(chart, N, P) with its normals replaced by
cached_normals(SEED, 0, n, P), as tests/test_gpu_batch_ensemble.py plants its filters. Everything that is "truth" is restated with oracle/indep/eqvio_ref.py and
numpy; nothing here calls the product. A reference is computed once per case and shared."""
import functools

import numpy as np

from ensemble_cases import Case
from ensemble_output_cases import MEAS_VAR, get_case, log_weights, margin, weighted_resample
from ensemble_random_cases import cached_normals, cached_uniforms

SEED = 2026
MARGIN = 1e-9  # the project's condition under which device and sequential indices must agree (ensemble_output_cases.MARGIN_GPU)

# ---- likelihood parity: all three cameras, the eight lane groups and the 64-landmark capacity, 32 particles per workgroup and R = 1, 2, 3 in the weights kernel
SIZES_M = (0, 1, 2, 7, 8, 9, 11, 62)
SIZES_P = (1, 2, 31, 32, 33, 255, 256, 257, 513)
SMALL_M = (0, 1, 2)  # P = 513 runs with these only: the restatement walks every (particle, landmark) in Python


def likelihood_cases():
    """(camera, M, P): every M with every camera and every P with some camera; P = 513 with small M only, M = 62 with P <= 33"""
    out = []
    for c in range(3):
        for i, M in enumerate(SIZES_M):
            P = SIZES_P[(i + 3 * c) % len(SIZES_P)]
            if P == 513 and M not in SMALL_M:
                P = 255
            if M == 62:
                P = (31, 32, 33)[c]
            out.append((c, M, P))
    out += [(0, 1, 513), (1, 0, 513), (1, 9, 256), (2, 7, 257), (0, 11, 2)]
    return out


def lik_key(cam, M, P):
    return f"cam{cam}-M{M}-P{P}"


def loglik_at(c, var):
    """the restated log-likelihoods of OutputCase c at another measurement variance"""
    return -0.5 * c.quad * (c.var / var)


PLANTED_UNDERFLOW = (0, 62, 31, MEAS_VAR)  # (camera, M, P, meas_var): the reference's plain exp(-q / 2) sums to exactly 0.0 here

# ---- resampling: (camera, M, P, P_new, stream, meas_var)
RESAMPLE = [
    (0, 2, 33, 33, 1, 400.0),
    (1, 11, 257, 257, 2, 4000.0),
    (1, 2, 257, 300, 5, 400.0),
    (0, 2, 255, 256, 8, 400.0),
    (0, 11, 16, 17, 10, 4000.0),
    (0, 5, 257, 1, 4, 400.0),
    (2, 1, 1, 33, 3, 4.0),
    (2, 62, 31, 31, 7, 40000.0),  # the 64-landmark capacity: variance and stream chosen as the others were, asserted in tests/test_batch_ensemble_output_cases.py
]
MAXP = 300  # room of the test ensembles
STAT_STREAM = 6  # the stream of the reference's output check at StatFixture's N = 2, P = 1000 (its margin: tests/test_batch_ensemble_output_cases.py)


def res_key(cam, M, P, Pn, stream, var):
    return f"cam{cam}-M{M}-P{P}to{Pn}-s{stream}-v{var:g}"


class ResampleCase:
    def __init__(self, cam, M, P, Pn, stream, var):
        self.c, self.Pn, self.stream, self.var = get_case(cam, M, P), Pn, stream, var
        self.u = cached_uniforms(SEED, stream, Pn)
        self.loglik = loglik_at(self.c, var)
        self.w = log_weights(self.loglik)[0]
        self.margin = margin(self.w, self.u)
        self.src = weighted_resample(self.w, self.u)


@functools.lru_cache(maxsize=None)
def resample_case(cam, M, P, Pn, stream, var):
    return ResampleCase(cam, M, P, Pn, stream, var)


# ---- five entries over a 7-slot batch, in the call's order: (slot, likelihood case, meas_var, P_new, stream)
FIVE = [(6, (1, 11, 257), 4000.0, 257, 2), (0, (2, 1, 1), 4.0, 33, 3), (3, (0, 2, 33), 400.0, 33, 1), (5, (2, 62, 31), 40000.0, 31, 7), (1, (0, 5, 257), 400.0, 1, 4)]
OTHERS = [(2, (0, 2, 255), 400.0, 256, 8), (4, (0, 11, 16), 4000.0, 17, 10)]  # the two slots the 5-entry call does not list

# ---- covariance: (chart, N, P). n = 21, 24, 45, 48, 51, 213: the 16 x 16 tile edges; P: the steps of 4
COV_N = (0, 1, 8, 9, 10, 64)
COV_P = (1, 2, 3, 4, 5, 33, 257)
COV_CASES = [(0, 0, 1), (0, 1, 2), (0, 8, 3), (0, 9, 4), (0, 10, 5), (0, 64, 33), (1, 0, 257), (1, 1, 33), (1, 8, 5), (1, 9, 257), (1, 10, 2), (1, 64, 3),
             (2, 0, 4), (2, 1, 5), (2, 8, 257), (2, 9, 1), (2, 10, 33), (2, 64, 2)]
COV_FIVE = [(6, (1, 9, 257)), (0, (0, 0, 1)), (3, (2, 10, 33)), (5, (0, 64, 33)), (1, (2, 1, 5))]
COV_OTHERS = [(2, (0, 8, 3)), (4, (1, 1, 33))]
assert all(c in COV_CASES for _, c in COV_FIVE + COV_OTHERS)
assert {c[1] for c in COV_CASES} == set(COV_N) and {c[2] for c in COV_CASES} == set(COV_P) and {c[0] for c in COV_CASES} == {0, 1, 2}


def cov_key(chart, N, P):
    return f"chart{chart}-N{N}-P{P}"


@functools.lru_cache(maxsize=None)
def seeded_case(chart, N, P):
    c = Case(chart, N, P)
    c.xi = np.array(cached_normals(SEED, 0, c.n, P))
    return c


def cov_truth(c):
    """(ids, sensor, p) handed to the device and the restated eps (n, P): the sampled particles with two more landmarks in another order, or, where 66
    landmarks do not fit a cloud, the filter's own in another order"""
    ids, sens, p = c.truth_x
    if c.N + 2 > 64:
        keep = c.perm[c.perm < c.N]
        ids, p = c.ids[keep], np.ascontiguousarray(c.sampled[1][:, keep])
    return (ids, sens, p), c.restated_errors(ids, sens, p)


@functools.lru_cache(maxsize=None)
def cov_reference(chart, N, P):
    c = seeded_case(chart, N, P)
    truth, eps = cov_truth(c)
    return truth, eps, eps @ eps.T / P
