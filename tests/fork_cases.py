"""Forking a context and changing its chart on the device (helper module, not a test): eqf_copy_ctx, eqf_convert_chart, k_ctx_copy / k_ctx_rechart
(eqvio_amd/csrc/eqf_fork.hpp). The planted states, Sigma and the changes of coordinates T are tests/rechart_cases.py's - case(N), T(N, a, b), expected(N, a, b),
built without the product's code - at the sizes the context's kernel needs beside rechart_cases.NS:

 * k_ctx_rechart cuts Sigma into row groups along landmark boundaries: the 21 sensor rows, then RC_G = 16 landmarks per group. Every multiple of 16 is a group
   boundary; the sizes take the last landmark of a group and the first of the next at the first, second and fourth boundary (16 | 17, 32 | 33, 64 | 65);
 * N = 200 (13.5 groups: 105 tiles) and N = 520 (33.5 groups: 595 tiles - more tiles than compute units, a ragged last group).
The 50-digit construction of T takes 3.3 s at N = 520 with the Normal chart's blocks (1.3 s at N = 200), so all six ordered pairs run at every size.

block_congruence(T, S): T S T^T block by block - the sum order of the device's kernel, not numpy's dense one."""
import numpy as np

import rechart_cases as rcs

RC_G = 16  # eqf_fork.hpp
BOUNDARY_NS = [16, 17, 32, 33, 65]  # (64 is in rechart_cases.NS)
SIZES = sorted(set(rcs.NS) | set(BOUNDARY_NS) | {200, 520})
NEW_SIZES = [N for N in SIZES if N not in rcs.NS]
MP_MAX = 64  # the 50-digit product T Sigma T^T is affordable up to here


def groups(N):
    """[(first row, one past the last row)] of k_ctx_rechart's row groups"""
    out = [(0, 21)]
    for l0 in range(0, N, RC_G):
        out.append((21 + 3 * l0, 21 + 3 * min(N, l0 + RC_G)))
    return out


def block_congruence(Tm, S):
    """T S T^T with T block diagonal (21 x 21, then 3 x 3 per landmark): per block pair (T_a S_ab) first, then (. T_b^T); lower triangle, mirrored"""
    n = len(S)
    N = (n - 21) // 3
    Ts = Tm[:21, :21]
    Tl = np.stack([Tm[21 + 3 * i:24 + 3 * i, 21 + 3 * i:24 + 3 * i] for i in range(N)]) if N else np.zeros((0, 3, 3))
    out = np.zeros_like(S)
    out[:21, :21] = np.tril((Ts @ S[:21, :21]) @ Ts.T)
    if N:
        S_ls = S[21:, :21].reshape(N, 3, 21)  # landmark rows, sensor columns
        out[21:, :21] = (np.einsum("iab,ibc->iac", Tl, S_ls) @ Ts.T).reshape(3 * N, 21)
        S_ll = S[21:, 21:].reshape(N, 3, N, 3)
        P = np.einsum("iab,ibjc->iajc", Tl, S_ll)
        out[21:, 21:] = np.tril(np.einsum("iajc,jdc->iajd", P, Tl).reshape(3 * N, 3 * N))
    low = np.tril(out)
    return low + np.tril(low, -1).T
