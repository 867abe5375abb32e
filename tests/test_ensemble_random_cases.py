"""tests/ensemble_random_cases.py proved on the CPU: the restated Philox4x64-10 is np.random.Philox word for word (numpy's carry between counter words
included), U is exact, open and symmetric, the restated normals of (2026, 0) look Gaussian by three conditions fixed in advance, and they pass the
reference's initial-distribution check (test/test_FilterStatistics.cpp:98) with half its band to spare.

Seen on the restatement, 256 x 256 normals of (seed, stream) = (2026, 0), (2026, 1), (1, 0): mean sqrt(n) 0.83, -0.28, -0.67; (var - 1) / sqrt(2 / n) 0.89,
-0.19, -1.41; Kolmogorov distance sqrt(n) 0.62, 0.75, 0.87 (1.36 is the 5 % point of the Kolmogorov distribution)."""
import numpy as np
import pytest

from ensemble_cases import STAT_BANDS, STAT_SEEDS, StatFixture
from ensemble_random_cases import MASK64, cached_normals, gaussian_summary, mulhi, numpy_block, philox4x64_10, uniforms, unit

KEYS = [(0, 0), (2026, 0), (2026, 1), (1, 0), (MASK64, MASK64), (0x0123456789ABCDEF, 0xFEDCBA9876543210)]
COUNTERS = [
    (0, 0, 0, 0), (1, 0, 0, 0), (5, 256, 0, 0), (8, 999, 0, 0), (64, 0, 0, 1), (0, 0, 0, 1),
    (MASK64, 4, 0, 0),   # word 0 is 2^64 - 1 ...
    (0, 5, 0, 0),        # ... and its successor: numpy reaches it by a carry into word 1
    (0, 0, 1, 0),        # a carry through two words
    (MASK64, MASK64, MASK64, MASK64),
]


def test_mulhi_from_halves_is_the_high_word():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1 << 64, 200, dtype=np.uint64)
    b = rng.integers(0, 1 << 64, 200, dtype=np.uint64)
    a[:3], b[:3] = (MASK64, 0, MASK64), (MASK64, MASK64, 1)
    assert [int(v) for v in mulhi(a, b)] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]


@pytest.mark.parametrize("key", KEYS, ids=[f"key{i}" for i in range(len(KEYS))])
def test_restatement_is_numpys_philox_word_for_word(key):
    for c in COUNTERS:
        mine = [int(w) for w in philox4x64_10(key[0], key[1], *c)]
        ref = [int(w) for w in numpy_block(key[0], key[1], sum(w << (64 * i) for i, w in enumerate(c)))]
        assert mine == ref, (key, c)


def test_a_run_of_counters_is_numpys_stream():
    """numpy's own sequence from counter 0: blocks 1, 2, 3, ... in order"""
    raw = np.random.Philox(key=np.array([2026, 3], np.uint64), counter=np.zeros(4, np.uint64)).random_raw(4 * 50).reshape(50, 4)
    mine = np.stack(philox4x64_10(2026, 3, np.arange(1, 51, dtype=np.uint64), np.uint64(0), np.uint64(0), np.uint64(0)), axis=1)
    assert np.array_equal(raw, mine)


def test_unit_is_exact_open_and_symmetric():
    rng = np.random.default_rng(8)
    x = rng.integers(0, 1 << 64, 4096, dtype=np.uint64)
    x[:4] = (0, MASK64, 1 << 12, (1 << 63) - 1)
    u = unit(x)
    assert np.all(u > 0.0) and np.all(u < 1.0)
    assert u[0] == 2.0**-53 and u[1] == 1.0 - 2.0**-53
    # exact: an odd integer below 2^53 times 2^-53
    from fractions import Fraction

    for xv, uv in zip(x[:64], u[:64]):
        assert Fraction(float(uv)) == Fraction(2 * (int(xv) >> 12) + 1, 1 << 53)
    assert np.all(u + unit(~x) == 1.0)
    assert np.all(2.0 * u == np.ldexp(u, 1))


def test_uniforms_layout():
    u = uniforms(2026, 0, 9)
    w = philox4x64_10(2026, 0, np.arange(3, dtype=np.uint64), np.uint64(0), np.uint64(0), np.uint64(1))
    for i in range(9):
        assert u[i] == unit(w[i & 3][i >> 2])
    assert np.array_equal(uniforms(2026, 0, 5), u[:5])


def test_normals_layout_and_subset_rule():
    z = cached_normals(2026, 0, 33, 40)
    for (j, k) in ((0, 0), (5, 39), (8, 17)):
        x = philox4x64_10(2026, 0, np.uint64(j), np.uint64(k), np.uint64(0), np.uint64(0))
        r = np.sqrt(-2.0 * np.log(unit(x[0])))
        assert z[4 * j, k] == r * np.cos(2.0 * np.pi * unit(x[1]))
        if 4 * j + 1 < 33:
            assert z[4 * j + 1, k] == r * np.sin(2.0 * np.pi * unit(x[1]))
    assert np.array_equal(cached_normals(2026, 0, 5, 33), z[:5, :33])
    assert not np.array_equal(cached_normals(2027, 0, 5, 33), z[:5, :33]) and not np.array_equal(cached_normals(2026, 1, 5, 33), z[:5, :33])


def test_restated_normals_look_gaussian():
    m, v, ks = gaussian_summary(cached_normals(2026, 0, 256, 256))
    print(f"[ensemble random] restated normals (2026, 0) 256 x 256: |mean| sqrt(n) {m:.2f}, |var - 1| / sqrt(2 / n) {v:.2f}, Kolmogorov sqrt(n) {ks:.2f}")
    assert m <= 3.0
    assert v <= 3.0
    assert ks <= 1.36


def test_restated_normals_pass_the_initial_distribution_check():
    f = StatFixture(2, 1000, STAT_SEEDS[(2, "initial")])
    xi = cached_normals(2026, 0, f.n, 1000)
    mean = float(np.mean(np.einsum("ik,ik->k", xi, xi) / f.n))
    print(f"[ensemble random] N=2 P=1000 mean |xi|^2 / n = {mean:.6f} (band {STAT_BANDS['initial']})")
    assert abs(mean - 1.0) <= 0.5 * STAT_BANDS["initial"]
