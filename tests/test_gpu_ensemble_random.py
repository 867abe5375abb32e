"""The ensemble's seeded draws on the device (include/eqf_ensemble_random.h, ParticleEnsemble.normals / uniforms / sample_seeded / resample_weighted_seeded /
integrate_seeded) against the numpy restatement of tests/ensemble_random_cases.py and against the unseeded calls.

Bounds. uniforms: byte-identical to the restatement - the path is integer arithmetic and one exact conversion. normals: 1e-13 absolute. numpy rounds the
argument 2 pi U (at most 2 pi 2^-53 ~ 7e-16 of angle) where the device's sincospi takes 2 U exactly, a few ulp of the two libraries' log, sqrt, sin and cos
come on top, and all of it is multiplied by r <= sqrt(2 * 53 * ln 2) ~ 8.6: under 1e-14, so the bound has a margin of ten. Every seeded call is held to its
unseeded twin BYTE FOR BYTE (both sides run the same kernels on the same doubles), so no margin condition is needed anywhere. The identity NEES = |xi|^2 / n
keeps the bound of test_gpu_ensemble.py: ten times what the restatement itself loses on that filter (tests/golden/ensemble_identity_baseline.json), floor
1e-12. Seen values are printed (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from ensemble_cases import STAT_BANDS, STAT_SEEDS, StatFixture, case_key, get_case, load_baseline, size_cases
from ensemble_output_cases import device_camera
from ensemble_output_cases import get_case as get_output_case
from ensemble_random_cases import cached_normals, cached_uniforms
from eqvio_amd.capi import COORD_INVDEPTH, OPT_SIGMA_FP32, EqfCore, EqfError
from eqvio_amd.ensemble import ParticleEnsemble

pytestmark = pytest.mark.gpu
SEED, STREAM = 2026, 0
BIG = (1, 11, 257)  # the 257-particle case of ensemble_output_cases.py


def make_core(c):
    core = EqfCore(max(c.N, 1), c.chart)
    core.set_state(c.xi0f, c.Xsf, c.ids, c.q0, c.Q)
    core.set_sigma(c.Sigma)
    return core


def ens_bytes(ens):
    ids, s, p = ens.get()
    return ens.size, ids.tobytes(), s.tobytes(), p.tobytes()


def counters(core):
    lib, h = core.lib, core.h
    la, lf = C.c_long(), C.c_long()
    lib.eqf_lookahead_stats(h, C.byref(la), C.byref(lf), 0)
    a, b, c = C.c_long(), C.c_long(), C.c_long()
    lib.eqf_speculation_stats(h, C.byref(a), C.byref(b), C.byref(c), 0)
    calls, secs = (C.c_long * 2)(), (C.c_double * 2)()
    lib.eqf_host_wait_stats(h, calls, secs, 0)
    return (la.value, lf.value, a.value, b.value, c.value, core.fork_stats(), core.nees_lu_fallbacks(), calls[1], core.innovation_totals())


def ctx_bytes(core):
    xi0, Xs, ids, q0, Q = core.get_state()
    return xi0.tobytes(), Xs.tobytes(), ids.tobytes(), q0.tobytes(), Q.tobytes(), core.get_sigma().tobytes(), core.last_gamma().tobytes()


def code_of(call):
    with pytest.raises(EqfError) as e:
        call()
    return e.value.code


@pytest.fixture(scope="module")
def big():
    """an ensemble of capacity 300 x 13 holding the BIG case, with kept weights, and the bytes it then has; the tests below only read it"""
    c = get_output_case(*BIG)
    ens = ParticleEnsemble(None, 300, c.N)
    ens.set(c.ids, c.sensor, c.p)
    ens.likelihood(device_camera(c.cam), c.mids, c.y, c.var)
    return c, ens, ens_bytes(ens)


# ---- the generator read back ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 4, 5, 257])
def test_uniforms_are_the_restatement_byte_for_byte(big, count):
    c, ens, before = big
    u = ens.uniforms(SEED, STREAM, count)
    assert u.shape == (count,)
    assert u.tobytes() == cached_uniforms(SEED, STREAM, count).tobytes()
    assert ens.uniforms(SEED, STREAM, count).tobytes() == u.tobytes()
    assert np.all(u > 0.0) and np.all(u < 1.0)
    assert ens_bytes(ens) == before


ROWS = (1, 3, 4, 5, 21, 24, 33)
PS = (1, 2, 31, 32, 33, 257)
NORMAL_SHAPES = [(rows, PS[i % len(PS)]) for i, rows in enumerate(ROWS)] + [(33, 257), (40, 300)]  # ... the subset test's request, and the capacity of `big`


@pytest.mark.parametrize("rows,P", NORMAL_SHAPES, ids=[f"{r}x{p}" for r, p in NORMAL_SHAPES])
def test_normals_match_the_restatement(big, rows, P):
    c, ens, before = big
    z = ens.normals(SEED, STREAM, rows, P)
    assert z.shape == (rows, P)
    err = float(np.max(np.abs(z - cached_normals(SEED, STREAM, rows, P))))
    print(f"[ensemble normals] {rows} x {P}: max |device - restatement| {err:.2e} (bound 1e-13), largest |z| {float(np.max(np.abs(z))):.2f}")
    assert err <= 1e-13
    assert ens.normals(SEED, STREAM, rows, P).tobytes() == z.tobytes(), "differs run to run"
    assert ens_bytes(ens) == before


def test_normals_subset_rule_and_keys(big):
    c, ens, before = big
    full = ens.normals(SEED, STREAM, 33, 257)
    part = ens.normals(SEED, STREAM, 5, 33)
    assert np.ascontiguousarray(full[:5, :33]).tobytes() == np.ascontiguousarray(part).tobytes()
    small = ParticleEnsemble(None, 33, 0)  # another ensemble, another capacity: the same values
    assert small.normals(SEED, STREAM, 5, 33).tobytes() == part.tobytes()
    assert small.normals(SEED, STREAM, 22, 1).tobytes() == np.asfortranarray(full[:22, :1]).tobytes()
    other_seed, other_stream = ens.normals(SEED + 1, STREAM, 5, 33), ens.normals(SEED, STREAM + 1, 5, 33)
    assert not np.any(other_seed == part) and not np.any(other_stream == part) and not np.any(other_seed == other_stream)
    assert ens.normals(SEED + 2**64, STREAM - 2**64, 5, 33).tobytes() == part.tobytes()  # modulo 2^64
    u = ens.uniforms(SEED, STREAM, 33)
    assert not np.any(ens.uniforms(SEED + 1, STREAM, 33) == u) and not np.any(ens.uniforms(SEED, STREAM + 1, 33) == u)
    assert ens_bytes(ens) == before


def test_generator_calls_keep_the_kept_weights(big):
    c, _, _ = big
    dcam = device_camera(c.cam)
    out = []
    for draw in (False, True):
        ens = ParticleEnsemble(None, c.P, c.N)
        ens.set(c.ids, c.sensor, c.p)
        ens.likelihood(dcam, c.mids, c.y, c.var)
        if draw:
            ens.uniforms(7, 7, c.P)
            ens.normals(7, 7, 40, c.P)
        out.append((ens.resample_weighted(c.u).tobytes(), ens_bytes(ens)))
    assert out[0] == out[1]


def test_generator_launches():
    ens = ParticleEnsemble(None, 257, 4)
    seen = []
    for rows, P in ((1, 1), (33, 257)):
        ens.stats(reset=True)
        ens.normals(SEED, STREAM, rows, P)
        a = ens.stats(reset=True)
        ens.uniforms(SEED, STREAM, P)
        seen.append((a, ens.stats(reset=True)))
    assert seen[0] == seen[1] == ((1, 0), (1, 0))


# ---- sample_seeded == sample(normals) ----------------------------------------------------------------------------------------------------------------
P_LISTED = {(c[0], c[1]): c[2] for c in size_cases() if c[1] in (0, 1)}  # the P whose filter ensemble_cases.py lists at N = 0 and N = 1
SAMPLE_CASES = [(chart, N, (1, 33, 257)[(i + chart) % 3]) for chart in range(3) for i, N in enumerate((0, 1, 4))]


@pytest.mark.parametrize("chart,N,P", SAMPLE_CASES, ids=[case_key(*s) for s in SAMPLE_CASES])
def test_sample_seeded_is_sample_of_the_normals(chart, N, P):
    key = (chart, N, P if N == 4 else P_LISTED[(chart, N)])  # the filter: a listed case (n = 21, 24, 33), whose identity baseline is on file
    c = get_case(*key)
    core = make_core(c)
    seeded, twin = ParticleEnsemble(core, 257, N), ParticleEnsemble(core, 257, N)
    ctx0 = ctx_bytes(core)
    cnt0 = counters(core)
    seeded.sample_seeded(P, SEED, STREAM)
    assert counters(core) == cnt0 and ctx_bytes(core) == ctx0
    z = twin.normals(SEED, STREAM, c.n, P)
    twin.sample(z)
    assert seeded.size == (P, N)
    assert ens_bytes(seeded) == ens_bytes(twin)
    vals, _ = seeded.nees()
    ident = np.einsum("ik,ik->k", z, z) / c.n
    dev = float(np.max(np.abs(vals - ident) / ident))
    bound = max(10.0 * load_baseline()[case_key(*key)], 1e-12)
    print(f"[ensemble sample_seeded] {case_key(chart, N, P)} on the filter of {case_key(*key)}: identity {dev:.2e} (bound {bound:.2e})")
    assert dev <= bound


def test_sample_seeded_launches_do_not_depend_on_P():
    c = get_case(1, 4, 257)
    core = make_core(c)
    seen = {}
    for P in (2, 257):
        ens = ParticleEnsemble(core, 257, 4)
        ens.stats(reset=True)
        ens.sample(np.asfortranarray(cached_normals(SEED, STREAM, c.n, P)))
        plain = ens.stats(reset=True)
        ens.sample_seeded(P, SEED, STREAM)
        seen[P] = (plain, ens.stats(reset=True))
    print(f"[ensemble sample_seeded] (launches, factorisations) of sample, sample_seeded: {seen}")
    assert seen[2] == seen[257]
    plain, seeded = seen[2]
    assert seeded == (plain[0] + 1, 1) and plain[1] == 1


# ---- resample_weighted_seeded == resample_weighted(uniforms) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True], ids=["kept", "given"])
@pytest.mark.parametrize("P,P_new", [(257, 257), (1, 33), (257, 1), (257, 300)])
def test_resample_weighted_seeded_is_resample_weighted_of_the_uniforms(P, P_new, given):
    c = get_output_case(*BIG)
    dcam = device_camera(c.cam)
    w = np.random.default_rng(21).uniform(0.0, 2.0, P) if given else None
    out = []
    for seeded in (True, False):
        ens = ParticleEnsemble(None, 300, c.N)
        ens.set(c.ids, c.sensor[:P], c.p[:P])
        if not given:
            ens.likelihood(dcam, c.mids, c.y, c.var)
        ens.stats(reset=True)
        if seeded:
            src = ens.resample_weighted_seeded(P_new, SEED, 5, w)
            launches = ens.stats(reset=True)
        else:
            u = ens.uniforms(SEED, 5, P_new)
            ens.stats(reset=True)
            src = ens.resample_weighted(u, w)
            launches = ens.stats(reset=True)
        assert ens.size == (P_new, c.N)
        out.append((src.tobytes(), ens_bytes(ens), launches))
        assert np.all((src >= 0) & (src < P))
    assert out[0][:2] == out[1][:2]
    assert out[0][2] == (out[1][2][0] + 1, 0)
    # the kept weights are gone afterwards, as after resample_weighted
    assert code_of(lambda: ens.resample_weighted_seeded(P_new, SEED, 5)) == -3


def test_resample_weighted_seeded_without_weights_is_refused():
    c = get_output_case(*BIG)
    ens = ParticleEnsemble(None, 300, c.N)
    ens.set(c.ids, c.sensor, c.p)
    before = ens_bytes(ens)
    assert code_of(lambda: ens.resample_weighted_seeded(257, SEED, STREAM)) == -3
    assert ens_bytes(ens) == before


# ---- integrate_seeded == integrate(sigma6 * normals) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", [(0, 1), (0, 33), (4, 1), (4, 33)])
def test_integrate_seeded_is_integrate_of_the_scaled_normals(N, P):
    c = get_case(1, 4, 33)
    sigma6 = np.array([0.01, 0.02, 0.03, 0.1, 0.2, 0.3])
    ids = c.ids[:N]
    sens = np.random.default_rng(31).normal(size=(P, 23))
    for lo in (6, 16):  # unit quaternions of the pose and the camera offset
        sens[:, lo:lo + 4] /= np.linalg.norm(sens[:, lo:lo + 4], axis=1, keepdims=True)
    pts = np.random.default_rng(32).normal(size=(P, N, 3)) + np.array([0.0, 0.0, 8.0])
    out = {}
    for route in ("seeded", "twin", "zero", "plain"):
        ens = ParticleEnsemble(None, 33, 4)
        ens.set(ids, sens, pts)
        ens.stats(reset=True)
        if route == "seeded":
            ens.integrate_seeded(c.imu, c.dt, sigma6, SEED, 9)
        elif route == "twin":
            z = ens.normals(SEED, 9, 6, P)
            ens.stats(reset=True)
            ens.integrate(c.imu, c.dt, (sigma6[:, None] * z).T)
        elif route == "zero":
            ens.integrate_seeded(c.imu, c.dt, np.zeros(6), SEED, 9)
        else:
            ens.integrate(c.imu, c.dt)
        out[route] = (ens_bytes(ens), ens.stats()[0])
    assert out["seeded"][0] == out["twin"][0]
    assert out["zero"][0] == out["plain"][0]
    assert out["seeded"][0] != out["plain"][0]
    assert out["seeded"][1] == out["twin"][1] + 1 and out["zero"][1] == out["plain"][1] + 1


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched():
    c = get_case(1, 4, 33)
    core = make_core(c)
    ens = ParticleEnsemble(core, 40, 6)  # padded state capacity 21 + 18 = 39 -> 40
    ens.set(*c.truth_x)
    oc = get_output_case(0, 2, 31)
    out_ens = ParticleEnsemble(None, 40, oc.N)
    out_ens.set(oc.ids, oc.sensor, oc.p)
    out_ens.likelihood(device_camera(0), oc.mids, oc.y, oc.var)
    before, out_before, ctx0 = ens_bytes(ens), ens_bytes(out_ens), ctx_bytes(core)
    sigma6 = np.full(6, 0.1)
    d = (C.c_double * 64)()
    refusals = [
        (lambda: ens.normals(SEED, STREAM, 0, 4), -3), (lambda: ens.normals(SEED, STREAM, 41, 4), -4), (lambda: ens.normals(SEED, STREAM, 4, 0), -3),
        (lambda: ens.normals(SEED, STREAM, 4, 41), -4), (lambda: ens.normals(SEED, STREAM, -1, 4), -3),
        (lambda: ens.uniforms(SEED, STREAM, 0), -3), (lambda: ens.uniforms(SEED, STREAM, 41), -4),
        (lambda: ens.sample_seeded(0, SEED, STREAM), -3), (lambda: ens.sample_seeded(41, SEED, STREAM), -4),
        (lambda: ParticleEnsemble(core, 40, 3).sample_seeded(4, SEED, STREAM), -4),  # the filter holds more landmarks than the ensemble has room for
        (lambda: out_ens.resample_weighted_seeded(0, SEED, STREAM), -3), (lambda: out_ens.resample_weighted_seeded(41, SEED, STREAM), -4),
        (lambda: out_ens.resample_weighted_seeded(31, SEED, STREAM, np.zeros(31)), -3), (lambda: out_ens.resample_weighted_seeded(31, SEED, STREAM, np.r_[np.ones(30), np.nan]), -3),
        (lambda: ens.integrate_seeded(c.imu, c.dt, None, SEED, STREAM), -3),
    ]
    for call, code in refusals:
        assert code_of(call) == code
        assert ens_bytes(ens) == before and ens_bytes(out_ens) == out_before
    assert ens.lib.eqf_ensemble_normals(ens.h, SEED, STREAM, 4, 4, None) == -3
    assert ens.lib.eqf_ensemble_uniforms(ens.h, SEED, STREAM, 4, None) == -3
    assert ens.lib.eqf_ensemble_integrate_seeded(ens.h, None, 0.01, d, SEED, STREAM) == -3
    assert ens.normals(SEED, STREAM, 40, 40).shape == (40, 40)  # the capacities themselves are served
    assert ens.uniforms(SEED, STREAM, 40).shape == (40,)
    assert ens_bytes(ens) == before and ens_bytes(out_ens) == out_before and ctx_bytes(core) == ctx0
    # the kept weights survived every refusal
    twin = ParticleEnsemble(None, 40, oc.N)
    twin.set(oc.ids, oc.sensor, oc.p)
    twin.likelihood(device_camera(0), oc.mids, oc.y, oc.var)
    assert np.array_equal(out_ens.resample_weighted_seeded(31, SEED, STREAM), twin.resample_weighted(twin.uniforms(SEED, STREAM, 31)))
    empty = ParticleEnsemble(None, 4, 2)
    assert code_of(lambda: empty.resample_weighted_seeded(1, SEED, STREAM, np.ones(0))) == -3
    # what sample refuses: the float Sigma store, a pivot <= 0
    core32 = make_core(c)
    core32.set_option(OPT_SIGMA_FP32, 2)
    e32 = ParticleEnsemble(core32, 40, 6)
    e32.set(*c.truth_x)
    b32 = ens_bytes(e32)
    assert code_of(lambda: e32.sample_seeded(4, SEED, STREAM)) == -6 and ens_bytes(e32) == b32
    S = c.Sigma.copy()
    S[32, 32] = -S[32, 32]
    core.set_sigma(S)
    assert code_of(lambda: ens.sample_seeded(4, SEED, STREAM)) == -2 and ens_bytes(ens) == before


# ---- the reference's initial-distribution check, drawn on the device -----------------------------------------------------------------------------------------
def test_reference_initial_distribution_N2_P1000_from_a_seed():
    f = StatFixture(2, 1000, STAT_SEEDS[(2, "initial")])
    core = EqfCore(2, COORD_INVDEPTH)
    core.set_state(f.xi0f, f.Xsf, f.ids, f.q0, f.Q)
    core.set_sigma(f.sigma0)
    ens = ParticleEnsemble(core, 1000, 2)
    ens.sample_seeded(1000, SEED, STREAM)
    _, mean = ens.nees()
    print(f"[ensemble statistics] N=2 P=1000 initial, particles of seed {SEED} stream {STREAM}: mean NEES {mean:.6f} (band {STAT_BANDS['initial']})")
    assert abs(mean - 1.0) <= STAT_BANDS["initial"]
