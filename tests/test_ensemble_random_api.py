"""include/eqf_ensemble_random.h on a box without a GPU: the library exports its five calls, the binding declares exactly those in a third list of its own
(and the lists of include/eqf_ensemble.h and include/eqf_ensemble_output.h are what they were), the header states its contract, and refusals that need no
device return their codes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "eqf_ensemble_random.h")
CALLS = ["normals", "uniforms", "sample_seeded", "resample_weighted_seeded", "integrate_seeded"]
THREE = ["measure", "likelihood", "resample_weighted"]
TWELVE = ["create", "destroy", "size", "set", "get", "sample", "integrate", "errors", "nees", "covariance", "resample", "stats"]


def declared_symbols(path=HEADER):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eqf_ensemble_[A-Za-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.ensemble import load_ensemble_protos

    return load_ensemble_protos()


def test_header_declares_the_five_calls():
    assert declared_symbols() == sorted("eqf_ensemble_" + c for c in CALLS)


def test_library_exports_and_binding_declares_them_in_a_third_list(lib):
    raw = ctypes.CDLL(os.path.join(ROOT, "eqvio_amd", "lib", "libeqf_hip.so"))
    for n in declared_symbols():
        assert hasattr(raw, n), f"{n} declared in include/eqf_ensemble_random.h but not exported"
    assert sorted(lib._ensemble_random_declared) == declared_symbols()
    assert sorted(lib._ensemble_output_declared) == sorted("eqf_ensemble_" + c for c in THREE)
    assert sorted(lib._ensemble_declared) == sorted("eqf_ensemble_" + c for c in TWELVE)
    assert declared_symbols(os.path.join(ROOT, "include", "eqf_ensemble.h")) == sorted("eqf_ensemble_" + c for c in TWELVE)
    assert declared_symbols(os.path.join(ROOT, "include", "eqf_ensemble_output.h")) == sorted("eqf_ensemble_" + c for c in THREE)
    from eqvio_amd.capi import load_eqf_lib

    assert not [n for n in load_eqf_lib()._declared if n.startswith("eqf_ensemble_")]


def test_binding_has_the_five_methods(lib):
    from eqvio_amd.ensemble import ParticleEnsemble

    for name in CALLS:
        assert callable(getattr(ParticleEnsemble, name))


def test_seeds_and_streams_are_taken_modulo_2_64():
    from eqvio_amd.ensemble import _u64

    assert _u64(-1) == 2**64 - 1 and _u64(2**64 + 5) == 5 and _u64(2026) == 2026


def test_header_states_the_contract():
    txt = " ".join(open(HEADER).read().split())
    for phrase in ("Philox4x64-10", "0xD2E7470EE14C6C93", "0xCA5A826395121157", "0x9E3779B97F4A7C15", "0xBB67AE8584CAA73B", "ten rounds", "KEY = (seed, stream)",
                   "counter (j, k, 0, 0)", "counter (i >> 2, 0, 0, 1)", "U(x) = (2 (x >> 12) + 1) 2^-53", "strictly inside (0, 1)", "BOX-MULLER",
                   "r = sqrt(-2 log U(x0))", "cospi(2 U(x1))", "sinpi(2 U(x1))", "depends on seed, stream, row and particle alone", "THE THREE EQUALITIES",
                   "byte for byte", "sigma6[c] *", "CHECKED BEFORE ANY DEVICE WORK", "untouched bit for bit", "EQF_E_BAD_ARG", "EQF_E_CAPACITY", "NO n x P COPY",
                   "none depending on P", "eqf_ensemble_stats counts these launches", "No kernel uses LDS or talks to another workgroup", "DISTINCT STREAMS FOR DISTINCT DRAWS",
                   "caller's business", "np.random.Philox"):
        assert phrase in txt, phrase
    pointer = " ".join(open(os.path.join(ROOT, "include", "eqf_ensemble.h")).read().split())
    assert "eqf_ensemble_random.h" in pointer


def test_null_arguments_are_refused_before_the_device(lib):
    d = (ctypes.c_double * 16)()
    i1 = (ctypes.c_int * 2)()
    assert lib.eqf_ensemble_normals(None, 1, 0, 4, 1, d) == -3
    assert lib.eqf_ensemble_uniforms(None, 1, 0, 4, d) == -3
    assert lib.eqf_ensemble_sample_seeded(None, None, 1, 1, 0) == -3
    assert lib.eqf_ensemble_resample_weighted_seeded(None, 1, None, 1, 0, i1) == -3
    assert lib.eqf_ensemble_integrate_seeded(None, d, 0.01, d, 1, 0) == -3
