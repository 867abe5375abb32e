"""include/eqf_ensemble_output.h on a box without a GPU: the library exports its three calls, the binding declares exactly those in a list of its own
(and the list of include/eqf_ensemble.h is what it was), the header states its contract, and refusals that need no device return their codes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "eqf_ensemble_output.h")
CALLS = ["measure", "likelihood", "resample_weighted"]
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


def test_header_declares_the_three_calls():
    assert declared_symbols() == sorted("eqf_ensemble_" + c for c in CALLS)


def test_library_exports_and_binding_declares_them_in_a_list_of_their_own(lib):
    raw = ctypes.CDLL(os.path.join(ROOT, "eqvio_amd", "lib", "libeqf_hip.so"))
    for n in declared_symbols():
        assert hasattr(raw, n), f"{n} declared in include/eqf_ensemble_output.h but not exported"
    assert sorted(lib._ensemble_output_declared) == declared_symbols()
    assert sorted(lib._ensemble_declared) == sorted("eqf_ensemble_" + c for c in TWELVE)
    assert declared_symbols(os.path.join(ROOT, "include", "eqf_ensemble.h")) == sorted("eqf_ensemble_" + c for c in TWELVE)
    from eqvio_amd.capi import load_eqf_lib

    assert not [n for n in load_eqf_lib()._declared if n.startswith("eqf_ensemble_")]
    assert "eqf_ensemble" not in open(os.path.join(ROOT, "include", "eqf_hip.h")).read()


def test_binding_has_the_three_methods(lib):
    from eqvio_amd.ensemble import ParticleEnsemble

    for name in ("measure", "likelihood", "resample_weighted"):
        assert callable(getattr(ParticleEnsemble, name))


def test_header_states_the_contract():
    txt = " ".join(open(HEADER).read().split())
    for phrase in ("IN THE LOG DOMAIN", "MATCHED BY ID", "IN A FIXED ORDER", "depends on that particle's own points alone", "M = 0: loglik is 0",
                   "COUNTS AS -INFINITY", "EQF_E_NONFINITE", "KEEPS NOTHING", "IN ONE FIXED ORDER", "fixed by P alone", "THE KEPT WEIGHTS", "INVALIDATE",
                   "CHECKED BEFORE ANY DEVICE WORK", "untouched bit for bit", "EQF_E_BAD_ARG", "EQF_E_CAPACITY", "DEPENDS ON NEITHER P NOR M",
                   "eqf_ensemble_stats counts these launches", "No kernel talks to another workgroup", "NO CALL TAKES OR TOUCHES A CONTEXT", "a repeated id",
                   "or P - 1 if there is none"):
        assert phrase in txt, phrase
    pointer = " ".join(open(os.path.join(ROOT, "include", "eqf_ensemble.h")).read().split())
    assert "eqf_ensemble_output.h" in pointer


def test_null_arguments_are_refused_before_the_device(lib):
    from eqvio_amd.capi import Camera

    cam = Camera.pinhole(458.654, 457.296, 367.215, 248.375, 752, 480)
    d1, i1 = (ctypes.c_double * 4)(), (ctypes.c_int * 2)()
    assert lib.eqf_ensemble_measure(None, ctypes.addressof(cam), i1, 1, d1) == -3
    assert lib.eqf_ensemble_likelihood(None, ctypes.addressof(cam), i1, d1, 1, 4.0, None, None, None, None) == -3
    assert lib.eqf_ensemble_resample_weighted(None, 1, None, d1, i1) == -3
