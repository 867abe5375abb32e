"""include/eqf_ensemble.h on a box without a GPU: the library exports what the header declares, the binding declares exactly that, the header states the
refusal codes and the one-factorisation contract, and constructing an ensemble without a device is a loud error. No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "eqf_ensemble.h")
CALLS = ["create", "destroy", "size", "set", "get", "sample", "integrate", "errors", "nees", "covariance", "resample", "stats"]


def declared_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eqf_ensemble_[A-Za-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    return True


def test_header_declares_the_twelve_calls():
    assert declared_symbols() == sorted("eqf_ensemble_" + c for c in CALLS)


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "eqvio_amd", "lib", "libeqf_hip.so"))
    for n in declared_symbols():
        assert hasattr(lib, n), f"{n} declared in include/eqf_ensemble.h but not exported"


def test_binding_declares_exactly_the_header(built):
    from eqvio_amd.capi import load_eqf_lib
    from eqvio_amd.ensemble import load_ensemble_protos

    lib = load_ensemble_protos()
    assert sorted(lib._ensemble_declared) == declared_symbols()
    # the context header's list stays what tests/test_abi_symbols.py pins
    assert not [n for n in load_eqf_lib()._declared if n.startswith("eqf_ensemble_")]


def test_eqf_hip_header_is_not_extended():
    txt = open(os.path.join(ROOT, "include", "eqf_hip.h")).read()
    assert "eqf_ensemble" not in txt


def test_header_states_refusals_and_the_one_factorisation_contract():
    txt = " ".join(open(HEADER).read().split())
    for code in ("EQF_E_BAD_ARG", "EQF_E_CAPACITY", "EQF_E_UNSUPPORTED", "EQF_E_NOT_SPD", "EQF_E_NO_DEVICE"):
        assert code in txt, code
    assert "ONE FACTORISATION PER CALL" in txt
    assert "factorised ONCE per call" in txt
    assert "does not depend on P" in txt
    assert "NO partial-pivot fallback" in txt
    assert "EQF_OPT_SIGMA_FP32 = 2" in txt
    assert "untouched bit for bit" in txt


def test_no_device_is_a_loud_error(built):
    import torch

    from eqvio_amd.capi import EqfError
    from eqvio_amd.ensemble import ParticleEnsemble

    if torch.cuda.is_available():  # a box with a device: the same constructor succeeds
        ParticleEnsemble(None, 8, 2).close()
        return
    with pytest.raises(EqfError) as e:
        ParticleEnsemble(None, 8, 2)
    assert e.value.code == -5


def test_bad_creation_arguments_are_refused_before_the_device(built):
    from eqvio_amd.ensemble import load_ensemble_protos

    lib = load_ensemble_protos()
    h = ctypes.c_void_p()
    assert lib.eqf_ensemble_create(ctypes.byref(h), 0, 0, 2) == -3
    assert lib.eqf_ensemble_create(ctypes.byref(h), 0, 8, -1) == -3
    assert lib.eqf_ensemble_create(None, 0, 8, 2) == -3
    assert lib.eqf_ensemble_size(None, None, None) == -3
    assert lib.eqf_ensemble_stats(None, None, None, 0) == -3
