"""include/eqf_batch_ensemble.h on a box without a GPU: the header declares exactly its ten calls, the library exports them, the binding declares exactly
those in a list of its own (_batch_ensemble_declared) while the context's, the batch's and the three single-filter ensemble lists are what they were, the
header states its contract, null and out-of-range arguments are refused with their codes before any device is looked at, and constructing a BatchEnsemble
without a device is a loud EqfError. No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "eqf_batch_ensemble.h")
CALLS = ["create", "destroy", "size", "stats", "set", "get", "sample_seeded", "integrate", "errors", "nees"]
TWELVE = ["create", "destroy", "size", "set", "get", "sample", "integrate", "errors", "nees", "covariance", "resample", "stats"]
THREE = ["measure", "likelihood", "resample_weighted"]
FIVE = ["normals", "uniforms", "sample_seeded", "resample_weighted_seeded", "integrate_seeded"]


def declared_symbols(path, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[A-Za-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch_ensemble import load_batch_ensemble_protos

    return load_batch_ensemble_protos()


def test_header_declares_exactly_the_ten_calls():
    assert declared_symbols(HEADER, "eqf_bens_") == sorted("eqf_bens_" + c for c in CALLS)
    # nothing of it is named after the batch or the single-filter ensemble, and it declares nothing of theirs
    assert not declared_symbols(HEADER, "eqf_batch_") and not declared_symbols(HEADER, "eqf_ensemble_")


def test_the_other_headers_are_not_extended():
    for name in ("eqf_hip.h", "eqf_batch.h", "eqf_ensemble.h", "eqf_ensemble_output.h", "eqf_ensemble_random.h"):
        assert "eqf_bens" not in open(os.path.join(INCLUDE, name)).read(), name
    assert declared_symbols(os.path.join(INCLUDE, "eqf_ensemble.h"), "eqf_ensemble_") == sorted("eqf_ensemble_" + c for c in TWELVE)
    assert declared_symbols(os.path.join(INCLUDE, "eqf_ensemble_output.h"), "eqf_ensemble_") == sorted("eqf_ensemble_" + c for c in THREE)
    assert declared_symbols(os.path.join(INCLUDE, "eqf_ensemble_random.h"), "eqf_ensemble_") == sorted("eqf_ensemble_" + c for c in FIVE)


def test_library_exports_every_declared_symbol(lib):
    raw = ctypes.CDLL(os.path.join(ROOT, "eqvio_amd", "lib", "libeqf_hip.so"))
    for n in declared_symbols(HEADER, "eqf_bens_"):
        assert hasattr(raw, n), f"{n} declared in include/eqf_batch_ensemble.h but not exported"


def test_binding_declares_exactly_the_header_in_a_list_of_its_own(lib):
    from eqvio_amd.batch import load_batch_protos
    from eqvio_amd.capi import load_eqf_lib
    from eqvio_amd.ensemble import load_ensemble_protos

    assert sorted(lib._batch_ensemble_declared) == declared_symbols(HEADER, "eqf_bens_")
    # the other lists are what they were: none of them names a call of this header, each equals its own header
    assert not [n for n in load_eqf_lib()._declared if n.startswith("eqf_bens_") or n.startswith("eqf_ensemble_") or n.startswith("eqf_batch_")]
    elib, _ = load_batch_protos()
    assert sorted(elib._batch_declared) == declared_symbols(os.path.join(INCLUDE, "eqf_batch.h"), "eqf_batch_")
    ens = load_ensemble_protos()
    assert sorted(ens._ensemble_declared) == sorted("eqf_ensemble_" + c for c in TWELVE)
    assert sorted(ens._ensemble_output_declared) == sorted("eqf_ensemble_" + c for c in THREE)
    assert sorted(ens._ensemble_random_declared) == sorted("eqf_ensemble_" + c for c in FIVE)


def test_binding_has_the_methods(lib):
    from eqvio_amd.batch_ensemble import BatchEnsemble

    for name in ("size", "stats", "set", "get", "sample_seeded", "integrate", "errors", "nees", "close"):
        assert callable(getattr(BatchEnsemble, name))


def test_header_states_the_contract():
    txt = " ".join(open(HEADER).read().replace("\n *", " ").split())  # the comment's line prefixes taken out
    for phrase in ("ONE FACTORISATION OF SIGMA PER (ENTRY, CALL)", "depends neither on the number of entries nor on any P", "EVERYTHING OF A CLOUD IS ON THE DEVICE",
                   "MEMORY PER SLOT", "BEFORE ANY DEVICE WORK", "untouched bit for bit", "SLOT IS READ ONLY", "EQF_E_BAD_ARG", "EQF_E_CAPACITY", "EQF_E_NOT_SPD",
                   "EQF_E_NO_DEVICE", "NO partial-pivot fallback", "no kernel communicates between workgroups", "A PARTICLE'S VALUE DEPENDS ON ITS SLOT'S DATA AND ITS OWN DATA ALONE",
                   "BY ID", "index order", "normals(seed, stream, n, P)", "normals(seed, stream, 6, P)", "v_mfma_f64_16x16x4_f64", "cancellation-free logarithm", "Out of scope",
                   "weightedResample", "caller-supplied normals", "landmark turnover", "eqf_batch_create"):
        assert phrase in txt, phrase


def test_null_and_out_of_range_arguments_are_refused_before_the_device(lib):
    from eqvio_amd.batch_ensemble import BensIntegrateEntry, BensSampleEntry

    h = ctypes.c_void_p()
    d = (ctypes.c_double * 64)()
    i4 = (ctypes.c_int * 4)()
    fake = ctypes.c_void_p(1)  # never dereferenced: max_particles is refused first
    assert lib.eqf_bens_create(None, None, 8) == -3
    assert lib.eqf_bens_create(ctypes.byref(h), None, 8) == -3
    assert lib.eqf_bens_create(ctypes.byref(h), fake, 0) == -3
    assert not h.value
    assert lib.eqf_bens_size(None, 0, i4, i4) == -3
    assert lib.eqf_bens_stats(None, None, None, 0) == -3
    assert lib.eqf_bens_set(None, 0, 1, 0, i4, d, d) == -3
    assert lib.eqf_bens_get(None, 0, i4, d, d, 1, 1) == -3
    assert lib.eqf_bens_sample_seeded(None, 1, (BensSampleEntry * 1)(), i4) == -3
    assert lib.eqf_bens_integrate(None, 1, (BensIntegrateEntry * 1)(), i4) == -3
    assert lib.eqf_bens_errors(None, 0, d) == -3
    assert lib.eqf_bens_nees(None, 1, i4, d, d, i4) == -3
    lib.eqf_bens_destroy(None)  # a null ensemble is ignored


def test_no_device_is_a_loud_error(lib):
    import torch

    from eqvio_amd.batch import BatchCore, BatchError
    from eqvio_amd.batch_ensemble import BatchEnsemble
    from eqvio_amd.capi import EqfError, Settings

    with pytest.raises(EqfError) as e:  # no batch: refused on every box
        BatchEnsemble(None, 8)
    assert e.value.code == -3
    s = Settings.defaults()
    s.fastRiccati = 1
    if torch.cuda.is_available():  # a box with a device: the constructor succeeds on a batch
        core = BatchCore(s, 2)
        BatchEnsemble(core, 8).close()
        return
    with pytest.raises(BatchError) as b:  # without one there is no batch to hold against
        BatchCore(s, 2)
    assert b.value.code == -5
