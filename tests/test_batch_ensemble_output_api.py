"""include/eqf_batch_ensemble_output.h on a box without a GPU: the header declares exactly its three calls with the eqf_bens_ prefix, the library exports them,
the binding declares exactly those in a list of its own (_batch_ensemble_output_declared) while _batch_ensemble_declared is still the ten of
include/eqf_batch_ensemble.h, the header states its contract, and null and out-of-range arguments are refused with their codes before any device is looked
at. No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "eqf_batch_ensemble_output.h")
OLD_HEADER = os.path.join(INCLUDE, "eqf_batch_ensemble.h")
THREE = ["likelihood", "resample_weighted_seeded", "covariance"]
TEN = ["create", "destroy", "size", "stats", "set", "get", "sample_seeded", "integrate", "errors", "nees"]


def declared_symbols(path, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[A-Za-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch_ensemble import load_batch_ensemble_protos

    return load_batch_ensemble_protos()


def test_header_declares_exactly_the_three_calls():
    assert declared_symbols(HEADER, "eqf_bens_") == sorted("eqf_bens_" + c for c in THREE)
    assert not declared_symbols(HEADER, "eqf_batch_") and not declared_symbols(HEADER, "eqf_ensemble_")
    # the first header keeps its ten, and the two are the only headers that name eqf_bens
    assert declared_symbols(OLD_HEADER, "eqf_bens_") == sorted("eqf_bens_" + c for c in TEN)
    named = sorted(n for n in os.listdir(INCLUDE) if "eqf_bens" in open(os.path.join(INCLUDE, n)).read())
    assert named == ["eqf_batch_ensemble.h", "eqf_batch_ensemble_output.h"]


def test_library_exports_every_declared_symbol(lib):
    raw = ctypes.CDLL(os.path.join(ROOT, "eqvio_amd", "lib", "libeqf_hip.so"))
    for n in declared_symbols(HEADER, "eqf_bens_"):
        assert hasattr(raw, n), f"{n} declared in include/eqf_batch_ensemble_output.h but not exported"


def test_binding_declares_exactly_the_header_in_a_list_of_its_own(lib):
    assert sorted(lib._batch_ensemble_output_declared) == declared_symbols(HEADER, "eqf_bens_")
    assert sorted(lib._batch_ensemble_declared) == sorted("eqf_bens_" + c for c in TEN)
    assert not set(lib._batch_ensemble_output_declared) & set(lib._batch_ensemble_declared)


def test_binding_has_the_methods(lib):
    from eqvio_amd.batch_ensemble import BatchEnsemble

    for name in ("likelihood", "resample_weighted_seeded", "covariance"):
        assert callable(getattr(BatchEnsemble, name))


def test_entry_structs_have_the_headers_layout(lib):
    from eqvio_amd.batch_ensemble import BensLikelihoodEntry, BensResampleEntry

    txt = open(HEADER).read()
    for struct, cls in (("eqf_bens_likelihood_entry", BensLikelihoodEntry), ("eqf_bens_resample_entry", BensResampleEntry)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", txt, flags=re.S).group(1)
        names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], struct


def test_header_states_the_contract():
    txt = " ".join(open(HEADER).read().replace("\n *", " ").split())  # the comment's line prefixes taken out
    for phrase in ("NOTHING P-SIZED CROSSES THE BUS", "THE SAME ORDERS OF THE SUMS", "THE LOG DOMAIN", "BEFORE ANY DEVICE WORK", "untouched bit for bit",
                   "SLOT IS READ ONLY", "no kernel communicates between workgroups", "A PARTICLE'S VALUE DEPENDS ON ITS OWN DATA AND ITS ENTRY'S ALONE",
                   "LAUNCHES PER CALL", "likelihood 2", "resample_weighted_seeded 3", "covariance 2", "THE KEPT WEIGHTS", "INVALIDATE", "MEMORY PER SLOT",
                   "MATCHED BY ID", "EQF_E_NONFINITE", "KEEPS NOTHING", "EQF_E_BAD_ARG", "EQF_E_CAPACITY", "c_(P-1) = 1 exactly",
                   "((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))", "uniforms(seed, stream, P_new)", "word i & 3 of the block of counter (i >> 2, 0, 0, 1)",
                   "second place", "v_mfma_f64_16x16x4_f64", "C == C^T exactly", "No factorisation", "213 * 213", "Out of scope", "caller-supplied uniforms",
                   "landmark turnover"):
        assert phrase in txt, phrase
    old = " ".join(open(OLD_HEADER).read().replace("\n *", " ").split())
    assert "eqf_batch_ensemble_output.h" in old  # the first header points here


def test_null_and_out_of_range_arguments_are_refused_before_the_device(lib):
    from eqvio_amd.batch_ensemble import BensLikelihoodEntry, BensResampleEntry

    d = (ctypes.c_double * 64)()
    i4 = (ctypes.c_int * 4)()
    le, re_ = (BensLikelihoodEntry * 1)(), (BensResampleEntry * 1)()
    assert lib.eqf_bens_likelihood(None, 1, le, d, d, d, d, i4) == -3
    assert lib.eqf_bens_likelihood(None, 0, le, d, d, d, d, i4) == -3
    assert lib.eqf_bens_resample_weighted_seeded(None, 1, re_, i4, i4) == -3
    assert lib.eqf_bens_covariance(None, 1, i4, d, i4) == -3
    fake = ctypes.c_void_p(1)  # never dereferenced: the count and the null lists are refused first
    assert lib.eqf_bens_likelihood(fake, -1, le, d, d, d, d, i4) == -3
    assert lib.eqf_bens_likelihood(fake, 1, None, d, d, d, d, i4) == -3
    assert lib.eqf_bens_likelihood(fake, 1, le, d, d, d, d, None) == -3
    assert lib.eqf_bens_likelihood(fake, 0, None, None, None, None, None, None) == 0  # nothing listed: nothing to do
    assert lib.eqf_bens_resample_weighted_seeded(fake, -1, re_, i4, i4) == -3
    assert lib.eqf_bens_resample_weighted_seeded(fake, 1, None, i4, i4) == -3
    assert lib.eqf_bens_resample_weighted_seeded(fake, 1, re_, i4, None) == -3
    assert lib.eqf_bens_resample_weighted_seeded(fake, 0, None, None, None) == 0
    assert lib.eqf_bens_covariance(fake, -1, i4, d, i4) == -3
    assert lib.eqf_bens_covariance(fake, 1, None, d, i4) == -3
    assert lib.eqf_bens_covariance(fake, 1, i4, None, i4) == -3
    assert lib.eqf_bens_covariance(fake, 1, i4, d, None) == -3
    assert lib.eqf_bens_covariance(fake, 0, None, None, None) == 0
