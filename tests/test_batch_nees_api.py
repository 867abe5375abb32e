"""NEES and augmentLandmarkStates of the filter batch (include/eqf_batch.h, include/eqvio_batch.h) on a CPU-only box: the new entry points are exported and
declared, refuse bad arguments before any device is looked at, and `eqvio_sim --batch` refuses the settings the batch refuses (exit status 2)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG = -3
NEW_DEVICE = ["eqf_batch_nees", "eqf_batch_nees_lu_fallbacks", "eqf_batch_augment"]
NEW_FILTER = ["eqvio_batch_compute_nees", "eqvio_batch_augment_landmark_states", "eqvio_batch_run_sim"]


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch import load_batch_protos

    return load_batch_protos()


def test_new_symbols_exported_and_declared(libs):
    elib, flib = libs
    for n in NEW_DEVICE:
        assert hasattr(elib, n) and n in elib._batch_declared, n
    for n in NEW_FILTER:
        assert hasattr(flib, n) and n in flib._batch_declared, n
    assert not any(n in elib._declared for n in NEW_DEVICE)
    assert not any(n in flib._declared for n in NEW_FILTER)


def test_bad_arguments_refused_without_a_device(libs):
    elib, flib = libs
    from eqvio_amd.batch import BatchAugmentEntry, BatchTruth

    nees, st = (C.c_double * 2)(), (C.c_int * 2)()
    t = (BatchTruth * 2)()
    a = (BatchAugmentEntry * 2)()
    cnt = C.c_long()
    assert elib.eqf_batch_nees(None, 1, t, nees, st) == EQF_E_BAD_ARG
    assert elib.eqf_batch_nees(None, -1, None, None, None) == EQF_E_BAD_ARG
    assert elib.eqf_batch_nees_lu_fallbacks(None, 0, C.byref(cnt)) == EQF_E_BAD_ARG
    assert elib.eqf_batch_augment(None, 1, a, st) == EQF_E_BAD_ARG
    assert elib.eqf_batch_augment(None, -1, None, None) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_compute_nees(None, 1, None, None, None, None, None, None, None) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_augment_landmark_states(None, 1, None, None, None, None, None, None, None) == EQF_E_BAD_ARG
    done = C.c_int()
    assert flib.eqvio_batch_run_sim(None, None, 4, None, C.byref(done)) == EQF_E_BAD_ARG


@pytest.mark.parametrize("args", [["--fastRiccati", "1", "--maxFeatures", "80"], ["--fastRiccati", "1", "--fullState"], [],
                                  ["--fastRiccati", "1", "--landmarkReset", "1"], ["--fastRiccati", "1", "--output", "/nonexistent/x"]])
def test_eqvio_sim_batch_refusals(libs, args):
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    out = subprocess.run([exe, "--batch", "4", *args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, (out.returncode, out.stdout, out.stderr)
    assert "--batch" in out.stderr
