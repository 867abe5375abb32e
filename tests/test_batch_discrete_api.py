"""The discrete-state-matrix mode of the filter batch on a CPU-only box: the entry points and the enum are declared in both headers, exported and in the
Python lists; their refusals come before any device is looked at and leave the outputs alone; the pins of the accurate mode stay; the tools' --batchRiccati
flag takes its third word and is checked before a file or device is opened."""
import ctypes as C
import os
import re
import subprocess

import pytest

from eqvio_amd.capi import COORD_INVDEPTH, Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
OPT = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")
EQF_E_BAD_ARG, EQF_E_UNSUPPORTED = -3, -6


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch import load_batch_protos

    return load_batch_protos()


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_declared_in_headers_and_python(libs):
    elib, flib = libs
    dev, flt = header("eqf_batch.h"), header("eqvio_batch.h")
    assert re.search(r"int\s+eqf_batch_step_discrete\s*\(\s*eqf_batch\s*\*\s*b\s*,\s*int\s+count\s*,\s*const\s+eqf_batch_frame\s*\*\s*frames\s*,\s*int\s*\*\s*status\s*\)", dev)
    assert re.search(r"enum\s*\{\s*EQVIO_BATCH_STATE_MATRIX_CONTINUOUS\s*=\s*0\s*,\s*EQVIO_BATCH_STATE_MATRIX_DISCRETE\s*=\s*1\s*\}", flt)
    assert re.search(r"int\s+eqvio_batch_set_slot_state_matrix\s*\(\s*eqvio_batch\s*\*\s*b\s*,\s*int\s+slot\s*,\s*int\s+kind\s*\)", flt)
    assert re.search(r"int\s+eqvio_batch_get_slot_state_matrix\s*\(\s*const\s+eqvio_batch\s*\*\s*b\s*,\s*int\s+slot\s*\)", flt)
    # the Riccati enum keeps exactly its two members
    assert re.search(r"enum\s*\{\s*EQVIO_BATCH_RICCATI_FAST\s*=\s*0\s*,\s*EQVIO_BATCH_RICCATI_ACCURATE\s*=\s*1\s*\}", flt)
    assert "eqf_batch_step_discrete" in elib._batch_declared and hasattr(elib, "eqf_batch_step_discrete")
    for n in ("eqvio_batch_set_slot_state_matrix", "eqvio_batch_get_slot_state_matrix"):
        assert hasattr(flib, n) and n in flib._batch_declared, n
    import eqvio_amd.batch as B

    assert (B.STATE_MATRIX_CONTINUOUS, B.STATE_MATRIX_DISCRETE) == (0, 1) and (B.RICCATI_FAST, B.RICCATI_ACCURATE) == (0, 1)
    assert callable(B.BatchCore.step_discrete)
    assert callable(B.VIOFilterBatch.set_slot_state_matrix) and callable(B.VIOFilterBatch.slot_state_matrix)
    assert isinstance(B.BatchSlot.state_matrix, property)
    # both headers say that the mode is a call and a per-slot choice, not a setting
    for name in ("eqf_batch.h", "eqvio_batch.h"):
        text = " ".join(open(os.path.join(ROOT, "include", name)).read().split())
        assert re.search(r"useDiscreteStateMatrix field of eqvio_settings is not read", text), name


def test_null_and_negative_arguments_refused_without_a_device(libs):
    elib, flib = libs
    st = C.c_int(7)
    assert elib.eqf_batch_step_discrete(None, 1, None, C.byref(st)) == EQF_E_BAD_ARG
    assert elib.eqf_batch_step_discrete(None, 0, None, None) == EQF_E_BAD_ARG
    assert elib.eqf_batch_step_discrete(None, -1, None, None) == EQF_E_BAD_ARG
    assert st.value == 7
    for kind in (0, 1, 2, -1):
        assert flib.eqvio_batch_set_slot_state_matrix(None, 0, kind) == EQF_E_BAD_ARG
        assert flib.eqvio_batch_set_slot_state_matrix(None, -1, kind) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_get_slot_state_matrix(None, 0) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_get_slot_state_matrix(None, -1) == EQF_E_BAD_ARG
    # the pins of the accurate mode: a third Riccati mode is still refused, and so are settings with fastRiccati = 0, whatever useDiscreteStateMatrix says
    assert flib.eqvio_batch_set_slot_riccati(None, 0, 2) == EQF_E_BAD_ARG
    for disc in (0, 1):
        s = Settings.defaults()
        s.coordinateChoice = COORD_INVDEPTH
        s.fastRiccati, s.useDiscreteStateMatrix = 0, disc
        assert elib.eqf_batch_check_settings(C.byref(s)) == EQF_E_UNSUPPORTED
        s.fastRiccati = 1  # ... and the field is not read: accepted either way
        assert elib.eqf_batch_check_settings(C.byref(s)) == 0


def have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except ImportError:
        return False


def test_kind_and_mode_checked_on_a_batch(libs):
    """a bad kind and the third Riccati mode on a batch that exists: needs a device to create one, so without one the creation's refusal is what is checked"""
    elib, flib = libs
    s = Settings.defaults()
    s.coordinateChoice, s.fastRiccati = COORD_INVDEPTH, 1
    h = C.c_void_p()
    gpu = have_gpu()  # asked before the library opens the device: the order smoke() uses
    rc = flib.eqvio_batch_create(C.byref(h), C.byref(s), 0, 3, 8)
    if rc == -5:  # EQF_E_NO_DEVICE, behind the argument checks
        assert not h and not gpu
        return
    assert rc == 0
    try:
        assert [flib.eqvio_batch_get_slot_state_matrix(h, k) for k in range(3)] == [0, 0, 0]
        for kind in (2, -1):
            assert flib.eqvio_batch_set_slot_state_matrix(h, 1, kind) == EQF_E_BAD_ARG
        assert flib.eqvio_batch_set_slot_state_matrix(h, 3, 1) == EQF_E_BAD_ARG and flib.eqvio_batch_get_slot_state_matrix(h, 3) == EQF_E_BAD_ARG
        assert flib.eqvio_batch_set_slot_riccati(h, 1, 2) == EQF_E_BAD_ARG
        assert [flib.eqvio_batch_get_slot_state_matrix(h, k) for k in range(3)] == [0, 0, 0]
        assert flib.eqvio_batch_set_slot_state_matrix(h, 1, 1) == 0 and [flib.eqvio_batch_get_slot_state_matrix(h, k) for k in range(3)] == [0, 1, 0]
        assert [flib.eqvio_batch_get_slot_riccati(h, k) for k in range(3)] == [0, 0, 0]  # the two choices are kept apart
        assert flib.eqvio_batch_set_slot_state_matrix(h, -1, 1) == 0 and [flib.eqvio_batch_get_slot_state_matrix(h, k) for k in range(3)] == [1, 1, 1]
    finally:
        flib.eqvio_batch_destroy(h)


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("exe,name", [(SIM, "eqvio_sim"), (OPT, "eqvio_opt")])
def test_tools_still_refuse_unknown_words(libs, tmp_path, exe, name):
    files = [] if exe == SIM else ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv")]
    rec = ["--record", str(tmp_path / "rec")]
    for args in (["--batch", "4", "--batchRiccati", "quick"], ["--batch", "4", "--batchRiccati", "fast,discrete,exact,fast"], ["--batch", "4", "--batchRiccati", "Discrete"],
                 ["--batch", "4", "--batchRiccati", "fast,discrete"], ["--batch", "4", "--batchRiccati", "discrete,"], ["--batchRiccati", "discrete"]):
        out = run(exe, *files, *(rec if "--batch" in args else []), *args)
        assert out.returncode == 2, (args, out.returncode, out.stdout, out.stderr)
        assert "--batchRiccati" in out.stderr and out.stderr.startswith(name + ": "), (args, out.stderr)
        assert not (tmp_path / "rec").exists()


@pytest.mark.parametrize("exe", [SIM, OPT])
def test_help_names_the_word(libs, exe):
    out = run(exe, "--help")
    assert out.returncode == 0 and "--batchRiccati" in out.stdout and "fast|accurate|discrete" in out.stdout and "useDiscreteStateMatrix" in out.stdout


def test_discrete_gets_past_the_argument_checks(libs, tmp_path):
    """past the argument checks the run needs a device: without one eqvio_sim ends with status 1 at eqvio_batch_create, with one it runs"""
    for modes in ("discrete", "fast,discrete"):
        out = run(SIM, "--batch", "2", "--batchRiccati", modes, "--duration", "0.2", "--maxFeatures", "10", "--quiet")
        if out.returncode == 0:
            assert "riccati discrete" in out.stdout
        else:
            assert out.returncode == 1 and "eqvio_batch_create" in out.stderr and not have_gpu(), (out.returncode, out.stderr)
        # eqvio_opt: past the flag's checks the next refusal is the missing dataset, not the flag
        out = run(OPT, "--batch", "2", "--batchRiccati", modes, "--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"))
        assert out.returncode != 2 and "--batchRiccati" not in out.stderr, (out.returncode, out.stderr)
