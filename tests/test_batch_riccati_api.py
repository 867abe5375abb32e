"""The accurate Riccati mode of the filter batch on a CPU-only box: the entry points are declared in both headers and in the Python lists, their refusals
come before any device is looked at, and the tools' --batchRiccati flag is checked before a file or device is opened."""
import ctypes as C
import os
import re
import subprocess

import pytest

from eqvio_amd.capi import COORD_INVDEPTH, Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
OPT = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")
EQF_E_BAD_ARG, EQF_E_NO_DEVICE, EQF_E_UNSUPPORTED = -3, -5, -6


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
    assert re.search(r"int\s+eqf_batch_step_accurate\s*\(\s*eqf_batch\s*\*\s*b\s*,\s*int\s+count\s*,\s*const\s+eqf_batch_frame\s*\*\s*frames\s*,\s*int\s*\*\s*status\s*\)", dev)
    assert re.search(r"int\s+eqf_batch_last_riccati\s*\(\s*const\s+eqf_batch\s*\*\s*b\s*,\s*int\s+slot\s*,\s*int\s*\*\s*samples\s*,\s*int\s*\*\s*max_squarings\s*\)", dev)
    assert re.search(r"enum\s*\{\s*EQVIO_BATCH_RICCATI_FAST\s*=\s*0\s*,\s*EQVIO_BATCH_RICCATI_ACCURATE\s*=\s*1\s*\}", flt)
    assert re.search(r"int\s+eqvio_batch_set_slot_riccati\s*\(\s*eqvio_batch\s*\*\s*b\s*,\s*int\s+slot\s*,\s*int\s+mode\s*\)", flt)
    assert re.search(r"int\s+eqvio_batch_get_slot_riccati\s*\(\s*const\s+eqvio_batch\s*\*\s*b\s*,\s*int\s+slot\s*\)", flt)
    for n in ("eqf_batch_step_accurate", "eqf_batch_last_riccati"):
        assert hasattr(elib, n) and n in elib._batch_declared, n
    for n in ("eqvio_batch_set_slot_riccati", "eqvio_batch_get_slot_riccati"):
        assert hasattr(flib, n) and n in flib._batch_declared, n
    import eqvio_amd.batch as B

    assert (B.RICCATI_FAST, B.RICCATI_ACCURATE) == (0, 1)
    assert callable(B.BatchCore.step_accurate) and callable(B.BatchCore.last_riccati)
    assert callable(B.VIOFilterBatch.set_slot_riccati) and callable(B.VIOFilterBatch.slot_riccati)
    assert isinstance(B.BatchSlot.riccati, property)


def test_null_and_negative_arguments_refused_without_a_device(libs):
    elib, flib = libs
    n, sq, st = C.c_int(7), C.c_int(7), C.c_int(7)
    assert elib.eqf_batch_step_accurate(None, 1, None, C.byref(st)) == EQF_E_BAD_ARG
    assert elib.eqf_batch_step_accurate(None, 0, None, None) == EQF_E_BAD_ARG
    assert elib.eqf_batch_step_accurate(None, -1, None, None) == EQF_E_BAD_ARG
    assert elib.eqf_batch_last_riccati(None, 0, C.byref(n), C.byref(sq)) == EQF_E_BAD_ARG
    assert elib.eqf_batch_last_riccati(None, -1, None, None) == EQF_E_BAD_ARG
    assert (n.value, sq.value, st.value) == (7, 7, 7)
    assert flib.eqvio_batch_set_slot_riccati(None, 0, 1) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_set_slot_riccati(None, -1, 0) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_get_slot_riccati(None, 0) == EQF_E_BAD_ARG
    # the settings' refusal of fastRiccati = 0 stays what it was: the mode does not arrive through eqvio_settings
    s = Settings.defaults()
    s.coordinateChoice = COORD_INVDEPTH
    s.fastRiccati = 0
    assert elib.eqf_batch_check_settings(C.byref(s)) == EQF_E_UNSUPPORTED


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("exe,name", [(SIM, "eqvio_sim"), (OPT, "eqvio_opt")])
def test_tools_refuse_misuse_before_anything_is_opened(libs, tmp_path, exe, name):
    files = [] if exe == SIM else ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv")]
    rec = ["--record", str(tmp_path / "rec")]
    for args in (["--batch", "4", "--batchRiccati", "quick"], ["--batch", "4", "--batchRiccati", "fast,exact,fast,fast"],  # an unknown word
                 ["--batch", "4", "--batchRiccati", "fast,accurate"], ["--batch", "4", "--batchRiccati", "fast,fast,fast,fast,fast"],  # neither 1 nor B values
                 ["--batch", "4", "--batchRiccati", ""], ["--batchRiccati", "accurate"], ["--batchRiccati", "fast", "--fastRiccati", "1"]):  # without --batch
        out = run(exe, *files, *(rec if "--batch" in args else []), *args)  # (--record has a refusal of its own without --batch)
        assert out.returncode == 2, (args, out.returncode, out.stdout, out.stderr)
        assert "--batchRiccati" in out.stderr and out.stderr.startswith(name + ": "), (args, out.stderr)
        assert not (tmp_path / "rec").exists()


@pytest.mark.parametrize("exe", [SIM, OPT])
def test_help_names_the_flag(libs, exe):
    out = run(exe, "--help")
    assert out.returncode == 0 and "--batchRiccati" in out.stdout and "accurate" in out.stdout


def have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except ImportError:
        return False


def test_valid_flag_gets_past_the_argument_checks(libs, tmp_path):
    """eqvio_sim --batch B --batchRiccati ... is valid WITHOUT --fastRiccati 1: the tool hands the batch that setting itself. Past the argument checks the run
    needs a device: without one it ends with status 1 at eqvio_batch_create, with one it runs."""
    for modes in ("accurate", "fast,accurate"):
        out = run(SIM, "--batch", "2", "--batchRiccati", modes, "--duration", "0.2", "--maxFeatures", "10", "--quiet")
        if have_gpu():
            assert out.returncode == 0, out.stderr
            assert "riccati accurate" in out.stdout
        else:
            assert out.returncode == 1 and "eqvio_batch_create" in out.stderr, (out.returncode, out.stderr)
    # without the flag, today's refusal and message
    out = run(SIM, "--batch", "2", "--duration", "0.2")
    assert out.returncode == 2 and "--batch needs --fastRiccati 1" in out.stderr and "--batchRiccati" not in out.stderr
    # eqvio_opt: past the flag's checks the next refusal is the missing dataset, not the flag
    out = run(OPT, "--batch", "2", "--batchRiccati", "fast,accurate", "--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"))
    assert out.returncode != 2 and "--batchRiccati" not in out.stderr, (out.returncode, out.stderr)
    out = run(OPT, "--batch", "2", "--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"))
    assert out.returncode == 2 and "needs --fastRiccati 1" in out.stderr
