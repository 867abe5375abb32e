"""The filter batch's Normal chart on a CPU-only box: eqf_batch_set_slot_chart / _get_slot_chart and their filter-level twins are declared in both headers,
exported and in the Python lists; their refusals come before any device is looked at; the settings calls keep refusing the Normal chart; the tools' --batchChart
flag is checked before a file or device is opened. (What eqf_batch_get_slot_settings reports of a slot's chart needs a batch, and a batch needs a device:
tests/test_gpu_batch_normal.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, Settings

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
    assert re.search(r"int\s+eqf_batch_set_slot_chart\s*\(\s*eqf_batch\s*\*\s*b\s*,\s*int\s+slot\s*,\s*int\s+chart\s*\)", dev)
    assert re.search(r"int\s+eqf_batch_get_slot_chart\s*\(\s*const\s+eqf_batch\s*\*\s*b\s*,\s*int\s+slot\s*\)", dev)
    assert re.search(r"int\s+eqvio_batch_set_slot_chart\s*\(\s*eqvio_batch\s*\*\s*b\s*,\s*int\s+slot\s*,\s*int\s+chart\s*\)", flt)
    assert re.search(r"int\s+eqvio_batch_get_slot_chart\s*\(\s*const\s+eqvio_batch\s*\*\s*b\s*,\s*int\s+slot\s*\)", flt)
    for lib, names in ((elib, ("eqf_batch_set_slot_chart", "eqf_batch_get_slot_chart")), (flib, ("eqvio_batch_set_slot_chart", "eqvio_batch_get_slot_chart"))):
        for n in names:
            assert hasattr(lib, n) and n in lib._batch_declared, n
    import eqvio_amd.batch as B

    assert callable(B.VIOFilterBatch.set_slot_chart) and callable(B.VIOFilterBatch.slot_chart) and isinstance(B.BatchSlot.chart, property)
    assert callable(B.BatchCore.set_slot_chart) and callable(B.BatchCore.slot_chart)
    # the header no longer says that the chart is missing, and says what of it still is
    text = " ".join(open(os.path.join(ROOT, "include", "eqf_batch.h")).read().split())
    assert "Only the Normal chart is not available" not in text
    assert re.search(r"eqf_batch_load_ctx / eqf_batch_store_ctx refuse a Normal-chart context", text)


def test_refused_without_a_device(libs):
    elib, flib = libs
    for chart in (COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, 3, -1):
        for slot in (0, -1, 5):
            assert elib.eqf_batch_set_slot_chart(None, slot, chart) == EQF_E_BAD_ARG
            assert flib.eqvio_batch_set_slot_chart(None, slot, chart) == EQF_E_BAD_ARG
    for slot in (0, -1):
        assert elib.eqf_batch_get_slot_chart(None, slot) == EQF_E_BAD_ARG
        assert flib.eqvio_batch_get_slot_chart(None, slot) == EQF_E_BAD_ARG
    # the settings calls keep their refusal of the Normal chart
    s = Settings.defaults()
    s.fastRiccati, s.coordinateChoice = 1, COORD_NORMAL
    assert elib.eqf_batch_check_settings(C.byref(s)) == EQF_E_UNSUPPORTED
    h = C.c_void_p()
    assert elib.eqf_batch_create(C.byref(h), 0, 2, 8, C.byref(s)) == EQF_E_UNSUPPORTED and not h
    assert elib.eqf_batch_set_slot_settings(None, 0, C.byref(s)) == EQF_E_BAD_ARG
    s.coordinateChoice = 3
    assert elib.eqf_batch_check_settings(C.byref(s)) == EQF_E_BAD_ARG


def have_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except ImportError:
        return False


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("exe,name", [(SIM, "eqvio_sim"), (OPT, "eqvio_opt")])
def test_tools_refuse_misuse_of_the_flag(libs, tmp_path, exe, name):
    files = [] if exe == SIM else ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv")]
    rec = ["--record", str(tmp_path / "rec")]
    for args in (["--batchChart", "normal"],  # without --batch
                 ["--batch", "4", "--batchChart", "euclidean,normal"], ["--batch", "4", "--batchChart", "normal,normal,normal,normal,normal"],  # wrong count
                 ["--batch", "4", "--batchChart", "Normal"], ["--batch", "4", "--batchChart", "polar"], ["--batch", "4", "--batchChart", "normal,"],  # unknown name
                 ["--batch", "2", "--batchChart", "invdepth,2"]):
        out = run(exe, *files, *(rec if "--batch" in args else []), "--fastRiccati", "1", *args)
        assert out.returncode == 2, (args, out.returncode, out.stdout, out.stderr)
        assert "--batchChart" in out.stderr and out.stderr.startswith(name + ": "), (args, out.stderr)
        assert not (tmp_path / "rec").exists()
    # the chart as a swept setting stays refused
    out = run(exe, *files, "--batch", "2", "--fastRiccati", "1", "--sweep", "coordinateChoice=Euclidean,Normal")
    assert out.returncode == 2 and "--sweep" in out.stderr, (out.returncode, out.stderr)
    # ... and two flags cannot both name the slots' charts
    out = run(exe, *files, "--batch", "2", "--fastRiccati", "1", "--sweep", "coordinateChoice=Euclidean,InvDepth", "--batchChart", "normal")
    assert out.returncode == 2 and "--batchChart" in out.stderr and "--sweep coordinateChoice" in out.stderr, (out.returncode, out.stderr)


def test_warmup_and_chart_do_not_combine(libs, tmp_path):
    out = run(OPT, "--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2",
              "--warmup", "3", "--batchChart", "normal")
    assert out.returncode == 2 and "--batchChart" in out.stderr, (out.returncode, out.stderr)


@pytest.mark.parametrize("exe", [SIM, OPT])
def test_help_names_the_flag(libs, exe):
    out = run(exe, "--help")
    assert out.returncode == 0 and "--batchChart" in out.stdout and "euclidean|invdepth|normal" in out.stdout


def test_the_flag_gets_past_the_argument_checks(libs, tmp_path):
    """past the argument checks the run needs a device: without one eqvio_sim ends with status 1 at eqvio_batch_create, with one it runs"""
    for charts, riccati in (("normal", []), ("euclidean,normal", ["--batchRiccati", "accurate,discrete"])):
        out = run(SIM, "--batch", "2", "--fastRiccati", "1", "--batchChart", charts, *riccati, "--duration", "0.2", "--maxFeatures", "10", "--quiet")
        if out.returncode == 0:
            assert "chart normal" in out.stdout
        else:
            assert out.returncode == 1 and "eqvio_batch_create" in out.stderr and not have_gpu(), (out.returncode, out.stderr)
        out = run(OPT, "--batch", "2", "--fastRiccati", "1", "--batchChart", charts, *riccati, "--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"))
        assert out.returncode != 2 and "--batchChart" not in out.stderr, (out.returncode, out.stderr)
