"""Changing a slot's chart under landmarks on a CPU-only box: eqf_batch_convert_chart and eqvio_batch_convert_chart are declared in both headers, exported and
in the Python lists; their whole-call refusals come before any device is looked at; eqvio_opt's --rechart flag is checked before a file or device is opened.
(Everything a conversion does needs a batch, and a batch needs a device: tests/test_gpu_batch_rechart.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")
EQF_E_BAD_ARG = -3


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
    args = r"\s*b\s*,\s*int\s+count\s*,\s*const\s+int\s*\*\s*slots\s*,\s*const\s+int\s*\*\s*charts\s*,\s*int\s*\*\s*status\s*\)"
    assert re.search(r"int\s+eqf_batch_convert_chart\s*\(\s*eqf_batch\s*\*" + args, header("eqf_batch.h"))
    assert re.search(r"int\s+eqvio_batch_convert_chart\s*\(\s*eqvio_batch\s*\*" + args, header("eqvio_batch.h"))
    assert hasattr(elib, "eqf_batch_convert_chart") and "eqf_batch_convert_chart" in elib._batch_declared
    assert hasattr(flib, "eqvio_batch_convert_chart") and "eqvio_batch_convert_chart" in flib._batch_declared
    import eqvio_amd.batch as B

    assert callable(B.BatchCore.convert_chart) and callable(B.VIOFilterBatch.convert_chart) and callable(B.BatchSlot.convert_chart)
    # the calls that keep refusing a chart change under landmarks point to the new one
    text = " ".join(open(os.path.join(ROOT, "include", "eqf_batch.h")).read().split())
    assert text.count("eqf_batch_convert_chart") >= 5


def test_refused_without_a_device(libs):
    elib, flib = libs
    ip = C.POINTER(C.c_int)
    slots, charts, status = (np.zeros(2, np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(ip)  # noqa: E731
    fake = C.c_void_p(1)  # never dereferenced: every case below is refused on its arguments alone
    for lib, fn in ((elib, elib.eqf_batch_convert_chart), (flib, flib.eqvio_batch_convert_chart)):
        assert fn(None, 2, p(slots), p(charts), p(status)) == EQF_E_BAD_ARG
        assert fn(None, 0, p(slots), p(charts), p(status)) == EQF_E_BAD_ARG
        assert fn(fake, -1, p(slots), p(charts), p(status)) == EQF_E_BAD_ARG
        assert fn(fake, 2, None, p(charts), p(status)) == EQF_E_BAD_ARG
        assert fn(fake, 2, p(slots), None, p(status)) == EQF_E_BAD_ARG
        assert fn(fake, 2, p(slots), p(charts), None) == EQF_E_BAD_ARG
    assert not np.any(status)


def run(*args):
    return subprocess.run([OPT, *args], capture_output=True, text=True, timeout=120)


def test_tool_refuses_misuse_of_the_flag(libs, tmp_path):
    files = ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--fastRiccati", "1"]
    rec = ["--record", str(tmp_path / "rec")]
    three = "euclidean,invdepth,normal"
    cases = [
        (["--warmup", "3", "--rechart", three], False),  # without --batch
        (["--batch", "3", "--rechart", three], True),  # without --warmup
        (["--batch", "3", "--warmup", "0", "--rechart", three], True),  # ... or with F = 0
        (["--batch", "3", "--warmup", "3", "--rechart", "euclidean,normal"], True),  # a count other than 1 or B
        (["--batch", "2", "--warmup", "3", "--rechart", three], True),
        (["--batch", "3", "--warmup", "3", "--rechart", "euclidean,invdepth,polar"], True),  # an unknown word
        (["--batch", "3", "--warmup", "3", "--rechart", "Normal"], True),
        (["--batch", "3", "--warmup", "3", "--rechart", "normal,"], True),
        (["--batch", "3", "--warmup", "3", "--rechart", three, "--batchChart", "invdepth"], True),  # beside --batchChart
        (["--batch", "3", "--warmup", "3", "--rechart", three, "--sweep", "coordinateChoice=Euclidean,InvDepth,Euclidean"], True),  # beside a sweep of the chart
    ]
    for args, with_rec in cases:
        out = run(*files, *(rec if with_rec else []), *args)
        assert out.returncode == 2, (args, out.returncode, out.stdout, out.stderr)
        assert "--rechart" in out.stderr and out.stderr.startswith("eqvio_opt: "), (args, out.stderr)
        assert not (tmp_path / "rec").exists()


def test_existing_warmup_refusals_stay(libs, tmp_path):
    files = ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--fastRiccati", "1"]
    out = run(*files, "--batch", "2", "--sweep", "measurementNoise=1,2", "--warmup", "3", "--batchChart", "normal")
    assert out.returncode == 2 and "--batchChart" in out.stderr and "the chart cannot change under a filter that holds landmarks" in out.stderr, out.stderr
    out = run(*files, "--batch", "2", "--warmup", "3")
    assert out.returncode == 2 and "--warmup" in out.stderr, out.stderr


def test_the_flag_gets_past_the_argument_checks(libs, tmp_path):
    """with --warmup alone (no --sweep) and beside a --sweep: past the argument checks the run opens its files, which are not there"""
    files = ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--fastRiccati", "1"]
    for extra in ([], ["--sweep", "measurementNoise=1,2,3"], ["--warmupOnFilter"]):
        for charts in ("euclidean,invdepth,normal", "normal"):
            out = run(*files, "--batch", "3", "--warmup", "3", "--rechart", charts, *extra)
            assert out.returncode == 1 and "--rechart" not in out.stderr, (extra, charts, out.returncode, out.stderr)


def test_help_names_the_flag(libs):
    out = run("--help")
    assert out.returncode == 0 and "--rechart" in out.stdout
