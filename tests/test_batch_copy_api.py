"""Copying slots of the filter batch (eqf_batch_copy_slots / eqvio_batch_copy_slots) on a CPU-only box: the new entry points are exported, declared in both
headers and in the Python lists, refuse null arguments before any device is looked at, and `eqvio_opt --warmup` refuses its misuses with status 2 before it
opens a file or a device. What the copy does is tests/test_gpu_batch_copy.py's."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG = -3
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # no device to open: a run that tried would end with status 1


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch import load_batch_protos

    return load_batch_protos()


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_new_symbols_exported_declared_and_listed(libs):
    elib, flib = libs
    for n, lib, hdr in (("eqf_batch_copy_slots", elib, "eqf_batch.h"), ("eqvio_batch_copy_slots", flib, "eqvio_batch.h")):
        assert hasattr(lib, n), n
        assert re.search(r"\bint\s+%s\s*\(\s*\w+\s*\*\s*b\s*,\s*int\s+count\s*,\s*const\s+int\s*\*\s*src\s*,\s*const\s+int\s*\*\s*dst\s*,\s*int\s*\*\s*status\s*\)\s*;" % n, header(hdr)), n
        assert n in lib._batch_declared, n
    from eqvio_amd.batch import BatchSlot, VIOFilterBatch

    assert callable(VIOFilterBatch.copy_slots) and callable(BatchSlot.copy_to)


def test_header_comment_says_what_is_kept_and_what_is_refused():
    txt = " ".join(open(os.path.join(ROOT, "include", "eqf_batch.h")).read().split())
    doc = txt[txt.rindex("/*", 0, txt.index("int eqf_batch_copy_slots")):txt.index("int eqf_batch_copy_slots")]
    for word in ("BEFORE the call", "bit for bit", "own settings", "innovation totals", "coordinateChoice", "EQF_E_BAD_ARG", "One launch"):
        assert word in doc, word


def test_null_arguments_are_refused_without_a_device(libs):
    elib, flib = libs
    one = (C.c_int * 1)(0)
    st = (C.c_int * 1)(7)
    for fn in (elib.eqf_batch_copy_slots, flib.eqvio_batch_copy_slots):
        assert fn(None, 1, one, one, st) == EQF_E_BAD_ARG
        assert fn(None, 0, one, one, st) == EQF_E_BAD_ARG
        assert fn(None, -1, one, one, st) == EQF_E_BAD_ARG
        assert fn(None, 1, None, None, None) == EQF_E_BAD_ARG
    assert st[0] == 7  # a refused call writes nothing


WARMUP_MISUSES = {
    "without_batch_and_sweep": (["--fastRiccati", "1", "--warmup", "10"], "needs --batch B and --sweep"),
    "without_sweep": (["--batch", "2", "--fastRiccati", "1", "--warmup", "10"], "needs --batch B and --sweep"),
    "negative": (["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2", "--warmup", "-3"], "needs F >= 0"),
    "not_a_number": (["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2", "--warmup", "ten"], "is not a number"),
    "trailing_text": (["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2", "--warmup", "10x"], "is not a number"),
    # a value that cannot reach a filter that already runs: the chart of a slot with landmarks, a variance that is read only when a filter starts
    "chart_sweep": (["--batch", "2", "--fastRiccati", "1", "--sweep", "coordinateChoice=Euclidean,InvDepth", "--warmup", "10"], "the chart cannot change"),
    "start_only_sweep": (["--batch", "2", "--fastRiccati", "1", "--sweep", "initialVelocityVariance=0.01,0.1", "--warmup", "10"], "only when a filter starts"),
}


@pytest.mark.parametrize("case", sorted(WARMUP_MISUSES))
def test_eqvio_opt_refuses_warmup_misuse_without_a_device(libs, case, tmp_path):
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")
    files = ["--imu", str(tmp_path / "imu.csv"), "--features", str(tmp_path / "features.csv")]  # never opened: the refusal comes first
    args, message = WARMUP_MISUSES[case]
    out = subprocess.run([exe] + files + args, capture_output=True, text=True, timeout=60, env=dict(os.environ, **NO_DEVICE), cwd=tmp_path)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--warmup" in out.stderr and message in out.stderr, out.stderr
    assert "NIS" not in out.stdout
    assert not os.listdir(tmp_path)


def test_a_valid_warmup_gets_past_the_argument_checks(libs, tmp_path):
    """accepted up to the first file: status 1 (the file is missing), not the refusals' 2"""
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")
    files = ["--imu", str(tmp_path / "imu.csv"), "--features", str(tmp_path / "features.csv")]
    #                                        without a warm-up these reach every slot before it starts       a value that every new landmark reads
    for sweep, f in (("measurementNoise=1,2", "0"), ("measurementNoise=1,2", "10"), ("coordinateChoice=Euclidean,InvDepth", "0"), ("initialVelocityVariance=0.01,0.1", "0"),
                     ("initialPointVariance=0.5,1", "10")):
        out = subprocess.run([exe] + files + ["--batch", "2", "--fastRiccati", "1", "--sweep", sweep, "--warmup", f], capture_output=True, text=True,
                             timeout=60, env=dict(os.environ, **NO_DEVICE), cwd=tmp_path)
        assert out.returncode == 1 and "--warmup" not in out.stderr, (out.returncode, out.stderr)


def test_help_mentions_warmup(libs):
    out = subprocess.run([os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt"), "--help"], capture_output=True, text=True, timeout=60, env=dict(os.environ, **NO_DEVICE))
    assert out.returncode == 0 and "--warmup F" in out.stdout
