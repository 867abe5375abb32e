"""The feature predictions of the filter batch (eqf_batch_predictions / eqvio_batch_feature_predictions, `eqvio_opt --batch B --predictions`) on a CPU-only box:
the new entry points are exported, declared in the headers and bound, the record's ctypes layout is the C one and has no padding, bad arguments are refused
before any device is looked at, and the command line refuses --predictions without --batch before it opens a file."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG = -3
NEW_DEVICE = ["eqf_batch_predictions", "eqf_batch_sensor_estimate"]
NEW_FILTER = ["eqvio_batch_feature_predictions"]
EXE = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch import load_batch_protos

    return load_batch_protos()


def test_new_symbols_exported_and_bound(libs):
    elib, flib = libs
    for names, lib, hdr in ((NEW_DEVICE, elib, "eqf_batch.h"), (NEW_FILTER, flib, "eqvio_batch.h")):
        txt = open(os.path.join(ROOT, "include", hdr)).read()
        for n in names:
            assert hasattr(lib, n), n
            assert n in lib._batch_declared, n
            assert f"int {n}(" in txt, n
    from eqvio_amd.batch import BatchPredictionRecord, BatchSlot, VIOFilterBatch

    assert callable(VIOFilterBatch.predictions) and callable(VIOFilterBatch.feature_predictions) and callable(BatchSlot.feature_predictions)
    assert callable(BatchPredictionRecord.trimmed)


def compiled_layout(tmp_path, struct, fields):
    """sizeof and the fields' offsetof of a struct of eqf_batch.h, from a compiled C program"""
    src = tmp_path / f"{struct}.c"
    offs = ", ".join(f"offsetof({struct}, {f})" for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eqf_batch.h"\n'
                   f'int main(void) {{ size_t v[] = {{sizeof({struct}), {offs}, (size_t)EQF_BATCH_MAX_LANDMARKS}};\n'
                   '  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);\n  return 0; }\n')
    exe = tmp_path / struct
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_record_layout_is_the_c_one(libs, tmp_path):
    from eqvio_amd.batch import EQF_BATCH_MAX_LANDMARKS, BatchPredictionEntry as En, BatchPredictionRecord as R

    fields = [name for name, _ in R._fields_]
    assert fields == ["N", "reserved", "sensor", "ids", "p", "y", "out_cov"]
    size, *offsets, cap = compiled_layout(tmp_path, "eqf_batch_prediction_record", fields)
    assert size == C.sizeof(R)
    assert offsets == [getattr(R, f).offset for f in fields]
    assert cap == EQF_BATCH_MAX_LANDMARKS == 64
    # the fields fill the record: no padding byte whose value a comparison of records would depend on
    assert size == 8 + 8 * 23 + 4 * 64 + 8 * (3 + 2 + 4) * 64
    fields = [name for name, _ in En._fields_]
    size, *offsets, _ = compiled_layout(tmp_path, "eqf_batch_prediction_entry", fields)
    assert size == C.sizeof(En) and offsets == [getattr(En, f).offset for f in fields]


def test_bad_arguments_refused_without_a_device(libs):
    elib, flib = libs
    from eqvio_amd.batch import BatchPredictionEntry, BatchPredictionRecord
    from eqvio_amd.capi import Camera

    ent, rec, st = (BatchPredictionEntry * 2)(), (BatchPredictionRecord * 2)(), (C.c_int * 2)()
    C.memset(rec, 0xA5, C.sizeof(rec))
    assert elib.eqf_batch_predictions(None, 1, ent, rec, st) == EQF_E_BAD_ARG
    assert elib.eqf_batch_predictions(None, 0, ent, rec, st) == EQF_E_BAD_ARG
    assert elib.eqf_batch_predictions(None, -1, None, None, None) == EQF_E_BAD_ARG
    assert elib.eqf_batch_sensor_estimate(None, 0, (C.c_double * 23)()) == EQF_E_BAD_ARG
    sl, cams, stamps = (C.c_int * 2)(0, 1), (Camera * 2)(), (C.c_double * 2)()
    assert flib.eqvio_batch_feature_predictions(None, 1, sl, cams, stamps, rec, st) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_feature_predictions(None, 0, sl, cams, stamps, rec, st) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_feature_predictions(None, -1, None, None, None, None, None) == EQF_E_BAD_ARG
    assert bytes(rec) == b"\xa5" * C.sizeof(rec)


def test_eqvio_opt_predictions_flag(libs, tmp_path):
    out = subprocess.run([EXE, "--predictions"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--predictions needs --batch" in out.stderr, (out.returncode, out.stderr)
    # ... before any file is opened: with dataset files named that do not exist, the refusal is the same
    out = subprocess.run([EXE, "--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--predictions"], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 2 and "--predictions needs --batch" in out.stderr, (out.returncode, out.stderr)
    assert os.listdir(tmp_path) == []
    out = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--predictions" in out.stdout
    # with --batch the flag is accepted: the next refusal is the batch's own
    out = subprocess.run([EXE, "--batch", "2", "--predictions"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "needs --fastRiccati 1" in out.stderr, (out.returncode, out.stderr)
    assert os.listdir(tmp_path) == []
