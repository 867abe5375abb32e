"""The estimate records of the filter batch (eqf_batch_estimates / eqvio_batch_estimates / eqvio_batch_run_prepared_recorded, `eqvio_opt --batch B --record DIR`)
on a CPU-only box: the new entry points are exported, declared in the headers and bound, the record's ctypes layout is the C one, bad arguments are refused
before any device is looked at, and the command line refuses --record without --batch while --output stays refused with --batch."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG = -3
NEW_DEVICE = ["eqf_batch_estimates"]
NEW_FILTER = ["eqvio_batch_estimates", "eqvio_batch_run_prepared_recorded"]
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
    from eqvio_amd.batch import BatchEstimateRecord, VIOFilterBatch

    assert callable(VIOFilterBatch.state_estimates) and callable(BatchEstimateRecord.trimmed)
    assert "record_dir" in VIOFilterBatch.run_prepared.__code__.co_varnames


def test_record_layout_is_the_c_one(libs, tmp_path):
    from eqvio_amd.batch import EQF_BATCH_MAX_LANDMARKS, BatchEstimateRecord as R

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eqf_batch.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(eqf_batch_estimate_record), offsetof(eqf_batch_estimate_record, N),\n'
                   '  offsetof(eqf_batch_estimate_record, reserved), offsetof(eqf_batch_estimate_record, sensor), offsetof(eqf_batch_estimate_record, sigma_sensor),\n'
                   '  offsetof(eqf_batch_estimate_record, ids), offsetof(eqf_batch_estimate_record, p), offsetof(eqf_batch_estimate_record, p_world),\n'
                   '  (int)EQF_BATCH_MAX_LANDMARKS); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    size, o_n, o_res, o_sensor, o_sigma, o_ids, o_p, o_pw, cap = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(R)
    assert (o_n, o_res, o_sensor, o_sigma, o_ids, o_p, o_pw) == (R.N.offset, R.reserved.offset, R.sensor.offset, R.sigma_sensor.offset, R.ids.offset, R.p.offset,
                                                                R.p_world.offset)
    assert cap == EQF_BATCH_MAX_LANDMARKS == 64
    # the fields fill the record: no padding byte whose value a comparison of records would depend on
    assert size == 8 + 8 * 23 + 8 * 441 + 4 * cap + 2 * 8 * 3 * cap


def test_bad_arguments_refused_without_a_device(libs):
    elib, flib = libs
    from eqvio_amd.batch import BatchEstimateRecord

    rec, st, sl, times = (BatchEstimateRecord * 2)(), (C.c_int * 2)(), (C.c_int * 2)(0, 1), (C.c_double * 2)()
    assert elib.eqf_batch_estimates(None, 1, sl, rec, st) == EQF_E_BAD_ARG
    assert elib.eqf_batch_estimates(None, 0, sl, rec, st) == EQF_E_BAD_ARG
    assert elib.eqf_batch_estimates(None, -1, None, None, None) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_estimates(None, 1, sl, rec, times, st) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_estimates(None, 0, sl, rec, None, st) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_estimates(None, -1, None, None, None, None) == EQF_E_BAD_ARG
    seqs = (C.c_void_p * 2)()
    assert flib.eqvio_batch_run_prepared_recorded(None, seqs, 0, 1, b"x") == EQF_E_BAD_ARG  # a null batch
    assert flib.eqvio_batch_run_prepared_recorded(None, seqs, 0, 1, None) == EQF_E_BAD_ARG  # and a null directory
    assert flib.eqvio_batch_run_prepared_recorded(None, None, 0, 1, b"x") == EQF_E_BAD_ARG
    assert not os.path.exists("x")


def test_eqvio_opt_record_flag(libs, tmp_path):
    out = subprocess.run([EXE, "--record", str(tmp_path / "x")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--record needs --batch" in out.stderr, (out.returncode, out.stderr)
    assert not (tmp_path / "x").exists()
    # ... before any file is opened: with dataset files named that do not exist, the refusal is the same
    out = subprocess.run([EXE, "--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--record", str(tmp_path / "x")], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 2 and "--record needs --batch" in out.stderr, (out.returncode, out.stderr)
    assert not (tmp_path / "x").exists()
    out = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--record DIR" in out.stdout
    # with --batch the flag is accepted; --output stays refused with its present message
    out = subprocess.run([EXE, "--batch", "2", "--fastRiccati", "1", "--record", str(tmp_path / "y"), "--output", str(tmp_path / "z")], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 2 and "does not support --output" in out.stderr, (out.returncode, out.stderr)
    assert not (tmp_path / "y").exists() and not (tmp_path / "z").exists()
    for flag, msg in ((["--dumpStates", str(tmp_path / "s")], "does not support --dumpStates"), (["--sigmaFP32"], "does not support --sigmaFP32")):
        out = subprocess.run([EXE, "--batch", "2", "--fastRiccati", "1", "--record", str(tmp_path / "y"), *flag], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and msg in out.stderr, (flag, out.returncode, out.stderr)
