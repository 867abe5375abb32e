"""The consistency record of the filter batch (eqf_batch_consistency / eqvio_batch_consistency / eqvio_batch_run_sim_recorded, `eqvio_sim --batch B --record DIR`)
on a CPU-only box: the new entry points are exported and bound, the record's ctypes layout is the C one, bad arguments are refused before any device is looked
at, the command line refuses --record without --batch and accepts it with --batch up to the device check; and - by the CPU oracle alone - the eps of
tests/consistency_cases.py, which the GPU test (tests/test_gpu_batch_consistency.py) compares the device's records with, is the eps of computeNEES."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG = -3
NEW_DEVICE = ["eqf_batch_consistency"]
NEW_FILTER = ["eqvio_batch_consistency", "eqvio_batch_run_sim_recorded"]
EXE = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # no device to open: a run that tried would end with status 1


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
    from eqvio_amd.batch import BatchSlot, VIOFilterBatch

    assert callable(VIOFilterBatch.consistency) and callable(BatchSlot.consistency)
    assert "record_dir" in VIOFilterBatch.run_sim.__code__.co_varnames


def test_record_layout_is_the_c_one(libs, tmp_path):
    from eqvio_amd.batch import EQF_BATCH_NBLOCKS, BatchConsistencyRecord

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eqf_batch.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(eqf_batch_consistency_record), offsetof(eqf_batch_consistency_record, eps),\n'
                   '  offsetof(eqf_batch_consistency_record, ids), offsetof(eqf_batch_consistency_record, lm_err), (int)EQF_BATCH_NBLOCKS); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    size, o_eps, o_ids, o_err, nblocks = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(BatchConsistencyRecord)
    assert (o_eps, o_ids, o_err) == (BatchConsistencyRecord.eps.offset, BatchConsistencyRecord.ids.offset, BatchConsistencyRecord.lm_err.offset)
    assert nblocks == EQF_BATCH_NBLOCKS == 7


def test_bad_arguments_refused_without_a_device(libs):
    elib, flib = libs
    from eqvio_amd.batch import BatchConsistencyRecord, BatchTruth

    rec, st, t = (BatchConsistencyRecord * 2)(), (C.c_int * 2)(), (BatchTruth * 2)()
    assert elib.eqf_batch_consistency(None, 1, t, rec, st) == EQF_E_BAD_ARG
    assert elib.eqf_batch_consistency(None, -1, None, None, None) == EQF_E_BAD_ARG
    assert elib.eqf_batch_consistency(None, 0, None, None, None) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_consistency(None, 1, None, None, None, None, None, None, None) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_consistency(None, -1, None, None, None, None, None, rec, st) == EQF_E_BAD_ARG
    done = C.c_int()
    assert flib.eqvio_batch_run_sim_recorded(None, None, 4, None, C.byref(done), b"x") == EQF_E_BAD_ARG


def test_eqvio_sim_record_flag(libs, tmp_path):
    out = subprocess.run([EXE, "--record", str(tmp_path / "x")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--record needs --batch" in out.stderr, (out.returncode, out.stderr)
    assert not (tmp_path / "x").exists()
    out = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--record DIR" in out.stdout
    # with --batch the flag is accepted; --output stays refused
    out = subprocess.run([EXE, "--batch", "2", "--fastRiccati", "1", "--record", str(tmp_path / "y"), "--output", str(tmp_path / "z")], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 2 and "--batch does not support --output" in out.stderr


def test_eqvio_sim_record_reaches_the_device_check(libs, tmp_path):
    out = subprocess.run([EXE, "--batch", "2", "--fastRiccati", "1", "--record", str(tmp_path / "rec")], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, **NO_DEVICE))
    assert out.returncode == 1, (out.returncode, out.stdout, out.stderr)  # past the argument checks, stopped by the missing device (EQF_E_NO_DEVICE's message)
    assert "eqvio_batch_create" in out.stderr and "no gfx950" in out.stderr and "usage" not in out.stdout


@pytest.mark.parametrize("N", [0, 2, 5])
def test_helper_eps_is_pinned_by_the_oracle(libs, N):
    """With Sigma = I, n NEES = |eps|^2; with entry k of the diagonal at 1e-6 it grows by (1e6 - 1) eps_k^2: the oracle's computeNEES gives every eps_k^2."""
    import consistency_cases as cc

    for case in (c for c in cc.planted_cases() if c["N"] == N):
        n = 21 + 3 * N
        orc, state, truth = cc.OracleFilter(case["settings"]), case["state"], case["truth"]
        orc.set_eqf(*state, np.eye(n))
        base = orc.compute_nees(*truth)
        eps = case["exp"]["eps"]
        worst = 0.0
        for k in range(n):
            d = np.ones(n)
            d[k] = 1e-6
            orc.set_eqf(*state, np.diag(d))
            sq = n * (orc.compute_nees(*truth) - base) / (1e6 - 1)
            worst = max(worst, abs(sq - eps[k] ** 2))
        assert worst <= 1e-9 * np.max(eps ** 2), (case["chart"], N, worst, np.max(eps ** 2))


def test_helper_nees_is_the_oracles_on_the_planted_sigma(libs):
    import consistency_cases as cc

    for case in cc.planted_cases():
        ref = case["orc"].compute_nees(*case["truth"])
        assert abs(case["exp"]["nees"] - ref) <= 1e-9 * abs(ref), (case["chart"], case["N"], case["exp"]["nees"], ref)


def test_planted_eps_stays_away_from_zero(libs):
    """every entry of a planted case's eps is above consistency_cases.eps_floor, so the GPU test can ask for each entry to 1e-9 of itself"""
    import consistency_cases as cc

    for case in cc.planted_cases():
        assert np.min(np.abs(case["exp"]["eps"])) >= cc.eps_floor(case["state"], case["chart"]), (case["chart"], case["N"])
        assert cc.eps_floor(case["state"], case["chart"]) <= 1e-4
