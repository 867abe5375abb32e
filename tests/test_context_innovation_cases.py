"""The frames of tests/context_innovation_cases.py on the CPU: every frame's S is well conditioned and its float64 reference exact (so that the GPU bound of
tests/test_gpu_context_innovation.py reads the device, not the reference); the select frames really discard landmarks; the planted failure really fails; and
what needs no device of the new entry points: the null-context refusal, the exported symbols, the command lines' refusal of --nis with --batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import context_innovation_cases as cic
import context_scenarios as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    g.build()


@pytest.mark.parametrize("name", [sc.name for sc, _ in cic.FRAMES])
def test_every_frame_is_well_conditioned_and_its_reference_exact(name):
    sc, _ = cic.FRAME_BY_NAME[name]
    run, refs = cic.oracle_run(sc)
    assert len(refs) == sc.frames == len(run.frames)
    for k, ref in enumerate(refs):
        assert np.all(np.isfinite(ref.S)) and np.linalg.eigvalsh(ref.S)[0] > 0, (name, k)
        g_nis, g_ld = cic.exact_gap(ref)
        print(f"{name}[{k}]: dof {ref.dof}  cond(S) {ref.cond:.3g}  NIS {ref.nis!r} gap {g_nis:.2e}  log det S {ref.logdet!r} gap {g_ld:.2e}")
        assert ref.cond < cic.COND_MAX, (name, k, ref.cond)
        assert g_nis <= cic.EXACT_GAP, (name, k, g_nis)
        assert g_ld <= cic.EXACT_GAP * max(1.0, abs(ref.logdet)), (name, k, g_ld)


def test_the_frames_are_the_shapes_they_are_meant_to_be():
    by = {sc.name: sc for sc, _ in cic.FRAMES}
    assert [by[f"inn_update_N{N}"].NJ for N in (1, 16, 17, 40, 200, 257)] == [1, 1, 2, 3, 13, 17] and by["update_inv_N513"].NJ == 33
    assert 2 * 17 - 32 == 2 and 2 * 200 % 32 == 16  # a second panel of width 2; a ragged last panel
    assert [cs.lookahead_fits(N, N) for N in (1, 16, 17, 40, 200, 257, 513)] == [False, False, False, True, True, True, False]
    assert [by[f"inn_staged_N{N}"].NJ for N in (40, 129, 257)] == [3, 9, 17]  # ZB = 2 | k_build_Z in front (9 panels) | the 17 .. 32-panel form; then ZB = 3
    assert sum(1 for sc, _ in cic.FRAMES if sc.N > 257) == 2  # the natural chain and the masked columns above 16 panels: the forms that exist only there
    assert by["select_inv_N40_M36"].NJ == 3 and by["select_inv_N200_M190"].NJ <= 16 < by["select_inv_N513_M257"].NJ and by["select_inv_N513_M257"].N > 512


@pytest.mark.parametrize("name", cic.SELECT)
def test_select_frames_discard_landmarks_and_the_reference_counts_the_kept(name):
    sc, _ = cic.FRAME_BY_NAME[name]
    run, refs = cic.oracle_run(sc)
    discarded = run.candidates[2]
    assert 0 < len(discarded) == sc.cap  # the cap binds
    assert all(i in sc.measured for i in discarded)
    assert refs[0].dof == 2 * (sc.M - len(discarded)) < 2 * sc.M


def test_the_planted_failure_has_no_cholesky_factor():
    sc = cic.NOT_SPD
    run, _ = cic.oracle_run(sc)
    orc = cic.OracleFilter(sc.settings())
    orc.set_eqf(*run.state0, cic.not_spd_sigma(sc), time=0.0)
    fr = run.frames[0]
    orc.integrate_riccati_fast(fr.mean, fr.total)
    ref = cic.reference_at(orc, sc.settings(), cs.CAMERAS[sc.cam], fr.mid, fr.y)
    assert ref.dof == 16 and np.isnan(ref.nis) and np.isnan(ref.logdet)
    assert ref.S[0, 0] < 0  # the first pivot already


# ------------------------------------------------------------------------------------------------ no device needed
def test_a_null_context_is_refused_and_a_refused_call_writes_nothing():
    from eqvio_amd.capi import load_eqf_lib

    lib = load_eqf_lib()
    dof, nis, logdet = C.c_int(-7), C.c_double(-7.5), C.c_double(-8.5)
    upd, tdof = C.c_long(-9), C.c_long(-10)
    assert lib.eqf_last_innovation(None, C.byref(dof), C.byref(nis), C.byref(logdet)) == -3
    assert lib.eqf_innovation_totals(None, C.byref(upd), C.byref(tdof), C.byref(nis), C.byref(logdet)) == -3
    assert lib.eqf_reset_innovation_totals(None) == -3
    assert (dof.value, nis.value, logdet.value, upd.value, tdof.value) == (-7, -7.5, -8.5, -9, -10)
    assert lib.eqf_last_innovation(None, None, None, None) == -3


def test_the_entry_points_are_exported_and_declared():
    from eqvio_amd.capi import OPT_INNOVATION_STATS, EqfCore, VIOFilter, load_eqf_lib, load_filter_lib

    assert OPT_INNOVATION_STATS == 30
    header = open(os.path.join(ROOT, "include", "eqf_hip.h")).read()
    assert "EQF_OPT_INNOVATION_STATS = 30" in header
    lib, flib = load_eqf_lib(), load_filter_lib()
    for n in ("eqf_last_innovation", "eqf_innovation_totals", "eqf_reset_innovation_totals"):
        assert n in lib._declared and hasattr(lib, n) and n + "(" in header
    fheader = open(os.path.join(ROOT, "include", "eqvio_filter.h")).read()
    for n in ("eqvio_filter_set_innovation_stats", "eqvio_filter_last_innovation", "eqvio_filter_innovation_totals", "eqvio_filter_reset_innovation_totals"):
        assert n in flib._declared and hasattr(flib, n) and n + "(" in fheader
    for cls in (EqfCore, VIOFilter):
        for m in ("last_innovation", "innovation_totals", "reset_innovation_totals"):
            assert callable(getattr(cls, m))
    assert callable(VIOFilter.set_innovation_stats)
    assert lib.eqf_kernel_name(15) == b"k_innovation_stats"  # the KN_ slot eqf_last_kernel_times reports the new kernel in


@pytest.mark.parametrize("tool", ["eqvio_opt", "eqvio_sim"])
def test_nis_with_batch_is_refused_before_anything_is_opened(tool, tmp_path):
    exe = os.path.join(ROOT, "eqvio_amd", "lib", tool)
    missing = str(tmp_path / "not_there")
    args = [exe, "--nis", "--batch", "2"]
    if tool == "eqvio_opt":  # files that do not exist: opening them would be another error, with status 1
        args = [exe, "--imu", os.path.join(missing, "imu.csv"), "--features", os.path.join(missing, "features.csv"), "--fastRiccati", "1", "--nis", "--batch", "2"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--batch" in r.stderr and "--nis" in r.stderr
    assert r.stdout == "" and not os.path.exists(missing)
