"""Innovation statistics of the filter batch on a CPU-only box: the new entry points are exported, declared in the headers and in the Python lists and refuse
bad handles and slots before any device is looked at; `eqvio_opt --batch --sweep` refuses its misuses and `eqvio_sim --batch --innovation` is accepted up to
the device check; and - by the CPU oracle alone - every planted frame the GPU test (tests/test_gpu_batch_innovation.py) compares is well conditioned, its
float64 reference agrees with a 50-digit evaluation, and the score tells tunings of measurementNoise apart."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_scenarios as bs
import innovation_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG = -3
NEW_DEVICE = ["eqf_batch_last_innovation", "eqf_batch_innovation_totals", "eqf_batch_reset_innovation_totals"]
NEW_FILTER = ["eqvio_batch_last_innovation", "eqvio_batch_innovation_totals", "eqvio_batch_reset_innovation_totals"]
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
    for names, lib, hdr in ((NEW_DEVICE, elib, "eqf_batch.h"), (NEW_FILTER, flib, "eqvio_batch.h")):
        for n in names:
            assert hasattr(lib, n), n
            assert re.search(r"\b%s\s*\(" % n, header(hdr)), n
            assert n in lib._batch_declared, n
    from eqvio_amd.batch import VIOFilterBatch

    for m in ("last_innovation", "innovation_totals", "reset_innovation_totals"):
        assert callable(getattr(VIOFilterBatch, m)), m


def test_header_comment_says_what_S_is_and_leaves_the_likelihood_to_the_caller():
    txt = " ".join(open(os.path.join(ROOT, "include", "eqf_batch.h")).read().split())
    at = txt.index("Innovation statistics")
    doc = txt[at:txt.index("int eqf_batch_last_innovation", at)]
    assert "measurementNoise" in doc and "useEquivariantOutput" in doc
    assert "-1/2 (nis + logdet + dof ln 2 pi)" in doc


def test_bad_handles_and_slots_refused(libs):
    elib, flib = libs
    dof, n, d = C.c_int(7), C.c_long(7), C.c_double(7.0)
    for lib, pre in ((elib, "eqf"), (flib, "eqvio")):
        last, totals, reset = (getattr(lib, f"{pre}_batch_{x}") for x in ("last_innovation", "innovation_totals", "reset_innovation_totals"))
        for slot in (0, -1, 5):
            assert last(None, slot, C.byref(dof), C.byref(d), C.byref(d)) == EQF_E_BAD_ARG
            assert totals(None, slot, C.byref(n), C.byref(n), C.byref(d), C.byref(d)) == EQF_E_BAD_ARG
            assert reset(None, slot) == EQF_E_BAD_ARG
        assert last(None, 0, None, None, None) == EQF_E_BAD_ARG and totals(None, 0, None, None, None, None) == EQF_E_BAD_ARG
    assert (dof.value, n.value, d.value) == (7, 7, 7.0)  # a refused call writes nothing


OPT_MISUSES = {
    "sweep_without_batch": ["--fastRiccati", "1", "--sweep", "measurementNoise=1,2"],
    "too_few_values": ["--batch", "3", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2"],
    "too_many_values": ["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2,3"],
    "unknown_name": ["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoize=1,2"],
    "not_a_number": ["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,x"],
    "fast_riccati_off": ["--batch", "2", "--fastRiccati", "1", "--sweep", "fastRiccati=1,0"],
    "normal_chart": ["--batch", "2", "--fastRiccati", "1", "--sweep", "coordinateChoice=InvDepth,Normal"],
    "batch_without_fast_riccati": ["--batch", "2"],
    "batch_zero_slots": ["--batch", "-1", "--fastRiccati", "1"],
    "output": ["--batch", "2", "--fastRiccati", "1", "--output", "somewhere"],
    "dumpStates": ["--batch", "2", "--fastRiccati", "1", "--dumpStates", "states.txt"],
    "sigmaFP32": ["--batch", "2", "--fastRiccati", "1", "--sigmaFP32"],
}


@pytest.mark.parametrize("case", sorted(OPT_MISUSES))
def test_eqvio_opt_refuses_batch_misuse_without_a_device(libs, case, tmp_path):
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")
    files = ["--imu", str(tmp_path / "imu.csv"), "--features", str(tmp_path / "features.csv")]  # never opened: the refusal comes first
    out = subprocess.run([exe] + files + OPT_MISUSES[case], capture_output=True, text=True, timeout=60, env=dict(os.environ, **NO_DEVICE), cwd=tmp_path)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--batch" in out.stderr, out.stderr
    assert "NIS" not in out.stdout
    assert not os.listdir(tmp_path)


def test_eqvio_sim_innovation_flag_is_accepted_up_to_the_device(libs):
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    env = dict(os.environ, **NO_DEVICE)
    out = subprocess.run([exe, "--batch", "2", "--fastRiccati", "1", "--duration", "1", "--innovation"], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 1 and "eqvio_batch_create" in out.stderr, (out.returncode, out.stderr)  # past the argument checks, stopped by the missing device
    out = subprocess.run([exe, "--fastRiccati", "1", "--innovation"], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 2 and "--batch" in out.stderr, (out.returncode, out.stderr)
    out = subprocess.run([exe, "--batch", "2", "--innovation"], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 2 and "--batch needs --fastRiccati 1" in out.stderr  # the existing refusals keep their messages


@pytest.fixture(scope="module")
def references():
    return [(name, s, sc, ic.reference(s, sc)) for name, s, sc in ic.all_frames()]


def test_every_frame_is_well_conditioned_and_its_reference_exact(references):
    """cond(S) <= 1e6 on every frame the GPU test compares, and the float64 reference within a few ulps of the 50-digit value of the same S and yTilde"""
    worst_nis, worst_logdet = 0.0, 0.0
    for name, s, sc, ref in references:
        assert ref.dof > 0 and np.isfinite(ref.nis) and np.isfinite(ref.logdet), name
        assert ref.cond <= ic.COND_MAX, (name, ref.cond)
        nis, logdet = ic.exact(ref)
        g_nis, g_logdet = abs(ref.nis - nis) / nis, abs(ref.logdet - logdet)
        print(f"{name}: dof {ref.dof} cond(S) {ref.cond:.3g} NIS {ref.nis:.9g} (gap {g_nis:.2e} rel) log det S {ref.logdet:.9g} (gap {g_logdet:.2e} abs)")
        worst_nis, worst_logdet = max(worst_nis, g_nis), max(worst_logdet, g_logdet)
        assert g_nis <= 1e-12 and g_logdet <= 1e-12 * max(1.0, abs(logdet)), (name, g_nis, g_logdet)  # cond(S) eps = 2e-10 would be allowed; it is far less
    print(f"largest gap float64 to 50 digits: NIS {worst_nis:.3e} relative, log det S {worst_logdet:.3e} absolute")


def test_the_frames_are_the_sizes_and_edges_they_claim(references):
    by = {name: ref for name, _, _, ref in references}
    assert [by[f"inn{N}"].dof for N in ic.GRID] == [2, 16, 62, 64, 66, 126, 128]
    assert all(by[n].dof == 66 for n in by if n.startswith("inn33_c"))
    assert len([n for n in by if n.startswith("inn33_c")]) == 4
    frames = {name: (s, sc) for name, s, sc in ic.dof_frames()}
    s, sc = frames["rank64_cap"]  # 64 measured, 11 candidates, the cap of 5 binds
    d = bs.describe(s, sc)
    assert (len(sc.mid), d["n_abs"], d["n_prob"], d["max_outliers"], len(d["discarded"])) == (64, bs.C_ABS, bs.C_PROB, ic.RANK_CAP, ic.RANK_CAP)
    assert by["rank64_cap"].dof == 2 * (64 - ic.RANK_CAP)
    s, sc = frames["turnover16"]  # 64 landmarks lose 16 and gain 16: the new features count
    d = bs.describe(s, sc)
    assert (d["N_before"], len(d["lost"]), len(d["new"]), len(d["discarded"])) == (64, 16, 16, 0) and by["turnover16"].dof == 128
    s, sc = frames["keep_lost_8of64"]  # removeLostLandmarks = 0: 64 landmarks stay, 8 are measured
    d = bs.describe(s, sc)
    assert (d["N_before"], len(d["lost"]), len(sc.mid), len(d["discarded"])) == (64, 0, 8, 0) and by["keep_lost_8of64"].dof == 16


def test_the_score_tells_tunings_apart(references):
    """two tunings of measurementNoise on the same frame differ in NIS (and log det S) by more than 1e-3 relative: a score blind to the tuning would make the
    GPU comparison empty"""
    refs = [ref for name, _, _, ref in references if name.startswith("noise")]
    assert len(refs) == len(ic.NOISES) and len({r.dof for r in refs}) == 1
    for a in range(len(refs)):
        for b in range(a + 1, len(refs)):
            d_nis = abs(refs[a].nis - refs[b].nis) / max(refs[a].nis, refs[b].nis)
            d_ld = abs(refs[a].logdet - refs[b].logdet) / max(abs(refs[a].logdet), abs(refs[b].logdet))
            print(f"measurementNoise {ic.NOISES[a]} against {ic.NOISES[b]}: NIS differs by {d_nis:.3e}, log det S by {d_ld:.3e}")
            assert d_nis > 1e-3 and d_ld > 1e-3, (a, b, d_nis, d_ld)
