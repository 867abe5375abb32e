"""Per-slot settings of the filter batch on a CPU-only box: the new entry points are exported, declared in the headers and in the Python lists and
refuse null handles; `eqvio_sim --sweep` refuses its misuses before any device is opened; and - by the CPU oracle alone - every settings pair the GPU test
(tests/test_gpu_batch_slot_settings.py) runs in one step tells its two oracles apart by far more than the 1e-9 that test holds each slot to, so a kernel that
ignored a slot's settings could not pass it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import slot_settings_cases as ssc
from eqvio_amd.capi import Settings
from util import rel_fro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG, EQF_E_UNSUPPORTED = -3, -6
NEW_DEVICE = ["eqf_batch_check_settings", "eqf_batch_get_slot_settings", "eqf_batch_set_slot_settings"]
NEW_FILTER = ["eqvio_batch_get_slot_settings", "eqvio_batch_set_slot_settings"]
MARGIN = 1e-6  # relative difference of Sigma+ between the two oracles of a pair, at least


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
    from eqvio_amd.batch import BatchSlot, VIOFilterBatch

    for cls in (VIOFilterBatch, BatchSlot):
        assert callable(getattr(cls, "set_slot_settings")) and callable(getattr(cls, "get_slot_settings"))


def test_header_comments_state_the_new_rule():
    for hdr in ("eqf_batch.h", "eqvio_batch.h"):
        txt = open(os.path.join(ROOT, "include", hdr)).read()
        assert "hold for every slot" not in txt
        assert "set_slot_settings" in txt


def test_null_handles_and_settings_refused(libs):
    elib, flib = libs
    s, out = ssc.clone(ssc.cases()[0]), Settings()
    assert elib.eqf_batch_set_slot_settings(None, 0, C.byref(s)) == EQF_E_BAD_ARG
    assert elib.eqf_batch_get_slot_settings(None, 0, C.byref(out)) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_set_slot_settings(None, 0, C.byref(s)) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_get_slot_settings(None, 0, C.byref(out)) == EQF_E_BAD_ARG
    assert elib.eqf_batch_set_slot_settings(None, 0, None) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_set_slot_settings(None, 0, None) == EQF_E_BAD_ARG


def test_check_settings_gives_the_codes_of_create_and_set(libs):
    elib, _ = libs
    s = ssc.clone(ssc.cases()[0])
    assert elib.eqf_batch_check_settings(C.byref(s)) == 0
    assert elib.eqf_batch_check_settings(None) == EQF_E_BAD_ARG
    for field, value, code in (("fastRiccati", 0, EQF_E_UNSUPPORTED), ("coordinateChoice", 2, EQF_E_UNSUPPORTED), ("coordinateChoice", 7, EQF_E_BAD_ARG),
                               ("coordinateChoice", -1, EQF_E_BAD_ARG)):
        bad = ssc.clone(s)
        setattr(bad, field, value)
        assert elib.eqf_batch_check_settings(C.byref(bad)) == code, (field, value)
        h = C.c_void_p()
        assert elib.eqf_batch_create(C.byref(h), 0, 1, 8, C.byref(bad)) == code and not h.value  # the same code, before any device is looked at


SWEEP_MISUSES = {
    "without_batch": ["--fastRiccati", "1", "--sweep", "measurementNoise=1,2"],
    "too_few_values": ["--batch", "3", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2"],
    "too_many_values": ["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,2,3"],
    "unknown_name": ["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoize=1,2"],
    "no_values": ["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise"],
    "not_a_number": ["--batch", "2", "--fastRiccati", "1", "--sweep", "measurementNoise=1,x"],
    "fast_riccati_off": ["--batch", "2", "--fastRiccati", "1", "--sweep", "fastRiccati=1,0"],
    "normal_chart": ["--batch", "2", "--fastRiccati", "1", "--sweep", "coordinateChoice=InvDepth,Normal"],
    "chart_outside_the_enum": ["--batch", "2", "--fastRiccati", "1", "--sweep", "coordinateChoice=InvDepth,7"],
}


@pytest.mark.parametrize("case", sorted(SWEEP_MISUSES))
def test_eqvio_sim_refuses_sweep_misuse_without_a_device(libs, case):
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # no device to open: a run that tried would end with status 1
    out = subprocess.run([exe] + SWEEP_MISUSES[case], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "--sweep" in out.stderr, out.stderr
    assert "mean NEES" not in out.stdout


def test_existing_batch_refusals_keep_their_messages(libs):
    exe = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_sim")
    out = subprocess.run([exe, "--batch", "2", "--sweep", "measurementNoise=1,2"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--batch needs --fastRiccati 1" in out.stderr


@pytest.fixture(scope="module")
def pairs():
    """every case's two oracles on the case's frame"""
    base, cs = ssc.cases()
    return base, [(c, ssc.oracle_frame(c.settings, c.sc), ssc.oracle_frame(c.other, c.sc)) for c in cs]


def test_every_settings_pair_is_told_apart_by_the_oracle(pairs):
    base, ps = pairs
    assert len([c for c, _, _ in ps if not ssc.same_bytes(c.settings, base)]) >= 10
    for c, own, other in ps:
        if ssc.same_bytes(c.settings, c.other):
            assert c.name in ("unmodified", "equal_to_batch", "unmodified_b")
            continue
        ids_a, ids_b = own.get_eqf()[2], other.get_eqf()[2]
        if c.kind == "sigma":
            assert np.array_equal(ids_a, ids_b), c.name
            d = rel_fro(own.get_sigma(), other.get_sigma())
            print(f"{c.name}: Sigma+ differs by {d:.3e}")
            assert d > MARGIN, (c.name, d)
        elif c.kind == "state":
            # useDiscreteInnovationLift chooses how Gamma becomes a group element; it never enters the Riccati update, so Sigma+ is the same to the bit and
            # the flag shows in the lifted state alone, which the GPU test holds to the same 1e-9
            assert np.array_equal(ids_a, ids_b) and np.array_equal(own.get_sigma(), other.get_sigma()), c.name
            d = np.max(np.abs(own.state_estimate()[2] - other.state_estimate()[2]))
            print(f"{c.name}: landmark estimates differ by {d:.3e}")
            assert d > MARGIN, (c.name, d)
        elif c.kind in ("discards", "ids"):
            print(f"{c.name}: ids {ids_a.tolist()} against {ids_b.tolist()}")
            assert not np.array_equal(ids_a, ids_b), c.name
        else:
            da, db = ssc.new_depth(own, c.sc), ssc.new_depth(other, c.sc)
            print(f"{c.name}: depth {da!r} against {db!r}")
            assert abs(da - db) > MARGIN * db, (c.name, da, db)


def test_the_ranking_frame_is_what_it_claims(pairs):
    """N = 16 with 3 absolute and 2 probabilistic-only candidates; caps 0, 2 and 5 discard 0, 2 and 5 of them, the raised thresholds none"""
    import batch_scenarios as bs

    base, ps = pairs
    by = {c.name: (c, own) for c, own, _ in ps}
    for cap in ssc.CAPS:
        c, own = by[f"cap{cap}"]
        d = bs.describe(c.settings, c.sc)
        assert (d["N_before"], d["n_abs"], d["n_prob"], d["max_outliers"]) == (16, 3, 2, cap), (cap, d["n_abs"], d["n_prob"], d["max_outliers"])
        assert len(d["discarded"]) == cap and d["distinct"]
        assert len(own.get_eqf()[2]) == 16 - cap
    c, own = by["thresholds"]
    assert len(own.get_eqf()[2]) == 16
    c, own = by["removeLostLandmarks"]
    assert len(c.sc.mid) == 5 and len(own.get_eqf()[2]) == 12
    for name in ("fixed_depth", "median_depth"):
        assert len(by[name][0].sc.plan["new"]) == 3
    assert ssc.new_depth(by["fixed_depth"][1], by["fixed_depth"][0].sc) == pytest.approx(7.5, rel=1e-12)
