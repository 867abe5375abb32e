"""eqvio_amd/csrc/eqf_batch_ensemble_follow.h on a box without a GPU: the header declares exactly its one call with the eqf_bens_ prefix, the library exports it, the
binding declares it in a third list of its own (_batch_ensemble_follow_declared) while the other two lists are what they were, the entry struct has the header's
layout, the header states its contract and the older headers point to it, and null and out-of-range arguments are refused before any device is looked at.

The call's plan (eqvio_amd/csrc/eqf_batch_ensemble_follow_host.hpp, first half: kept / dropped / added, the old -> new map, the suffix rule, bad and repeated
slots, empty clouds) makes no HIP call, so it is driven here without a device: tests/batch_ensemble_follow_plan_main.cpp is built as a stand-alone program with
g++ -fsanitize=address,undefined and run on every cloud of the table and on every refusal. No sanitizer runs on code loaded into python."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from batch_ensemble_follow_cases import TABLE, get_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(ROOT, "eqvio_amd", "csrc", "eqf_batch_ensemble_follow.h")  # beside its implementation: include/ keeps its two eqf_bens headers
OLD_HEADERS = {"eqf_batch_ensemble.h": ["create", "destroy", "size", "stats", "set", "get", "sample_seeded", "integrate", "errors", "nees"],
               "eqf_batch_ensemble_output.h": ["likelihood", "resample_weighted_seeded", "covariance"]}
BAD_ARG, UNSUPPORTED = -3, -6


def declared_symbols(path, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[A-Za-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch_ensemble import load_batch_ensemble_protos

    return load_batch_ensemble_protos()


def test_header_declares_exactly_the_one_call():
    assert declared_symbols(HEADER, "eqf_bens_") == ["eqf_bens_follow"]
    assert not declared_symbols(HEADER, "eqf_batch_") and not declared_symbols(HEADER, "eqf_ensemble_")
    for name, calls in OLD_HEADERS.items():  # the fourteen existing calls are where they were
        assert declared_symbols(os.path.join(INCLUDE, name), "eqf_bens_") == sorted("eqf_bens_" + c for c in calls)
    # include/ is what it was: the two older headers are still the only ones there that name eqf_bens, and the new header needs nothing but them
    named = sorted(n for n in os.listdir(INCLUDE) if "eqf_bens" in open(os.path.join(INCLUDE, n)).read())
    assert named == ["eqf_batch_ensemble.h", "eqf_batch_ensemble_output.h"]
    assert re.findall(r'#include "([^"]+)"', open(HEADER).read()) == ["eqf_batch_ensemble.h"]


def test_library_exports_the_symbol(lib):
    raw = ctypes.CDLL(os.path.join(ROOT, "eqvio_amd", "lib", "libeqf_hip.so"))
    assert hasattr(raw, "eqf_bens_follow"), "eqf_bens_follow declared in eqvio_amd/csrc/eqf_batch_ensemble_follow.h but not exported"


def test_binding_declares_it_in_a_third_list(lib):
    assert lib._batch_ensemble_follow_declared == ["eqf_bens_follow"]
    assert sorted(lib._batch_ensemble_declared) == sorted("eqf_bens_" + c for c in OLD_HEADERS["eqf_batch_ensemble.h"])
    assert sorted(lib._batch_ensemble_output_declared) == sorted("eqf_bens_" + c for c in OLD_HEADERS["eqf_batch_ensemble_output.h"])
    from eqvio_amd.batch_ensemble import BatchEnsemble

    assert callable(BatchEnsemble.follow)


def test_entry_struct_has_the_headers_layout(lib):
    from eqvio_amd.batch_ensemble import BensFollowEntry

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct eqf_bens_follow_entry \{(.*?)\} eqf_bens_follow_entry;", txt, flags=re.S).group(1)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in BensFollowEntry._fields_] == ["slot", "seed", "stream"]
    assert ctypes.sizeof(BensFollowEntry) == 24 and BensFollowEntry.seed.offset == 8 and BensFollowEntry.stream.offset == 16


def test_header_states_the_contract():
    txt = " ".join(open(HEADER).read().replace("\n *", " ").split())
    for phrase in ("FOLLOW THEIR SLOT'S LANDMARK TURNOVER", "NOTHING P-SIZED CROSSES THE BUS", "THE 23 SENSOR PLANES ARE UNTOUCHED", "THE BYTES THEY HELD",
                   "CONDITIONAL ON WHAT THE PARTICLE ALREADY IS", "z_K = L_KK^-1 eps_K", "eps_A = L_AK z_K + L_AA Xi_A", "normals(seed, stream, n, P)",
                   "WITHOUT EVER FORMING THE SCHUR COMPLEMENT", "Sigma_AK = 0", "generateInitialStateParticles", "THE SUFFIX RULE", "A is a suffix of F",
                   "both the step and eqf_batch_augment append new landmarks at the end", "no permuted factorisation", "EQF_E_UNSUPPORTED", "BEFORE ANY DEVICE WORK",
                   "untouched bit for bit", "SLOT IS READ ONLY", "no kernel communicates between workgroups", "every sum has a fixed order",
                   "A PARTICLE'S BYTES DEPEND ON ITS SLOT'S DATA, ITS OWN DATA AND (SEED, STREAM) ALONE", "EQF_E_BAD_ARG", "EQF_E_NOT_SPD", "EQF_E_CAPACITY",
                   "only after the flags have been read", "ENTRIES THAT DO LESS", "a no-op", "no factorisation is counted", "INVALIDATES", "LAUNCHES PER CALL",
                   "So 4, 2, 5 or 0", "v_mfma_f64_16x16x4_f64", "second place", "freed by eqf_bens_destroy", "one small copy back", "Out of scope",
                   "caller-supplied normals", "not a suffix", "weighted (un-resampled) covariance or NEES"):
        assert phrase in txt, phrase
    for name in OLD_HEADERS:  # the older headers point here instead of listing the item as not built
        old = " ".join(open(os.path.join(INCLUDE, name)).read().replace("\n *", " ").split())
        assert "eqf_batch_ensemble_follow.h" in old, name


def test_null_and_out_of_range_arguments_are_refused_before_the_device(lib):
    from eqvio_amd.batch_ensemble import BensFollowEntry

    i4 = (ctypes.c_int * 4)()
    fe = (BensFollowEntry * 1)()
    assert lib.eqf_bens_follow(None, 1, fe, i4, i4, i4) == BAD_ARG
    assert lib.eqf_bens_follow(None, 0, fe, i4, i4, i4) == BAD_ARG
    fake = ctypes.c_void_p(1)  # never dereferenced: the count and the null lists are refused first
    assert lib.eqf_bens_follow(fake, -1, fe, i4, i4, i4) == BAD_ARG
    assert lib.eqf_bens_follow(fake, 1, None, i4, i4, i4) == BAD_ARG
    assert lib.eqf_bens_follow(fake, 1, fe, i4, i4, None) == BAD_ARG
    assert lib.eqf_bens_follow(fake, 0, None, None, None, None) == 0  # nothing listed: nothing to do


# ---- the plan, stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("follow_plan") / "follow_plan")
    src = os.path.join(ROOT, "tests", "batch_ensemble_follow_plan_main.cpp")
    # the sanitizers' runtimes are linked into the program itself: it needs nothing of the environment it is started in
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INCLUDE,
                    "-I", os.path.dirname(HEADER), "-o", exe, src], check=True)
    return exe


def run_plan(exe, calls):
    """calls: list of (slots [(P, F, G)], entry slots); returns per call the list of output rows (ints)"""
    text = ""
    for slots, entries in calls:
        text += f"{len(slots)}\n"
        for P, F, G in slots:
            text += " ".join(str(int(v)) for v in [P, len(F), *F, len(G), *G]) + "\n"
        text += " ".join(str(int(v)) for v in [len(entries), *entries]) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    out, at = [], 0
    for _, entries in calls:
        out.append(rows[at:at + len(entries)])
        at += len(entries)
    assert at == len(rows)
    return out


def expected_row(P, F, G):
    """the plan restated: [status] or [0, nK, nD, nA, noop, moves, from ...]"""
    F, G = [int(v) for v in F], [int(v) for v in G]
    if P < 1:
        return [BAD_ARG]
    held = [f in G for f in F]
    nK = held.index(False) if False in held else len(F)
    if any(held[nK:]):
        return [UNSUPPORTED]
    frm = [G.index(f) for f in F[:nK]]
    moves = frm != list(range(nK))
    nD, nA = len(G) - nK, len(F) - nK
    return [0, nK, nD, nA, int(nA == 0 and nD == 0 and not moves), int(moves), *frm]


def test_plan_of_every_cloud_of_the_table(plan_program):
    slots = [(get_case(*t).P, get_case(*t).c.ids, get_case(*t).cloud[0]) for t in TABLE]
    got = run_plan(plan_program, [(slots, list(range(len(TABLE))))])[0]
    for t, row in zip(TABLE, got):
        fc = get_case(*t)
        assert row == expected_row(fc.P, fc.c.ids, fc.cloud[0]), t
        assert row[0] == 0 and row[1] == fc.nK and (row[2], row[3]) == fc.counts and row[4] == 0 and row[5] == int(fc.moves), t


def test_plan_refusals_no_ops_and_random_lists(plan_program):
    F = [7, 3, 9, 4]
    slots = [(5, F, [7, 3, 9, 4]),        # 0: in step: a no-op
             (5, F, [3, 7]),              # 1: lacks a suffix, the kept ones swapped
             (5, F, [7, 9]),              # 2: lacks 3, which sits in front of 9: the suffix rule is broken
             (5, F, [4]),                 # 3: holds only the last: broken
             (0, F, []),                  # 4: an empty cloud
             (5, [], [11, 12]),           # 5: a slot without landmarks: drops only, nothing moves
             (5, F, [7, 3, 9, 4, 100]),   # 6: a foreign id behind the kept ones: drops only, no move
             (5, F, [100, 7, 3, 9, 4]),   # 7: ... in front of them: a move
             (1, list(range(64)), list(range(63, -1, -1))),  # 8: the capacity, reversed
             (1, [], [])]                 # 9: nothing on either side: a no-op
    entries = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, -1, 3, 0, 2147483647, -2147483648]
    got = run_plan(plan_program, [(slots, entries)])[0]
    want = [expected_row(*slots[s]) for s in range(10)] + [[BAD_ARG]] * 6  # 10, -1, the int limits: no such slot; 3, 0: listed twice
    assert got == want
    assert got[0] == [0, 4, 0, 0, 1, 0, 0, 1, 2, 3] and got[1] == [0, 2, 0, 2, 0, 1, 1, 0] and got[2] == [UNSUPPORTED] and got[3] == [UNSUPPORTED] and got[4] == [BAD_ARG]
    assert got[5] == [0, 0, 2, 0, 0, 0] and got[6] == [0, 4, 1, 0, 0, 0, 0, 1, 2, 3] and got[7] == [0, 4, 1, 0, 0, 1, 1, 2, 3, 4] and got[9] == [0, 0, 0, 0, 1, 0]
    # a refused first listing still lists its slot: the second entry of slot 2 is a repetition, not a second opinion
    assert run_plan(plan_program, [(slots, [2, 2, 4, 4])])[0] == [[UNSUPPORTED], [BAD_ARG], [BAD_ARG], [BAD_ARG]]
    rng = np.random.default_rng(31)
    calls = []
    for _ in range(200):
        B = int(rng.integers(1, 6))
        sl = []
        for _ in range(B):
            N, NG = int(rng.integers(0, 65)), int(rng.integers(0, 65))
            pool = rng.permutation(90)
            F_, cut = pool[:N], int(rng.integers(0, N + 1))
            own = F_[:cut] if rng.random() < 0.7 else F_[rng.random(N) < 0.7]  # mostly a prefix of the slot's order, sometimes any subset
            G_ = rng.permutation(np.concatenate([own, 1000 + np.arange(max(0, min(NG, 64 - len(own))))]))
            sl.append((int(rng.integers(0, 3)), F_.tolist(), G_.tolist()))
        calls.append((sl, rng.integers(-1, B + 1, int(rng.integers(0, 8))).tolist()))
    for (sl, entries), rows in zip(calls, run_plan(plan_program, calls)):
        seen = set()
        for s, row in zip(entries, rows):
            if s < 0 or s >= len(sl) or s in seen:
                assert row == [BAD_ARG]
                continue
            seen.add(s)
            assert row == expected_row(*sl[s])
