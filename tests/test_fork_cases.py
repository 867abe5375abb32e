"""Forking a context and changing its chart, on a CPU-only box: eqf_chart / eqf_copy_ctx / eqf_convert_chart / eqf_fork_stats and eqvio_filter_copy /
eqvio_filter_convert_chart are declared in the headers, exported and bound; what they refuse on their arguments alone comes back without a device; eqvio_opt's
--branchAt / --branchCharts are checked before a file or device is opened; and the cases of tests/fork_cases.py are what tests/test_gpu_context_fork.py needs
them to be: far from a relabelling, two summation orders of the fp64 expectation 1e-12 apart, numpy within 1e-10 of 50 digits where that is affordable."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import fork_cases as fc
import rechart_cases as rcs
from eqvio_amd.capi import COORD_NORMAL
from util import rel_fro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = os.path.join(ROOT, "eqvio_amd", "lib", "eqvio_opt")
EQF_E_BAD_ARG = -3
NEW_DEVICE = ["eqf_chart", "eqf_copy_ctx", "eqf_convert_chart", "eqf_fork_stats"]
NEW_FILTER = ["eqvio_filter_copy", "eqvio_filter_convert_chart"]


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.capi import load_eqf_lib, load_filter_lib

    return load_eqf_lib(), load_filter_lib()


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------ declarations and exports
def test_declared_exported_and_bound(libs):
    elib, flib = libs
    h, fh = header("eqf_hip.h"), header("eqvio_filter.h")
    assert re.search(r"int\s+eqf_chart\s*\(\s*const\s+eqf_ctx\s*\*\s*\w+\s*\)", h)
    assert re.search(r"int\s+eqf_copy_ctx\s*\(\s*eqf_ctx\s*\*\s*dst\s*,\s*eqf_ctx\s*\*\s*src\s*\)", h)
    assert re.search(r"int\s+eqf_convert_chart\s*\(\s*eqf_ctx\s*\*\s*\w+\s*,\s*int\s+chart\s*\)", h)
    assert re.search(r"int\s+eqf_fork_stats\s*\(\s*eqf_ctx\s*\*\s*\w+\s*,\s*long\s*\*\s*copies_in\s*,\s*long\s*\*\s*rechart_launches\s*,\s*int\s+reset\s*\)", h)
    assert re.search(r"int\s+eqvio_filter_copy\s*\(\s*eqvio_filter\s*\*\s*dst\s*,\s*eqvio_filter\s*\*\s*src\s*\)", fh)
    assert re.search(r"int\s+eqvio_filter_convert_chart\s*\(\s*eqvio_filter\s*\*\s*\w+\s*,\s*int\s+chart\s*\)", fh)
    for n in NEW_DEVICE:
        assert hasattr(elib, n) and n in elib._declared, n
    for n in NEW_FILTER:
        assert hasattr(flib, n) and n in flib._declared, n
    from eqvio_amd.capi import EqfCore, VIOFilter

    assert isinstance(EqfCore.chart, property) and callable(EqfCore.copy_from) and callable(EqfCore.convert_chart) and callable(EqfCore.fork_stats)
    assert callable(VIOFilter.copy_from) and callable(VIOFilter.convert_chart)


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_refused_without_a_device(libs):
    elib, flib = libs
    a, b = C.c_long(7), C.c_long(7)
    assert elib.eqf_chart(None) == EQF_E_BAD_ARG
    assert elib.eqf_copy_ctx(None, None) == EQF_E_BAD_ARG
    assert elib.eqf_convert_chart(None, 0) == EQF_E_BAD_ARG and elib.eqf_convert_chart(None, 7) == EQF_E_BAD_ARG
    assert elib.eqf_fork_stats(None, C.byref(a), C.byref(b), 1) == EQF_E_BAD_ARG and (a.value, b.value) == (7, 7)
    assert flib.eqvio_filter_copy(None, None) == -1 and flib.eqvio_filter_convert_chart(None, 0) == -1
    assert EQF_E_BAD_ARG < 0


# ------------------------------------------------------------------------------------------------ the tool
def run(*args):
    return subprocess.run([OPT, *args], capture_output=True, text=True, timeout=120)


def test_tool_refuses_misuse_of_the_flags(libs, tmp_path):
    files = ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--fastRiccati", "1"]
    three = "euclidean,invdepth,normal"
    cases = [
        (["--batch", "3", "--branchAt", "10", "--branchCharts", three], "--branchAt"),  # beside --batch
        (["--batch", "3", "--branchCharts", three], "--branchCharts"),
        (["--branchAt", "10"], "--branchAt"),  # without each other
        (["--branchCharts", three], "--branchCharts"),
        (["--branchAt", "0", "--branchCharts", three], "--branchAt"),  # F <= 0
        (["--branchAt", "-4", "--branchCharts", three], "--branchAt"),
        (["--branchAt", "ten", "--branchCharts", three], "--branchAt"),
        (["--branchAt", "10", "--branchCharts", "euclidean,polar"], "--branchCharts"),  # an unknown word
        (["--branchAt", "10", "--branchCharts", "Normal"], "--branchCharts"),
        (["--branchAt", "10", "--branchCharts", "normal,"], "--branchCharts"),
        (["--branchAt", "10", "--branchCharts", three, "--sigmaFP32"], "--branchAt"),  # what a branch cannot carry
        (["--branchAt", "10", "--branchCharts", three, "--output", str(tmp_path / "out")], "--branchAt"),
        (["--branchAt", "10", "--branchCharts", three, "--dumpStates", str(tmp_path / "states.txt")], "--branchAt"),
    ]
    for args, flag in cases:
        out = run(*files, *args)
        assert out.returncode == 2, (args, out.returncode, out.stdout, out.stderr)
        assert flag in out.stderr and out.stderr.startswith("eqvio_opt: "), (args, out.stderr)
        assert not (tmp_path / "out").exists() and not (tmp_path / "states.txt").exists()


def test_existing_refusals_stay(libs, tmp_path):
    files = ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv"), "--fastRiccati", "1"]
    out = run(*files, "--rechart", "normal")
    assert out.returncode == 2 and "--rechart needs --batch" in out.stderr, out.stderr
    out = run(*files, "--warmup", "3")
    assert out.returncode == 2 and "--warmup 3: needs --batch B" in out.stderr, out.stderr
    out = run(*files, "--warmup", "3", "--rechart", "normal", "--branchAt", "3", "--branchCharts", "normal")
    assert out.returncode == 2 and "--rechart needs --batch" in out.stderr, out.stderr


def test_the_flags_get_past_the_argument_checks(libs, tmp_path):
    """past the argument checks the run opens its files, which are not there"""
    files = ["--imu", str(tmp_path / "no.csv"), "--features", str(tmp_path / "no2.csv")]
    for charts in ("euclidean,invdepth,normal", "normal", "invdepth,invdepth"):
        for extra in ([], ["--nis"], ["--fastRiccati", "1", "--groundtruth", str(tmp_path / "gt.csv")]):
            out = run(*files, "--branchAt", "10", "--branchCharts", charts, *extra)
            assert out.returncode == 1 and "--branch" not in out.stderr, (charts, extra, out.returncode, out.stderr)
    out = run("--help")
    assert out.returncode == 0 and "--branchAt" in out.stdout and "--branchCharts" in out.stdout


# ------------------------------------------------------------------------------------------------ the cases
def test_sizes_sit_on_both_sides_of_the_group_boundaries():
    assert set(rcs.NS) <= set(fc.SIZES) and 200 in fc.SIZES and max(fc.SIZES) > 512
    for last in (16, 32, 64):
        assert last in fc.SIZES and last + 1 in fc.SIZES and last % fc.RC_G == 0
        assert len(fc.groups(last + 1)) == len(fc.groups(last)) + 1 and fc.groups(last + 1)[-1] == (21 + 3 * last, 24 + 3 * last)
    for N in fc.SIZES:
        g = fc.groups(N)
        assert g[0] == (0, 21) and g[-1][1] == 21 + 3 * N and all(a[1] == b[0] for a, b in zip(g, g[1:]))
        assert all((hi - lo) % 3 == 0 and 0 < hi - lo <= 3 * fc.RC_G for lo, hi in g[1:])


def test_new_sizes_tell_the_charts_apart_and_have_a_sound_expectation():
    """at the sizes rechart_cases.NS does not have (tests/test_rechart_cases.py covers NS): a relabelling is far from the expectation; numpy's dense product and
    the block-by-block product agree to 1e-12; numpy is within 1e-10 of the 50-digit product where that is affordable"""
    t0 = time.perf_counter()
    rcs.T(max(fc.SIZES), rcs.CHARTS[0], COORD_NORMAL)
    t_T = time.perf_counter() - t0
    print(f"50-digit construction of T at N = {max(fc.SIZES)}, the Normal chart's blocks included: {t_T:.1f} s")
    worst_order = worst_mp = 0.0
    apart = []
    for N in fc.SIZES:
        S = rcs.case(N)[1]
        for a, b in rcs.PAIRS:
            E = rcs.expected(N, a, b)
            if N >= 1 or COORD_NORMAL in (a, b):
                d = rel_fro(E, S)
                apart.append(d)
                assert d > 1e-3, (N, rcs.pair_name((a, b)), d)
            else:
                assert np.array_equal(E, S)
            d = rel_fro(fc.block_congruence(rcs.T(N, a, b), S), E)
            worst_order = max(worst_order, d)
            assert d <= 1e-12, (N, rcs.pair_name((a, b)), d)
            if N <= fc.MP_MAX and N in fc.NEW_SIZES:
                d = rel_fro(E, rcs.expected_mp(N, a, b))
                worst_mp = max(worst_mp, d)
                assert d <= 1e-10, (N, rcs.pair_name((a, b)), d)
    print(f"T Sigma T^T against Sigma: at least {min(apart):.2e}; dense against block by block: {worst_order:.1e}; numpy against 50 digits (N <= {fc.MP_MAX}): {worst_mp:.1e}")
