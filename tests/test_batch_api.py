"""The filter batch's C-ABI (include/eqf_batch.h, include/eqvio_batch.h) on a CPU-only box: the libraries export what the headers declare, the Python
binding declares exactly that, and every refusal comes before the device is looked at."""
import ctypes as C
import os
import re

import pytest

from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_INVDEPTH, COORD_NORMAL, Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQF_E_BAD_ARG, EQF_E_NO_DEVICE, EQF_E_UNSUPPORTED = -3, -5, -6


def declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eqf_[A-Za-z0-9_]+|eqvio_[A-Za-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g

    g.build()
    from eqvio_amd.batch import load_batch_protos

    return load_batch_protos()


def settings(**kw):
    s = Settings.defaults()
    s.fastRiccati = 1
    s.coordinateChoice = COORD_INVDEPTH
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_headers_exported_and_declared(libs):
    elib, flib = libs
    dev, flt = declared("eqf_batch.h"), declared("eqvio_batch.h")
    assert len(dev) >= 14 and len(flt) >= 15
    for n in dev:
        assert hasattr(elib, n), n
    for n in flt:
        assert hasattr(flib, n), n
    assert elib._batch_declared == dev
    assert flib._batch_declared == flt


def test_existing_declared_lists_untouched(libs):
    elib, flib = libs
    assert not any(n.startswith("eqf_batch") for n in elib._declared)
    assert not any(n.startswith("eqvio_batch") for n in flib._declared)


@pytest.mark.parametrize("slots,cap,code", [(4, 0, EQF_E_BAD_ARG), (4, 65, EQF_E_BAD_ARG), (0, 40, EQF_E_BAD_ARG), (-1, 40, EQF_E_BAD_ARG)])
def test_bad_sizes_refused(libs, slots, cap, code):
    elib, flib = libs
    h = C.c_void_p()
    s = settings()
    assert elib.eqf_batch_create(C.byref(h), 0, slots, cap, C.byref(s)) == code
    assert flib.eqvio_batch_create(C.byref(h), C.byref(s), 0, slots, cap) == code
    assert not h.value


@pytest.mark.parametrize("kw", [dict(fastRiccati=0), dict(coordinateChoice=COORD_NORMAL), dict(fastRiccati=0, useDiscreteStateMatrix=1)])
def test_unsupported_modes_refused(libs, kw):
    elib, flib = libs
    h = C.c_void_p()
    s = settings(**kw)
    assert elib.eqf_batch_create(C.byref(h), 0, 8, 40, C.byref(s)) == EQF_E_UNSUPPORTED
    assert flib.eqvio_batch_create(C.byref(h), C.byref(s), 0, 8, 40) == EQF_E_UNSUPPORTED


def test_bad_handles_and_slots(libs):
    elib, flib = libs
    assert elib.eqf_batch_create(None, 0, 8, 40, C.byref(settings())) == EQF_E_BAD_ARG
    assert elib.eqf_batch_step(None, 1, None, None) == EQF_E_BAD_ARG
    assert elib.eqf_batch_set_sigma(None, 0, None, 21) == EQF_E_BAD_ARG
    assert elib.eqf_batch_get_state(None, 3, None, None, None, None, None, 0) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_process_imu(None, 0, None) == EQF_E_BAD_ARG
    assert flib.eqvio_batch_sigma_dim(None, 0) == EQF_E_BAD_ARG


def test_valid_arguments_reach_the_device_check(libs):
    """valid arguments: EQF_E_NO_DEVICE on a box without a gfx950 device, a working batch on one that has it"""
    elib, flib = libs
    have_gpu = False
    try:
        import torch

        have_gpu = torch.cuda.is_available()
    except ImportError:
        pass
    for chart in (COORD_EUCLIDEAN, COORD_INVDEPTH):
        s = settings(coordinateChoice=chart)
        h = C.c_void_p()
        rc = elib.eqf_batch_create(C.byref(h), 0, 8, 40, C.byref(s))
        assert rc == (0 if have_gpu else EQF_E_NO_DEVICE)
        if rc == 0:
            assert elib.eqf_batch_slots(h) == 8
            elib.eqf_batch_destroy(h)
        f = C.c_void_p()
        rc = flib.eqvio_batch_create(C.byref(f), C.byref(s), 0, 8, 64)
        assert rc == (0 if have_gpu else EQF_E_NO_DEVICE)
        if rc == 0:
            flib.eqvio_batch_destroy(f)
