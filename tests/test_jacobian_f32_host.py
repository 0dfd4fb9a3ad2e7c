"""The opt-in fp32 reprojection Jacobian (VBA_OPT_JACOBIAN_F32) without a GPU: its closed form in vinsat_amd/csrc/vba_math.h
compiled for the host against the reference's fp64 Jacobian, the option's number in the C header and in the Python binding, and
the argument check of ``ba.configure``."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_inputs
from vinsat_amd import _lib

SRC = os.path.join(ROOT, "tests", "hostcheck", "hostcheck_f32.cpp")
LIB = os.path.join(ROOT, "tests", "hostcheck", "libhostcheck_f32.so")
P = ctypes.POINTER(ctypes.c_double)
PI = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def hc():
    hdr = os.path.join(ROOT, "vinsat_amd", "csrc", "vba_math.h")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


@pytest.mark.parametrize("k", [0, 10, 19])
def test_f32_jacobian_vs_reference(hc, c2, k):
    inp = golden_inputs(c2)
    st = np.ascontiguousarray(c2[f"states_in_{k}"][0])
    m = inp["xyz"].shape[0]
    terms = np.zeros((m, 10))
    J = np.zeros((m, 2, 6))
    hc.hc_jacobian_f32(ctypes.c_int64(m), st.ctypes.data_as(P), inp["K"].ctypes.data_as(P), inp["xyz"].ctypes.data_as(P),
                       inp["ii"].ctypes.data_as(PI), terms.ctypes.data_as(P), J.ctypes.data_as(P))
    # every camera-frame term is an fp32 number
    assert np.array_equal(terms.astype(np.float32).astype(np.float64), terms)
    # the world-frame rows: within 2^-20 of the reference's fp64 rows (norm of the row), and not its bits
    Jg = c2[f"Jg_{k}"][:, :, :6]
    row_err = np.linalg.norm(J - Jg, axis=2) / np.linalg.norm(Jg, axis=2)
    assert row_err.max() <= 2.0 ** -20, row_err.max()
    assert not np.array_equal(J, Jg)


def test_option_number_in_header_and_binding():
    with open(os.path.join(ROOT, "include", "vinsat_ba.h")) as f:
        hdr = f.read()
    m = re.search(r"VBA_OPT_JACOBIAN_F32\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 13
    assert _lib.OPT["jacobian_f32"] == 13


def test_configure_rejects_unknown_precision(monkeypatch):
    from vinsat_amd import ba, engine

    def no_device(*a, **k):
        raise AssertionError("configure touched a device")
    monkeypatch.setattr(engine.BAEngine, "__init__", no_device)
    monkeypatch.setattr(engine.BAEngine, "set_jacobian_f32", no_device)
    with pytest.raises(ValueError):
        ba.configure(jacobian="fp16")
