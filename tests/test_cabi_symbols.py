"""The C-ABI library must load without a GPU and export every symbol include/vinsat_ba.h declares, and the ctypes
prototype table must cover exactly that set (no compute calls here)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "vinsat_ba.h")


@pytest.fixture(scope="module")
def lib_path():
    path = os.path.join(ROOT, "vinsat_amd", "libvinsat_ba.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "vinsat_amd", "csrc"), "-j4"])
    return path


def declared_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(vba_[a-z0-9_]+)\s*\(", txt)))


def test_every_declared_symbol_is_exported(lib_path):
    lib = ctypes.CDLL(lib_path)
    names = declared_functions()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), f"{name} declared in vinsat_ba.h but not exported"


def test_ctypes_table_matches_header(lib_path):
    from vinsat_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_functions()
    lib = _lib.load()
    assert lib.vba_version() >= 100
    assert lib.vba_sh_partial_count(10) == 272


def test_no_gpu_is_reported_not_hidden(lib_path):
    """Without a device the library must fail loudly (there is no CPU fallback)."""
    from vinsat_amd import _lib
    lib = _lib.load()
    cnt = ctypes.c_int(-1)
    assert lib.vba_device_count(ctypes.byref(cnt)) == 0
    if cnt.value == 0:
        h = ctypes.c_void_p()
        rc = lib.vba_create(0, 1, 16, 256, ctypes.byref(h))
        assert rc != 0 and not h.value
        assert b"device" in lib.vba_last_error().lower()
        from vinsat_amd.engine import BAEngine
        with pytest.raises(_lib.VbaError):
            BAEngine(16, 256)


EINVAL = 1


@pytest.mark.parametrize("windows,n_max,m_max,mode", [(0, 8, 300, -1), (1, 1, 300, -1), (1, 8, 0, -1), (1, 8, 2**30 + 1, -1),
                                                      (1, 8, 300, 2), (1, 8, 300, -2)])
def test_create_refuses_bad_arguments_before_it_looks_for_a_device(lib_path, windows, n_max, m_max, mode):
    """The argument checks of vba_create_mode precede the device count: the same answer with and without a GPU, *out left null."""
    from vinsat_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p(1)
    assert lib.vba_create_mode(0, windows, n_max, m_max, mode, ctypes.byref(h)) == EINVAL
    assert not h.value


def test_create_refuses_a_null_out(lib_path):
    from vinsat_amd import _lib
    assert _lib.load().vba_create_mode(0, 1, 8, 300, -1, None) == EINVAL


def test_every_setter_refuses_a_null_handle(lib_path):
    from vinsat_amd import _lib
    lib = _lib.load()
    for name, opt in _lib.OPT.items():
        assert lib.vba_set_option(None, opt, 0) == EINVAL, name
    assert lib.vba_set_solver(None, -1) == EINVAL
    assert lib.vba_set_solver2(None, 8, 0) == EINVAL
    assert lib.vba_set_integrator(None, 0) == EINVAL
    assert lib.vba_set_stream(None, None, 0) == EINVAL
    assert lib.vba_set_prior(None, 0) == EINVAL
    assert lib.vba_set_host_watch(None, 0, None, None, 0) == EINVAL


def test_one_hip_runtime_in_the_process_whichever_is_imported_first():
    """The wheel of PyTorch bundles its own HIP runtime; the library binds to that copy (vinsat_amd/_lib.py), so that a
    process that calls BA() on numpy arrays first and touches torch.cuda later does not end up with two ROCr instances
    (the second one cannot open the device)."""
    import subprocess, sys
    code = ("from vinsat_amd import _lib; _lib.load(); import torch; "
            "maps = {l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}; print(len(maps))")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "1"
