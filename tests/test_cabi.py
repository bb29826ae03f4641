"""The C-ABI library builds for gfx950, loads, and exports every symbol include/medgp_hip.h declares.
No compute calls (there is no GPU here); the product must fail loudly, not fall back, without a device."""
import ctypes as C
import os
import re

import pytest

import medgp_amd
from medgp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(medgp_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_all_exported(built_lib):
    lib = C.CDLL(built_lib)
    names = _declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/medgp_hip.h but not exported"
    assert sorted(capi.SYMBOLS) == names, "medgp_amd.capi.SYMBOLS out of sync with the header"


def test_library_is_gfx950_code_object(built_lib):
    blob = open(built_lib, "rb").read()
    assert b"gfx950" in blob
    assert b"k_cholinv" in blob and b"k_wgrad" in blob and b"k_la_step" in blob
    # the first-generation dense kernels left the tree in round 4
    assert b"k_potrf" not in blob and b"k_ci_panel" not in blob


def test_no_cpu_fallback_without_device(built_lib):
    lib = capi.load()
    assert lib.medgp_abi_version() >= 1
    if lib.medgp_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.MedgpError) as e:
        medgp_amd.Context(7, 5, 2, 2)
    assert "no HIP device" in str(e.value) or "-3" in str(e.value)


def test_product_never_imports_oracle():
    """The shipped package must not reach into oracle/ (the checker)."""
    pkg = os.path.join(ROOT, "medgp_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".h", ".hip", ".cpp", ".hpp", "Makefile")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                assert "medgp_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, os.path.join(dp, fn)
