"""The C ABI of the basis calls: the three symbols are exported by the built library with the declared signatures (the header's
prototypes, argument for argument), the ABI version says so, and their profile entries are appended behind the existing ids.  No GPU."""
import ctypes as C
import os
import re

import medgp_amd
from medgp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(arg):
    t = arg.rsplit(" ", 1)[0].replace("const ", "").strip() + ("*" if arg.rsplit(" ", 1)[1].startswith("*") else "")
    t = t.replace(" ", "")
    return {"medgp_ctx*": C.c_void_p, "int": C.c_int, "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double),
            "int64_t*": C.POINTER(C.c_int64), "float*": C.POINTER(C.c_float)}[t]


def test_basis_symbols_exported_with_declared_signatures(built_lib):
    lib = capi.load()
    assert lib.medgp_abi_version() >= 21
    raw = C.CDLL(built_lib)
    for name, nargs in (("medgp_set_basis", 6), ("medgp_basis_nlml_grad", 14), ("medgp_basis_posterior_batch", 15)):
        assert hasattr(raw, name), name
        assert name in capi.SYMBOLS
        args = _prototype(name)
        assert len(args) == nargs, (name, args)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [_ctype(a) for a in args], (name, args)
    # a NULL context is refused before anything is touched
    assert lib.medgp_set_basis(None, 1, None, 1, None, None) == -1
    assert lib.medgp_basis_nlml_grad(None, 1, None, None, 0, None, None, 1, None, None, None, None, None, None) == -1
    assert lib.medgp_basis_posterior_batch(None, 1, None, None, 0, None, None, None, None, None, None, None, None, None, None) == -1


def test_basis_profile_entries_are_appended(built_lib):
    lib = capi.load()
    n = lib.medgp_profile_num_kernels_ext()
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(n)]
    assert names[55:58] == ["k_basis_g", "k_basis_small", "k_basis_post"] and n == 58
    assert names[50:55] == ["k_mean_g", "k_mean_small", "k_mean_panel", "k_mean_wgrad", "k_mean_post"] and names[7] == "k_wgrad"
    assert lib.medgp_profile_num_kernels() == 23 and lib.medgp_profile_num_kernels_all() == 29
    assert all(hasattr(medgp_amd.Context, m) for m in ("set_basis", "basis_nlml_grad", "basis_posterior"))
