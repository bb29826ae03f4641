"""The C ABI of the warp calls: the two symbols are exported by the built library with the declared signatures (the header's
prototypes, argument for argument), the ABI version says so, and their profile entries stand behind a new counter while the three
older counters keep their values.  No GPU."""
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


def test_warp_symbols_exported_with_declared_signatures(built_lib):
    lib = capi.load()
    assert lib.medgp_abi_version() >= 22
    raw = C.CDLL(built_lib)
    for name, nargs in (("medgp_warp_nlml_grad", 12), ("medgp_warp_posterior_batch", 17)):
        assert hasattr(raw, name), name
        assert name in capi.SYMBOLS
        args = _prototype(name)
        assert len(args) == nargs, (name, args)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [_ctype(a) for a in args], (name, args)
    # a NULL context is refused before anything is touched
    assert lib.medgp_warp_nlml_grad(None, 1, None, None, None, None, 1, None, None, None, None, None) == -1
    assert lib.medgp_warp_posterior_batch(None, 1, None, None, None, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert (capi.WARP_NONE, capi.WARP_SAS) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"#define\s+MEDGP_WARP_NONE\s+0\b", hdr) and re.search(r"#define\s+MEDGP_WARP_SAS\s+1\b", hdr)


def test_warp_profile_entries_stand_behind_a_new_counter(built_lib):
    lib = capi.load()
    assert hasattr(C.CDLL(built_lib), "medgp_profile_num_kernels_ext2")
    n = lib.medgp_profile_num_kernels_ext2()
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(n)]
    assert n == 62 and names[58:62] == ["k_warp_z", "k_warp_solve", "k_warp_small", "k_warp_post"]
    assert names[55:58] == ["k_basis_g", "k_basis_small", "k_basis_post"] and names[7] == "k_wgrad"
    assert lib.medgp_profile_num_kernels() == 23 and lib.medgp_profile_num_kernels_all() == 29 and lib.medgp_profile_num_kernels_ext() == 58
    assert lib.medgp_profile_kernel_name(62).decode() == ""
    assert lib.medgp_profile_read(None, 58, None, None) == -1
    assert all(hasattr(medgp_amd.Context, m) for m in ("warp_nlml_grad", "warp_posterior"))
