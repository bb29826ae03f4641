"""The C ABI of the heteroscedastic calls: the four symbols are exported by the built library with the declared signatures (the header's
prototypes, argument for argument), the ABI version says so, a NULL context is refused, and their profile entries stand behind a new
counter and a name call of their own while the four older counters and medgp_profile_kernel_name keep their values.  No GPU."""
import ctypes as C
import os
import re

import medgp_amd
from medgp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = (("medgp_set_noise_scale", 5), ("medgp_hetero_nlml_grad", 10), ("medgp_hetero_posterior_batch", 11), ("medgp_robust_nlml_grad", 15))


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


def test_hetero_symbols_exported_with_declared_signatures(built_lib):
    lib = capi.load()
    assert lib.medgp_abi_version() >= 23
    raw = C.CDLL(built_lib)
    for name, nargs in CALLS:
        assert hasattr(raw, name), name
        assert name in capi.SYMBOLS
        args = _prototype(name)
        assert len(args) == nargs, (name, args)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [_ctype(a) for a in args], (name, args)
    # a NULL context is refused before anything is touched
    assert lib.medgp_set_noise_scale(None, 1, None, None, None) == -1
    assert lib.medgp_hetero_nlml_grad(None, 1, None, None, 1, None, None, None, None, None) == -1
    assert lib.medgp_hetero_posterior_batch(None, 1, None, None, None, None, None, None, None, None, None) == -1
    assert lib.medgp_robust_nlml_grad(None, 1, None, None, None, 0, None, 1, None, None, None, None, None, None, None) == -1
    assert all(hasattr(medgp_amd.Context, m) for m in ("set_noise_scale", "hetero_nlml_grad", "hetero_posterior", "robust_nlml_grad"))
    # the header states that every other call ignores the tables
    hdr = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert "EVERY OTHER CALL IGNORES THEM" in hdr


def test_hetero_profile_entries_stand_behind_a_new_counter(built_lib):
    lib = capi.load()
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "medgp_profile_num_kernels_ext3") and hasattr(raw, "medgp_profile_kernel_name_ext3")
    n = lib.medgp_profile_num_kernels_ext3()
    names = [lib.medgp_profile_kernel_name_ext3(k).decode() for k in range(n)]
    assert n == 67 and names[62:] == ["k_het_load", "k_het_rows", "k_het_estep", "k_het_obj", "k_het_post"]
    assert names[58:62] == ["k_warp_z", "k_warp_solve", "k_warp_small", "k_warp_post"] and names[7] == "k_wgrad"
    assert names[:62] == [lib.medgp_profile_kernel_name(k).decode() for k in range(62)]
    # the older counters and the older name call keep their values
    assert (lib.medgp_profile_num_kernels(), lib.medgp_profile_num_kernels_all(), lib.medgp_profile_num_kernels_ext(),
            lib.medgp_profile_num_kernels_ext2()) == (23, 29, 58, 62)
    assert lib.medgp_profile_kernel_name(62).decode() == "" and lib.medgp_profile_kernel_name_ext3(67).decode() == ""
    assert lib.medgp_profile_read(None, 62, None, None) == -1
