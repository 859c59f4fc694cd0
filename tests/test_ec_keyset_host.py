"""The host-side contracts of the key sets of a curve group (include/mpvss_hip.h, "Key sets of a curve group"): the symbols and
their prototypes, the size of a key's rows, and the null-pointer rules.  Through the library, no GPU."""
import ctypes as C
import os
import re

from mpvss_rs_amd import EXPORTED_SYMBOLS, capi, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPVSS_E_INVALID = -1
MARK_BYTES = 1           # the documented per-key flag: one identity mark

# name -> (return type, parameter types) as include/mpvss_hip.h declares them
PROTOTYPES = {
    "mpvss_ec_keyset_bytes_per_key": ("size_t", ["int"]),
    "mpvss_ec_keyset_create": ("int", ["mpvss_ctx*", "int", "int", "const uint8_t*", "size_t", "mpvss_ec_keyset**"]),
    "mpvss_ec_keyset_destroy": ("void", ["mpvss_ctx*", "mpvss_ec_keyset*"]),
    "mpvss_ec_keyset_bytes": ("size_t", ["const mpvss_ec_keyset*"]),
    "mpvss_ec_keyset_twin_exp": ("int", ["mpvss_ctx*", "int", "int", "const mpvss_ec_keyset*", "size_t", "const uint8_t*",
                                         "const uint8_t*", "size_t", "uint8_t*", "uint8_t*"]),
    "mpvss_ec_keyset_dual_exp": ("int", ["mpvss_ctx*", "int", "int", "const mpvss_ec_keyset*", "size_t", "const uint8_t*",
                                         "const uint8_t*", "const uint8_t*", "int", "size_t", "uint8_t*"]),
    "mpvss_ec_deal_compute_keyset": ("int", ["mpvss_ctx*", "int", "const uint8_t*", "size_t", "const int64_t*",
                                             "const mpvss_ec_keyset*", "size_t", "const uint8_t*", "size_t"] + ["uint8_t*"] * 5),
    "mpvss_ec_deal_keyset": ("int", ["mpvss_ctx*", "int", "const uint8_t*", "size_t", "const int64_t*", "const mpvss_ec_keyset*",
                                     "size_t", "const uint8_t*", "size_t"] + ["uint8_t*"] * 7),
    "mpvss_ec_keyset_stats": ("int", ["mpvss_ctx*", "unsigned long long*", "unsigned long long*"]),
}


def declared():
    """{function: (return type, [parameter type])} of the header, comments removed"""
    text = open(os.path.join(ROOT, "include", "mpvss_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int|void|size_t)\s+(mpvss_ec_\w*keyset\w*)\s*\(([^)]*)\)\s*;", text):
        types = []
        for p in params.split(","):
            p = " ".join(p.split())
            types.append(re.sub(r"\s*\b\w+$", "", p) if not p.endswith("*") else p)      # drop the parameter's name
        out[name] = (ret, [t.replace(" *", "*") for t in types])
    return out


def test_the_header_declares_the_new_symbols_with_these_prototypes():
    assert declared() == PROTOTYPES


def test_the_library_and_the_binding_carry_them():
    lib = load_library()
    restype = {"int": C.c_int, "void": None, "size_t": C.c_size_t}
    for name, (ret, params) in PROTOTYPES.items():
        assert name in EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params), name
        assert fn.restype == restype[ret], name
        for at, ct in zip(fn.argtypes, params):
            want = {"int": C.c_int, "size_t": C.c_size_t}.get(ct)
            if want is not None:
                assert at is want, (name, ct)
            elif ct.startswith("unsigned long long"):
                assert at is C.POINTER(C.c_ulonglong), (name, ct)
            else:
                assert at in (C.c_void_p, C.POINTER(C.c_void_p)), (name, ct)


def test_bytes_per_key_is_65_windows_of_8_packed_entries_and_a_mark():
    lib = load_library()
    assert lib.mpvss_ec_keyset_bytes_per_key(capi.GROUP_SECP256K1) == 33280 + MARK_BYTES == 65 * 8 * 64 + MARK_BYTES
    assert lib.mpvss_ec_keyset_bytes_per_key(capi.GROUP_RISTRETTO255) == 49920 + MARK_BYTES == 65 * 8 * 96 + MARK_BYTES
    for unknown in (0, 3, -1, 99):
        assert lib.mpvss_ec_keyset_bytes_per_key(unknown) == 0


def test_no_set_has_no_bytes_and_destroys_to_nothing():
    lib = load_library()
    assert lib.mpvss_ec_keyset_bytes(None) == 0
    assert lib.mpvss_ec_keyset_destroy(None, None) is None


def test_a_null_context_is_invalid():
    lib = load_library()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    pos = C.cast((C.c_int64 * 1)(1), C.c_void_p)
    for group in (capi.GROUP_SECP256K1, capi.GROUP_RISTRETTO255):
        out = C.c_void_p(1)
        assert lib.mpvss_ec_keyset_create(None, group, 0, p, 1, C.byref(out)) == MPVSS_E_INVALID
        assert out.value is None                     # cleared even on this way out
        assert lib.mpvss_ec_keyset_twin_exp(None, group, 0, None, 0, p, p, 1, p, p) == MPVSS_E_INVALID
        assert lib.mpvss_ec_keyset_dual_exp(None, group, 0, None, 0, p, None, None, 0, 1, p) == MPVSS_E_INVALID
        assert lib.mpvss_ec_deal_compute_keyset(None, group, p, 1, pos, None, 0, p, 1, p, None, None, None, None) == MPVSS_E_INVALID
        assert lib.mpvss_ec_deal_keyset(None, group, p, 1, pos, None, 0, p, 1, None, p, None, None, None, None, p) == MPVSS_E_INVALID
    assert lib.mpvss_ec_keyset_stats(None, None, None) == MPVSS_E_INVALID
