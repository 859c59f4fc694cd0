"""The host-side contracts of the key sets of a run-time MODP group (include/mpvss_hip.h, "Key sets of a run-time group"): the
symbols, the size of a key's rows at every width, and the null-pointer rules.  Through the library, no GPU."""
import ctypes as C

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
from mpvss_rs_amd import EXPORTED_SYMBOLS, ModpGroup, load_library

MPVSS_E_INVALID = -1

NEW = ("mpvss_modp_group_keyset_bytes_per_key", "mpvss_modp_group_keyset_create", "mpvss_modp_group_keyset_destroy",
       "mpvss_modp_group_keyset_bytes", "mpvss_modp_group_keyset_dual_exp", "mpvss_modp_group_keyset_twin_exp",
       "mpvss_modp_group_verify_distribution_keyset", "mpvss_modp_group_deal_keyset")


def test_the_library_exports_the_new_symbols():
    lib = load_library()
    for name in NEW:
        assert name in EXPORTED_SYMBOLS
        assert hasattr(lib, name), name


def groups():
    sp = H.small_safe_primes()
    return [(40, ModpGroup(sp[40]), 5, 256), (256, ModpGroup(sp[256]), 5, 256), (1024, ModpGroup(H.rfc_prime(1024)), 9, 256),
            (1536, ModpGroup(H.rfc_prime(1536)), 18, 256), (2048, ModpGroup(H.rfc_prime(2048)), 18, 256),
            (3072, ModpGroup(WH.group15(), elem_bytes=WH.EB), 27, 384)]


def test_bytes_per_key_is_J_rows_of_16_numbers():
    lib = load_library()
    figures = {}
    for bits, grp, lpl, eb in groups():
        assert (grp.limbs_per_lane, grp.elem_bytes) == (lpl, eb)
        J, L = eb // 32, 4 * lpl
        assert lib.mpvss_modp_group_keyset_bytes_per_key(grp.handle) == J * 16 * L * 4 == grp.keyset_bytes_per_key, bits
        figures[lpl] = grp.keyset_bytes_per_key
    assert figures == {5: 10240, 9: 18432, 18: 36864, 27: 82944}
    assert lib.mpvss_modp_group_keyset_bytes_per_key(None) == 0


def test_no_set_has_no_bytes_and_destroys_to_nothing():
    lib = load_library()
    assert lib.mpvss_modp_group_keyset_bytes(None) == 0
    assert lib.mpvss_modp_group_keyset_destroy(None, None) is None


@pytest.mark.parametrize("with_group", [False, True], ids=["no group", "a group"])
def test_a_null_context_is_invalid(with_group):
    """no context (and no group): MPVSS_E_INVALID before anything is touched.  A null group under a live context is refused in
    tests/test_gpu_modp_rt_keyset.py."""
    lib = load_library()
    grp = ModpGroup(H.rfc_prime(1024)).handle if with_group else None
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    out = C.c_void_p(1)
    verdict = C.c_int(7)
    pos = C.cast((C.c_int64 * 1)(1), C.c_void_p)
    assert lib.mpvss_modp_group_keyset_create(None, grp, 0, p, 1, C.byref(out)) == MPVSS_E_INVALID
    assert out.value is None                     # cleared even on this way out
    assert lib.mpvss_modp_group_keyset_dual_exp(None, grp, 0, None, 0, p, None, None, 0, 1, p) == MPVSS_E_INVALID
    assert lib.mpvss_modp_group_keyset_twin_exp(None, grp, 0, None, 0, p, p, 1, p, p) == MPVSS_E_INVALID
    assert lib.mpvss_modp_group_verify_distribution_keyset(None, grp, 0, p, 1, pos, None, 0, p, p, 1, p, C.byref(verdict), None,
                                                           None, None, None) == MPVSS_E_INVALID
    assert lib.mpvss_modp_group_deal_keyset(None, grp, p, 1, pos, None, 0, p, 1, None, p, None, None, None, None, p) == MPVSS_E_INVALID
