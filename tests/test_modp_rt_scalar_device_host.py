"""The host-side surface of the device scalar ring of a run-time MODP group: which handles hold the constants of q' = (q-1)/2
(mpvss_modp_group_has_device_scalar) and the new symbols with the header's signatures.  Through the library, no GPU."""
import os
import random
import re

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
from mpvss_rs_amd import EXPORTED_SYMBOLS, ModpGroup, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {
    "mpvss_modp_group_poly_eval_device":
        "int mpvss_modp_group_poly_eval_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* coeffs_host, size_t t, "
        "const int64_t* positions_dev, size_t n, uint8_t* out_dev);",
    "mpvss_modp_group_dleq_responses_device":
        "int mpvss_modp_group_dleq_responses_device(mpvss_ctx* ctx, const mpvss_modp_group* grp, const uint8_t* w_dev, "
        "const uint8_t* alpha_dev, const uint8_t* c_host, size_t n, uint8_t* r_dev_out);",
    "mpvss_modp_group_batch_scalar_mul":
        "int mpvss_modp_group_batch_scalar_mul(mpvss_ctx* ctx, const mpvss_modp_group* grp, int space, const uint8_t* a, "
        "const uint8_t* b, size_t n, uint8_t* out);",
    "mpvss_modp_group_has_device_scalar": "int mpvss_modp_group_has_device_scalar(const mpvss_modp_group* grp);",
    "mpvss_ctx_set_rt_scalar": "int mpvss_ctx_set_rt_scalar(mpvss_ctx* ctx, int mode);",
    "mpvss_modp_group_scalar_min_shares": "int mpvss_modp_group_scalar_min_shares(const mpvss_modp_group* grp);",
    "mpvss_modp_group_scalar_stats":
        "int mpvss_modp_group_scalar_stats(mpvss_ctx* ctx, unsigned long long* device_calls, unsigned long long* host_calls);",
}


def _norm(text):
    return re.sub(r"\s+", " ", text).strip()


def test_has_device_scalar_for_safe_primes_above_5():
    sp = H.small_safe_primes()
    for q in (7, 23, sp[40], sp[512], H.rfc_prime(1024), H.rfc_prime(2048)):
        assert ModpGroup(q).has_device_scalar is True, q.bit_length()
    assert ModpGroup(WH.group15(), elem_bytes=WH.EB).has_device_scalar is True


def test_no_device_scalar_when_the_half_order_is_even_or_too_small():
    assert ModpGroup(5).has_device_scalar is False                      # q' = 2
    rng = random.Random(1)
    seen = 0
    while seen < 3:
        q = H.random_odd_modulus(rng.choice((61, 300, 2048)), rng)
        if q % 4 == 1:                                                  # q' even
            assert ModpGroup(q).has_device_scalar is False
            seen += 1
    assert ModpGroup(H.random_odd_modulus(2048, random.Random(2)) | 3).has_device_scalar is True    # any q = 3 mod 4
    assert load_library().mpvss_modp_group_has_device_scalar(None) == -1


def test_scalar_min_shares_is_a_positive_size_for_every_width():
    sp = H.small_safe_primes()
    for grp in (ModpGroup(23), ModpGroup(H.rfc_prime(1024)), ModpGroup(H.rfc_prime(2048)), ModpGroup(WH.group15(), elem_bytes=WH.EB)):
        assert grp.scalar_min_shares >= 1
    assert load_library().mpvss_modp_group_scalar_min_shares(None) == -1


def test_new_symbols_exist_with_the_headers_signatures():
    lib = load_library()
    header = open(os.path.join(ROOT, "include", "mpvss_hip.h")).read()
    decls = _norm(re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert name in EXPORTED_SYMBOLS
        assert _norm(sig) in decls, name
