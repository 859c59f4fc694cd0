"""CPU side of mpvss_modp_group_verify_many: the entry points refuse a missing context without a GPU, and the power that
modp_rt_many_helpers.libcrypto_pow lends the oracle at 2048 and 3072 bits is Python's pow."""
import ctypes as C
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import mpvss_oracle as O
import modp_rt_many_helpers as M


@pytest.mark.parametrize("name", M.LARGE)
def test_libcrypto_power_is_pythons(name):
    import openssl_ref
    if not openssl_ref.available():                                         # no libcrypto: the oracle keeps Python's pow
        with M.libcrypto_pow(name):
            assert O.ModpGroup.exp.__qualname__ == "ModpGroup.exp"
        return
    q, eb = M.GROUPS[name][0](), M.GROUPS[name][1]
    rng = random.Random(int(name))
    top = (1 << (8 * eb)) - 1
    for base, e in [(0, 0), (0, 5), (1, top), (q - 1, q - 2), (q, 3), (q + 5, 1), (top, top), (4, 0)] + \
                   [(rng.randrange(q), rng.getrandbits(bits)) for bits in (1, 64, 256, 8 * eb)]:
        assert M.bn_mod_exp(base, e, q) == pow(base, e, q), (name, base, e)
    plain = O.ModpGroup.exp
    with M.libcrypto_pow(name):
        assert O.ModpGroup.exp is not plain
        box = M.dealt_box(name, 1, 1, 100)                                  # dealt and judged over libcrypto ...
        assert M.oracle_verdict(q, eb, box) is True
    assert O.ModpGroup.exp is plain
    assert M.dealt_box(name, 1, 1, 100) == box                              # ... and over Python's pow
    assert M.oracle_verdict(q, eb, box) is True and M.oracle_verdict(q, eb, M.tampered(box, eb, ("shares", 0))) is False
    with M.libcrypto_pow("1024"):
        assert O.ModpGroup.exp is plain                                     # the narrower groups never leave Python's pow


def test_the_boxes_of_a_small_group():
    c = M.case("40")
    assert [(len(b["positions"]), len(b["commitments"]) // 256) for b in c["mixed"]] == M.SHAPES
    assert all(c["mixed_valid"]) and all(c["run_valid"]) and not any(c["tampered_valid"])


def test_no_context_is_refused_without_a_gpu():
    from mpvss_rs_amd import capi
    lib = capi.load_library()
    arr, verdicts = (capi.GroupBox * 1)(), (C.c_int * 1)(5)
    assert C.sizeof(capi.GroupBox) == C.sizeof(capi.ModpBox)
    assert lib.mpvss_modp_group_verify_many(None, None, 0, arr, 1, 0, verdicts, None) == -1 and verdicts[0] == 5
    assert lib.mpvss_modp_group_verify_many_stats(None, None, None, None) == -1
