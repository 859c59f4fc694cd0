"""The reference of tests/ec_lagrange_cases.py held to reconstruct_cases.exact_lagrange (fractions over Python integers, written
for another purpose) and to the polynomial identity sum lambda_i P(x_i) = P(0); the case list held to the kernel's edges; and the
three new symbols of the ABI without a GPU.  No engine, no GPU."""
import ctypes as C
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import ec_lagrange_cases as LC
import reconstruct_cases as K

GID = {"secp256k1": 1, "ristretto255": 2}
SYMBOLS = ("mpvss_ctx_set_ec_lagrange", "mpvss_ec_lagrange_scalars", "mpvss_ec_lagrange_stats")


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------
def test_the_library_exports_the_three_symbols():
    from mpvss_rs_amd import capi
    lib = capi.load_library()
    for sym in SYMBOLS:
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym


@pytest.mark.parametrize("name", LC.CURVES)
def test_no_context_is_refused_and_writes_nothing(name):
    from mpvss_rs_amd import capi
    lib = capi.load_library()
    pos = (C.c_int64 * 3)(1, 2, 3)
    out = (C.c_uint8 * 96)(*([0xA5] * 96))
    assert lib.mpvss_ec_lagrange_scalars(None, GID[name], C.cast(pos, C.c_void_p), 3, C.cast(out, C.c_void_p)) == -1
    assert bytes(out) == b"\xa5" * 96
    for mode in (0, 1, 2, 3):
        assert lib.mpvss_ctx_set_ec_lagrange(None, mode) == -1
    d, h = C.c_ulonglong(11), C.c_ulonglong(12)
    assert lib.mpvss_ec_lagrange_stats(None, C.byref(d), C.byref(h)) == -1
    assert (d.value, h.value) == (11, 12)
    assert lib.mpvss_ec_lagrange_stats(None, None, None) == -1


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_the_sizes_are_the_kernels_edges():
    assert (LC.WG, LC.STAGE) == (64, 256)
    assert LC.SIZES == [1, 2, 3, 63, 64, 65, 255, 256, 257, 513]
    assert {(m + LC.WG - 1) // LC.WG for m in LC.SIZES} == {1, 2, 4, 5, 9}             # workgroups of a list
    assert {(m + LC.STAGE - 1) // LC.STAGE for m in LC.SIZES} == {1, 2, 3}             # staging trips
    assert LC.BIG_M == K.SHAPE_M_BIG[1] == 4097
    csrc = os.path.join(HERE, "..", "mpvss_rs_amd", "csrc", "ec_lagrange.h")
    text = open(csrc).read()
    assert "constexpr int LAGRANGE_WG = 64;" in text and "constexpr int LAGRANGE_STAGE = 256;" in text


def test_the_case_list():
    cases = LC.cases()
    assert len(cases) == 3 * len(LC.SIZES) + 3 * len(LC.SPECIAL_M) and len({cid for cid, _ in cases}) == len(cases)
    for cid, xs in cases:
        assert len(set(xs)) == len(xs) and min(xs) >= 1 and max(xs) < 2 ** 63, cid
    by = dict(cases)
    for m in LC.SIZES:
        assert by[f"shuffled-{m}"] == K.Builder("secp256k1", power=lambda e: [b""] * len(e)).shape_positions(m)
        assert by[f"asc-{m}"] == by[f"desc-{m}"][::-1] == list(range(1, m + 1))
    for m in LC.SPECIAL_M:
        assert set(K.SPECIAL[:m]) <= set(by[f"special-{m}-asc"])
        assert sorted(by[f"special-{m}-shuffled"]) == by[f"special-{m}-asc"] == by[f"special-{m}-desc"][::-1]
    # both parities of the sign in every ascending list of two or more: lambda_0 > 0 > lambda_1
    for m in LC.SIZES[1:]:
        signs = K.lane_signs(by[f"asc-{m}"])
        assert signs[0] is False and signs[1] is True


@pytest.mark.parametrize("name", LC.CURVES)
def test_expected_is_the_exact_coefficient_reduced(name):
    n = LC.ORDER[name]
    assert n == K.O.GROUPS[name]().group_order_int()
    for cid, xs in LC.cases():
        want = [f.numerator * pow(f.denominator, -1, n) % n for f in K.exact_lagrange(xs)]
        assert LC.expected_ints(name, xs) == want, cid
        raw = LC.expected_of(name, cid, xs)
        assert len(raw) == 32 * len(xs)
        assert [int.from_bytes(raw[k:k + 32], LC.BYTE_ORDER[name]) for k in range(0, len(raw), 32)] == want, cid
    assert LC.expected(name, [7]) == (1).to_bytes(32, LC.BYTE_ORDER[name])             # m = 1: lambda = 1


@pytest.mark.parametrize("name", LC.CURVES)
def test_the_coefficients_interpolate_at_zero(name):
    """sum lambda_i P(x_i) = P(0) mod the order, for a seeded polynomial of min(m, 8) coefficients"""
    n = LC.ORDER[name]
    for cid, xs in LC.cases():
        rng = random.Random(len(xs))
        coeffs = [rng.randrange(n) for _ in range(min(len(xs), 8))]

        def P(x):
            acc = 0
            for a in reversed(coeffs):
                acc = (acc * x + a) % n
            return acc

        assert sum(l * P(x) for l, x in zip(LC.expected_ints(name, xs), xs)) % n == coeffs[0], cid
