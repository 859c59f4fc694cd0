"""CPU side of mpvss_ec_reconstruct_many: the library exports the call and refuses a missing context without a GPU, the ctypes
struct has the header's layout, and the cases of tests/test_gpu_ec_reconstruct_many.py (tests/ec_reconstruct_many_cases.py) are
held to the oracle's ref_reconstruct -- with shares made by the oracle -- for every secret of at most 65 shares, so that the GPU
module's expectations do not rest on the engine alone."""
import ctypes as C
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import ec_reconstruct_many_cases as MC
import reconstruct_cases as K

GID = {"secp256k1": 1, "ristretto255": 2}


@functools.lru_cache(maxsize=None)
def builder(name):
    return K.Builder(name)


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------
def test_the_library_exports_both_symbols():
    from mpvss_rs_amd import capi
    lib = capi.load_library()
    for sym in ("mpvss_ec_reconstruct_many", "mpvss_ec_reconstruct_many_stats"):
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym), sym


@pytest.mark.parametrize("name", K.CURVES)
def test_no_context_is_refused_and_writes_nothing(name):
    from mpvss_rs_amd import capi
    lib = capi.load_library()
    L = capi.EC_ENC[GID[name]]
    pos = (C.c_int64 * 3)(1, 2, 3)
    shares = (C.c_uint8 * (3 * L))()
    arr = (capi.EcSecret * 1)(capi.EcSecret(C.cast(pos, C.c_void_p), C.cast(shares, C.c_void_p), 3))
    status = (C.c_int * 1)(5)
    gs, masks = (C.c_uint8 * L)(*([7] * L)), (C.c_uint8 * 32)(*([9] * 32))
    rc = lib.mpvss_ec_reconstruct_many(None, GID[name], capi.MPVSS_HOST, arr, 1, 0, status, C.cast(gs, C.c_void_p), C.cast(masks, C.c_void_p))
    assert rc == -1
    assert status[0] == 5 and bytes(gs) == bytes([7]) * L and bytes(masks) == bytes([9]) * 32
    p, g, s = C.c_ulonglong(11), C.c_ulonglong(12), C.c_ulonglong(13)
    assert lib.mpvss_ec_reconstruct_many_stats(None, C.byref(p), C.byref(g), C.byref(s)) == -1
    assert (p.value, g.value, s.value) == (11, 12, 13)
    assert lib.mpvss_ec_reconstruct_many_stats(None, None, None, None) == -1


def test_the_struct_has_the_headers_layout():
    from mpvss_rs_amd import capi
    assert C.sizeof(capi.EcSecret) == 24
    assert [(n, getattr(capi.EcSecret, n).offset) for n, _ in capi.EcSecret._fields_] == [("positions_host", 0), ("shares", 8), ("m", 16)]


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_the_sizes_are_the_boundaries_of_a_sum_by_one_wave():
    assert MC.SEGMENT_M == [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
    assert all(a != b for a, b in zip(MC.SEGMENT_M, MC.SEGMENT_M[1:]))          # neighbours differ: a read past m changes a sum
    assert {(m + 63) // 64 for m in MC.SEGMENT_M} == {1, 2, 3, 5}               # trips of the stride loop
    # where the tree starts: the smallest power of two not below min(m, 64)
    assert {1 << (min(m, 64) - 1).bit_length() for m in MC.SEGMENT_M} == {1, 2, 4, 32, 64}
    assert MC.SECRET_COUNTS == [1, 2, 9, 65, 513]
    assert all(m <= MC.CHUNK or m == 33 for m in MC.CHUNK_M)
    # the grouping rule on CHUNK_M: passes of at most CHUNK shares cut at secret boundaries, a pass of one and m > CHUNK single
    passes, single, run = [], [], []
    for m in MC.CHUNK_M + [None]:
        if m is None or m > MC.CHUNK or sum(run) + m > MC.CHUNK:
            (passes if len(run) > 1 else single).extend([run] if len(run) > 1 else run)
            run = []
        if m is not None:
            if m > MC.CHUNK:
                single.append(m)
            else:
                run.append(m)
    assert passes == [[16, 16], [3, 5], [20, 7]] and sorted(single) == [17, 33]
    assert MC.CHUNK_STATS == {"passes": len(passes), "grouped_secrets": sum(map(len, passes)), "single_secrets": len(single)}


@pytest.mark.parametrize("name", K.CURVES)
def test_cases_equal_the_reference(name):
    """every good case of at most 65 shares: the closed form G^P(0) is what ref_reconstruct folds from the oracle's shares"""
    b = builder(name)
    G, memo = b.G, {}
    cases = [c for c in MC.segment_cases(b) if len(c.positions) <= 65]
    assert [len(c.positions) for c in cases] == [1, 2, 3, 31, 32, 33, 63, 64, 65]
    cases += MC.small_cases(b, 12) + MC.sharing_cases(b) + MC.chunk_cases(b)
    cases += [c for c, refused in MC.refused_between_good(b) if not refused]
    for c in cases:
        got = K.ref_reconstruct(G, c.positions, b.elements(c), memo)
        assert got is not K.REFUSED and G.element_to_fixed(got) == b.expected(c), c.id
    for c in MC.sign_and_degenerate_cases(b):
        assert len(c.positions) in (5, 17) and c.expect[0] == "ref", c.id
        assert b.expected(c, memo) is not None, c.id                              # (held to O.reconstruct by test_reconstruct_cases.py)
    assert len({tuple(c.positions) for c in MC.small_cases(b, 12)}) == 12


@pytest.mark.parametrize("name", K.CURVES)
def test_sharing_and_refusals_are_what_they_say(name):
    b = builder(name)
    sh = MC.sharing_cases(b)
    assert all(c.positions == sh[0].positions for c in sh[:8])
    assert sorted(sh[8].positions) == sorted(sh[0].positions) and sh[8].positions != sh[0].positions
    assert b.expected(sh[8]) == b.expected(sh[0]) and sh[9].positions != sh[0].positions
    pairs = MC.refused_between_good(b)
    assert [r for _, r in pairs] == [False, True, False, True, False, True, False, True, False, True, False, False]
    bad = {c.id: c for c, r in pairs if r}
    assert bad["R-empty"].positions == [] and bad["R-null-shares"].shares is None
    assert 0 in bad["R-position-0"].positions and len(set(bad["R-duplicate"].positions)) == 2
    enc = bad["R-encoding"]
    assert len(enc.shares) == 3
    for k, s in enumerate(enc.shares):
        if k == 1:
            with pytest.raises(ValueError):
                b.G.element_from_fixed(s)                                         # the oracle's decoder rejects the middle share
        else:
            b.G.element_from_fixed(s)
    lanes = MC.lane_cases(b)
    assert [c.shares.index(b.identity_enc()) for c in lanes] == [0, 63, 64, 255, 256]
    # the closed form that the GPU module holds those five to, against the reference at m = 9 (the same builder code, fewer shares)
    for lane in (0, 4, 8):
        nine = b.shape_case(9)
        shares = list(nine.shares)
        shares[lane] = b.identity_enc()
        got = K.ref_reconstruct(b.G, nine.positions, [b.G.element_from_fixed(s) for s in shares])
        assert b.G.element_to_fixed(got) == MC.identity_lane_expected(b, 9, lane) != b.expected(nine)
