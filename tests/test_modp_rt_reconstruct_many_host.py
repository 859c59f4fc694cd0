"""CPU side of mpvss_modp_group_reconstruct_many: the entry points refuse a missing context without a GPU, the ctypes struct has
the header's layout, and the cases of tests/test_gpu_modp_rt_reconstruct_many.py (tests/modp_rt_reconstruct_many_cases.py) are held
to the oracle's ref_reconstruct at 40 bits -- with shares made by Python's pow -- so that the GPU module's expectations, which are
the one-secret call's bytes, do not rest on the engine alone."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import functools

import modp_rt_reconstruct_cases as K
import modp_rt_reconstruct_many_cases as MC


@functools.lru_cache(maxsize=None)
def builder(key):
    return K.RtBuilder(key)


def test_no_context_is_refused_without_a_gpu():
    from mpvss_rs_amd import capi
    lib = capi.load_library()
    arr, status = (capi.GroupSecret * 1)(), (C.c_int * 1)(5)
    gs = (C.c_uint8 * 256)(*([7] * 256))
    assert lib.mpvss_modp_group_reconstruct_many(None, None, 0, arr, 1, 0, status, gs, None) == -1
    assert status[0] == 5 and bytes(gs) == bytes([7]) * 256
    assert lib.mpvss_modp_group_reconstruct_many_stats(None, None, None, None) == -1


def test_the_struct_has_the_headers_layout():
    from mpvss_rs_amd import capi
    assert C.sizeof(capi.GroupSecret) == 24
    assert [(n, getattr(capi.GroupSecret, n).offset) for n, _ in capi.GroupSecret._fields_] == [("positions_host", 0), ("shares", 8), ("m", 16)]


def test_the_sizes_are_the_boundaries_of_a_fold_over_16_quads():
    assert MC.segment_sizes("rfc2048") == [1, 2, 3, 15, 16, 17, 31, 32, 33, 65]
    assert MC.segment_sizes("b40") == [1, 2, 3, 15, 16, 17, 31, 32, 33, 65, 255, 256, 257]
    assert {(m + 15) // 16 for m in MC.segment_sizes("b40")} == {1, 2, 3, 5, 16, 17}
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


def test_the_gpu_modules_cases_equal_the_reference_at_40_bits():
    b, memo = builder("b40"), {}
    cases = MC.segment_cases(b) + MC.small_cases(b, 64) + MC.sharing_cases(b) + MC.chunk_cases(b)
    for c in cases:
        assert c.expect[0] == "identity" and b.reference(c, memo) == b.expected(c), c.id
    shared = MC.sharing_cases(b)
    assert [c.positions for c in shared[:8]] == [shared[0].positions] * 8 and len({tuple(c.shares) for c in shared[:8]}) == 8
    assert sorted(shared[8].positions) == sorted(shared[0].positions) and shared[8].positions != shared[0].positions
    assert b.reference(shared[8], memo) == b.reference(shared[0], memo)
    assert len(shared[9].positions) == len(shared[0].positions) and set(shared[9].positions) != set(shared[0].positions)
    assert len({tuple(c.positions) for c in MC.small_cases(b, 64)}) == 12


def test_the_refused_cases_are_refused_by_the_reference():
    b, memo = builder("b40"), {}
    pairs = MC.refused_between_good(b)
    assert [r for _, r in pairs] == [False, True, False, True, False, True, False, True, False, True, False, False]
    for c, r in pairs:
        if not r:
            assert b.reference(c, memo) == b.expected(c), c.id
    bad = {c.id: c for c, r in pairs if r}
    assert bad["R-empty"].positions == [] and bad["R-null-shares"].shares is None
    assert min(bad["R-position-0"].positions) == 0
    assert len(set(bad["R-duplicate"].positions)) == 2
    zero = [c for c in bad.values() if c.id.endswith("zero-neg")][0]
    assert b.reference(zero, memo) is None                                  # a share 0 mod q under a negative coefficient
    assert sum(int.from_bytes(s, "big") % b.q == 0 for s in zero.shares) == 1
    lane = [int.from_bytes(s, "big") % b.q == 0 for s in zero.shares].index(True)
    assert K.lane_signs(zero.positions)[lane]


def test_the_q23_cases_are_what_the_reference_says():
    b, memo = builder("q23"), {}
    pairs = MC.tiny_refused_between_good(b, lambda c: b.reference(c, memo))
    assert [r for _, r in pairs] == [False, False, False, True, False, True, False, True, False]
    for c, r in pairs:
        assert (b.reference(c, memo) is None) == r, c.id
        if r:                                                               # no duplicates: the reduced denominator decides
            assert len(set(c.positions)) == len(c.positions) and K.raw_denominator_vanishes(c.positions, b.sub)
