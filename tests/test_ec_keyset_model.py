"""The build and walk bodies of the curve groups' key sets (csrc/ec_keyset.h) compiled for the CPU (tests/ec_keyset_host_shim.cpp)
against the plain-C reference (oracle/ec_ref.c): every row entry is (i + 1) 16^w y, and the walk over the rows is k y at the edges
of the signed 4-bit recoding.  Keys: G, the identity, -G and five random multiples, on both curves."""
import ctypes as C

import pytest

import ec_dual_cases as D
import ec_keyset_cases as K


@pytest.fixture(scope="module", params=D.NAMES)
def kc(request):
    return K.cases(request.param)


@pytest.fixture(scope="module")
def rows(kc):
    """[(row words, ok, mark)] of the keys under test, built once"""
    so = K.shim()
    words = so.ks_row_words(kc.gid)
    assert words * 4 == K.ROW_BYTES[kc.name]
    out = []
    for key in kc.keys:
        row = (C.c_uint32 * words)()
        ok, mark = C.c_uint8(7), C.c_uint8(7)
        so.ks_build(kc.gid, (C.c_uint8 * kc.L).from_buffer_copy(key), row, C.byref(ok), C.byref(mark))
        out.append((row, ok.value, mark.value))
    return out


def test_marks_and_validity(kc, rows):
    assert [ok for _, ok, _ in rows] == [1] * len(kc.keys)
    assert [mark for _, _, mark in rows] == [1 if key == kc.cs.ident else 0 for key in kc.keys]


def test_every_row_entry_is_its_multiple_of_the_key(kc, rows):
    so = K.shim()
    ew = so.ks_entry_words(kc.gid)
    assert ew * 4 * K.WINDOWS * K.ENTRIES == K.ROW_BYTES[kc.name]
    out = (C.c_uint8 * kc.L)()
    for key, (row, _, mark) in zip(kc.keys, rows):
        if mark:
            continue          # a marked key's rows are never read (the walk test below holds the identity to its rule)
        for w in range(K.WINDOWS):
            for i in range(K.ENTRIES):
                entry = (C.c_uint32 * ew).from_buffer(row, 4 * ew * (w * K.ENTRIES + i))
                assert so.ks_entry_encode(kc.gid, entry, out) == 0, "entry (%d, %d) is not a consistent affine form" % (w, i)
                want = kc.mul(key, K.entry_scalar(kc.order, w, i))
                assert bytes(out) == want, "%s key %s: entry (%d, %d)" % (kc.name, key.hex(), w, i)


def test_packed_entries_are_canonical(kc, rows):
    """coordinates below the field prime: the packing is the generator comb's"""
    so = K.shim()
    ew = so.ks_entry_words(kc.gid)
    p = 2**256 - 2**32 - 977 if kc.name == "secp256k1" else 2**255 - 19
    for row, _, _ in rows:
        raw = bytes(row)
        for off in range(0, len(raw), 32):
            assert int.from_bytes(raw[off:off + 32], "little") < p
    assert ew in (16, 24)


def test_walk_is_k_times_the_key(kc, rows):
    so = K.shim()
    out = (C.c_uint8 * kc.L)()
    assert len(kc.edge) >= 8 + 4 * len(D.EXTREME_WINDOWS) - len(kc.unreachable)
    if kc.name == "secp256k1":
        assert not kc.unreachable and len(kc.top) >= 3
    for key, (row, _, mark) in zip(kc.keys, rows):
        for k in kc.edge:
            so.ks_walk(kc.gid, row, mark, (C.c_uint8 * 32).from_buffer_copy(kc.scalar(k)), out)
            assert bytes(out) == kc.mul(key, k), "%s key %s: k = %#x" % (kc.name, key.hex(), k)
