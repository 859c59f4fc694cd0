"""CPU side of the per-share DLEQ hash of a run-time MODP group on the device: the admission of a handle
(mpvss_modp_group_has_device_share_hash: (q-1)/2 >= 2^256, i.e. at least 258 bits) at its edge, and the case generator
tests/modp_rt_share_hash_cases.py held to what its docstring claims.  No GPU: the handle is host-only."""
import pytest

import modp_rt_helpers as H
import modp_rt_share_hash_cases as SH
import modp_rt_wide_helpers as WH
import mpvss_oracle as O
from mpvss_rs_amd import ModpGroup


def test_has_device_share_hash_at_its_edge():
    """odd moduli, not primes: 2^257 - 1 has (q-1)/2 = 2^256 - 1, one short; 2^257 + 1 has exactly 2^256"""
    assert ModpGroup(2 ** 257 - 1).has_device_share_hash is False
    assert ModpGroup(2 ** 257 + 1).has_device_share_hash is True
    small = H.small_safe_primes()
    assert ModpGroup(small[64]).has_device_share_hash is False
    assert ModpGroup(small[256]).has_device_share_hash is False
    assert ModpGroup(small[512]).has_device_share_hash is True
    assert ModpGroup(H.rfc_prime(1024)).has_device_share_hash is True
    assert ModpGroup(H.rfc_prime(2048)).has_device_share_hash is True
    assert ModpGroup(WH.group15(), elem_bytes=WH.EB).has_device_share_hash is True
    for q in (2 ** 257 - 1, 2 ** 257 + 1, small[256], small[512]):
        assert ModpGroup(q).has_device_share_hash is ((q - 1) // 2 >= 2 ** 256)


@pytest.mark.parametrize("eb,q", [(256, H.rfc_prime(2048)), (WH.EB, WH.group15())], ids=["256", "384"])
def test_transcript_rows_cover_what_they_claim(eb, q):
    rows = SH.transcript_rows(eb, q, seed=0xA0 + eb)
    n = len(rows)
    assert 320 <= n <= 400 and n % 64 != 0
    assert all(0 <= v < (1 << (8 * eb)) for row in rows for v in row)
    splits = {}
    for row in rows:
        ls = SH.lengths(row)
        c, ln = SH.challenge(*row)
        assert ln == 32 + sum(ls) and 0 <= c < (q - 1) // 2           # hash_to_scalar's reduction is the identity for this q
        assert O.append_transcript(O.ModpGroup(), *row) == b"".join(len(b).to_bytes(8, "big") + b for b in
                                                                    (v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big") for v in row))
        splits.setdefault(ln % 64, set()).add(ls)
    # every residue of the message length, each with at least four different splits of the four lengths
    assert sorted(splits) == list(range(64)) and min(len(v) for v in splits.values()) >= 4
    every = [s for v in splits.values() for s in v]
    edge = {1, 2, 3, 4, 5} | set(range(eb - 4, eb + 1))
    for k in range(4):
        assert edge <= {s[k] for s in every}, k
        assert {0, 1} <= {row[k] for row in rows}, k                  # length 1 as the value 0 and as the value 1
        assert any(row[k] >= q for row in rows), k                    # hashed as given, not reduced
        # each position of the leading non-zero byte within a word
        assert {(eb - s[k]) & 3 for s in every} == {0, 1, 2, 3}, k
    # each alignment of the block buffer where an element's bytes start (the first element always starts at byte 8)
    for k in range(1, 4):
        assert {(8 * (k + 1) + sum(s[:k])) & 3 for s in every} == {0, 1, 2, 3}, k
    # neighbouring rows (lanes of one wave) have different lengths
    assert sum(1 for a, b in zip(rows, rows[1:]) if SH.lengths(a) != SH.lengths(b)) > 0.9 * n
    # the generator is deterministic: the GPU tests share these rows
    assert rows == SH.transcript_rows(eb, q, seed=0xA0 + eb)


MUST_VERIFY = {
    "512": (lambda: H.small_safe_primes()[512], 256),
    "1024": (lambda: H.rfc_prime(1024), 256),
    "2048": (lambda: H.rfc_prime(2048), 256),
    "group15": (WH.group15, WH.EB),
    "2^257+1": (lambda: 2 ** 257 + 1, 256),
}


@pytest.mark.parametrize("name", list(MUST_VERIFY))
def test_must_verify_rows_verify_in_the_oracle(name):
    q, eb = MUST_VERIFY[name][0](), MUST_VERIFY[name][1]
    g = H.RtOracleGroup(q)
    rows = SH.must_verify_rows(g, seed=0xB0)
    nbytes = (q.bit_length() + 7) // 8
    assert len(rows) >= 4 * nbytes and len(rows) % 64 != 0
    assert {row[6] for row in rows} >= set(range(1, nbytes + 1))       # a1's length sweeps 1 .. bytes of q
    assert {(eb - row[6]) & 3 for row in rows} == {0, 1, 2, 3}
    assert {(8 + 1 + 8 + 1 + 8 + row[6]) & 3 for row in rows} == {0, 1, 2, 3}
    if nbytes >= 64:
        assert {row[5] % 64 for row in rows} == set(range(64))        # every padding residue of the message length
    for pk, s, y, c, r, ln, l1, l2 in rows:
        assert 0 < c < (q - 1) // 2 and 0 < r < q - 1
        assert O.dleq_verify(g, g.generator(), pk, s, y, c, r) is True
        # what the tampered variants of the GPU test rely on: none of them is the challenge again
        assert c ^ 1 != c and c + 2 ** 256 != c and (c + (q - 1) // 2) % (1 << (8 * eb)) != c
