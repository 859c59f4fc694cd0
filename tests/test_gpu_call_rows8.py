"""Call tables with eight rows of 256 bits and 5-bit windows per key (RowGeom<8, 256, 5>, k_modp_call_rows_dual_exp_pair): the a2 of
served boxes at the edges of that geometry.  Responses at the row boundaries 256 k (2^(256k) - 1, 2^(256k), 2^(256k) + 1), in the 1-bit
top window of every row (bit 256 k + 255), with one row set and the others zero, all-ones windows alternating with all-zero ones;
challenges that reach weight 255 (2^256 - 1, 2^255 + 1), which a chain started below 255 would lose; keys 1 and q - 1.

As in test_gpu_call_tables.test_a2_bytes_of_edge_exponents, the one-box block entry point is the only one that hands a2 out and it
never gets call rows: its a2 bytes are compared with Python's pow at the edge shares, and the served call's digest -- the SHA-256 over
every X, Y, a1, a2 byte of the box -- must be the digest of exactly those bytes, and of the same call with call tables off.

The smallest boxes that reach the path: n = 16 385, t = 8 (Horner X path: Y^c by the fixed nibbles of c, from a chain that starts
at 255 and multiplies first at 252) and n = 16 415, t = 64 (forward differences: the host's sliding-window schedule of c)."""
import random

import pytest

from helpers import EB
from mpvss_rs_amd import capi
from test_call_rows8_model import edge_responses
from test_gpu_call_tables import Deck, Q, fx, served

pytestmark = pytest.mark.gpu

C_TOP = [(1 << 256) - 1, (1 << 255) + 1]


def at_shares(n):
    return [0, 1, 31, 32, 33, 63, 64, 16383, 16384, n - 2, n - 1]


@pytest.fixture(scope="module", params=[(16385, 8), (16415, 64)], ids=["n16385_t8_horner", "n16415_t64_fd"])
def deck(request, engine):
    n, t = request.param
    dk = Deck(engine, n, t, seed=8 * n + t)
    rng = random.Random(n)
    at, edge = at_shares(n), edge_responses()
    keys = [pow(2, rng.randrange(Q - 1), Q) for _ in range(40)]
    keys = [keys[rng.randrange(40)] * pow(2, i, Q) % Q for i in range(n)]
    keys[1], keys[33], keys[16384], keys[n - 1] = 1, Q - 1, 1, Q - 1
    dk.key_ints = keys
    dk.pk = b"".join(map(fx, keys))
    K = dict(host=dk.pk, dev=dk.dev(dk.pk))
    dk.shares = rng.randbytes(EB * n)
    dk.cm = b"".join(fx(pow(4, rng.randrange(Q - 1), Q)) for _ in range(t))
    # box b: the named shares take the edges from 11 b on (three boxes: 33 of the 40), shares 100 .. 139 -- the end of one wave's 32 shares and
    # the start of the next -- take every edge in turn
    dk.checked = at + list(range(100, 100 + len(edge)))
    dk.boxes = []
    for b, c in enumerate([rng.randrange(1 << 255, 1 << 256)] + C_TOP):
        resp = bytearray(rng.randbytes(EB * n))
        for k, i in enumerate(at):
            resp[i * EB:(i + 1) * EB] = fx(edge[(len(at) * b + k) % len(edge)])
        for k, e in enumerate(edge):
            resp[(100 + k) * EB:(101 + k) * EB] = fx(e)
        dk.boxes.append(dict(keys=K, cm=dk.cm, Y=dk.shares, r=bytes(resp), c=fx(c)))
    assert engine.set_call_tables(3) in (0, 3)
    dk.arr = dk.array(dk.boxes)
    dk.on, dk.stats = served(engine, lambda: dk.run(dk.arr))
    yield dk
    engine.set_call_tables(3)


def test_served_digests_equal_the_plain_path(engine, deck):
    assert deck.stats == (1, 3)
    assert engine.set_call_tables(0) == 3
    try:
        off, st = served(engine, lambda: deck.run(deck.arr))
    finally:
        engine.set_call_tables(3)
    assert st == (0, 0)
    assert off == deck.on
    assert len({d for _, d in deck.on}) == 3
    assert engine.blocks_in_flight() == (0, 0)


def test_a2_bytes_at_row_and_challenge_edges(engine, deck):
    n = deck.n
    for b, (_, digest) in zip(deck.boxes, deck.on):
        engine.verify_block_compute(deck.cm, deck.pos, deck.pk, deck.shares, b["r"], b["c"])
        st_, _, _, A2 = engine.verify_block_absorb_dump(capi.transcript_init(), n)
        assert capi.transcript_verdict(st_, b["c"])[1] == digest
        c = int.from_bytes(b["c"], "big")
        for i in deck.checked:
            Y = int.from_bytes(deck.shares[i * EB:(i + 1) * EB], "big")
            r = int.from_bytes(b["r"][i * EB:(i + 1) * EB], "big")
            assert int.from_bytes(A2[i * EB:(i + 1) * EB], "big") == pow(deck.key_ints[i], r, Q) * pow(Y, c, Q) % Q, i


def test_nibble_form_with_the_top_bit_of_c(engine, deck):
    """a Horner box (t = 8) takes Y^c by the fixed nibbles of c: one more call whose three boxes all carry c = 2^255 + 1 -- nibble 8 at
    weight 252, reached from the chain's start at 255 by three squarings -- and differ in their responses"""
    if deck.t != 8:
        return                              # (the forward-difference deck takes the schedule of c: covered above)
    boxes = [dict(b, c=fx((1 << 255) + 1)) for b in deck.boxes]
    arr = deck.array(boxes)
    on, st = served(engine, lambda: deck.run(arr))
    assert st == (1, 3)
    engine.set_call_tables(0)
    try:
        off, st = served(engine, lambda: deck.run(arr))
    finally:
        engine.set_call_tables(3)
    assert st == (0, 0) and off == on
    assert on[2] == deck.on[2]              # the same box as in the deck's own call
    b = boxes[0]
    engine.verify_block_compute(deck.cm, deck.pos, deck.pk, deck.shares, b["r"], b["c"])
    st_, _, _, A2 = engine.verify_block_absorb_dump(capi.transcript_init(), deck.n)
    assert capi.transcript_verdict(st_, b["c"])[1] == on[0][1]
    for i in deck.checked:
        Y = int.from_bytes(deck.shares[i * EB:(i + 1) * EB], "big")
        r = int.from_bytes(b["r"][i * EB:(i + 1) * EB], "big")
        assert int.from_bytes(A2[i * EB:(i + 1) * EB], "big") == pow(deck.key_ints[i], r, Q) * pow(Y, (1 << 255) + 1, Q) % Q, i
