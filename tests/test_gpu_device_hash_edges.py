"""The per-share transcript hash that runs on the device (verdict_kernels.hip: LaneSha256, frame_modp, frame_fixed) at its byte
edges, with rows whose verdict must be 1 -- a row that comes out 0 cannot tell a right hash from a wrong one -- and with
the challenge the prover's kernel hands out.  The expected values come from hashlib over oracle.append_transcript.

Message length of a MODP row = 32 + the four minimal element lengths: the sweeps visit every residue mod 64 (SHA-256
padding spills into a further block at 56 ... 63, fills the block exactly at 55), every position of the leading non-zero
byte inside a 32-bit word (frame_modp's skip), and every alignment of the block buffer at the start of an element
(push_be32's word / byte path).

Not reachable here: the branch of the secp256k1 kernel that subtracts n once when the 256-bit hash is >= n needs a
SHA-256 output above 2^256 - 2^129, probability 2^-127 per row; the subtraction is written inline in the kernel
(ec_scalar.h does not hold it), so the CPU shim cannot reach it either.  It stays uncovered."""
import hashlib
import random

import pytest

import modp_rt_helpers as H
import mpvss_oracle as O
from helpers import cat, split
from mpvss_rs_amd import ModpGroup, capi

pytestmark = pytest.mark.gpu

G = O.ModpGroup()
Q = G.q


def challenge_of(g, pk, y, a1, a2):
    """hash_to_scalar(SHA256(transcript)) of modp.rs:142-148 with hashlib alone"""
    msg = O.append_transcript(g, pk, y, a1, a2)
    return int.from_bytes(hashlib.sha256(hashlib.sha256(msg).digest()).digest(), "big") % g.g, len(msg)


def must_verify_rows(g, max_len, seed, per_len=1):
    """DLEQ(2, pk, S, Y) rows with pk, Y in {0, 1}: a1 = 2^r pk^c and a2 = S^r Y^c do not depend on c > 0, so c can be the hash of the
    transcript.  r = 8 (L - 1) + j makes a1 = 2^r an L-byte element whose leading byte is 2^j; S = 1 / 2 makes a2 one byte or L bytes."""
    rows = []
    for L in range(1, max_len + 1):
        for j in ((L % 8), (L * 3 + 5) % 8)[:per_len]:
            r = 8 * (L - 1) + j
            if r < 1 or r >= g.q.bit_length() - 1:
                r = 8 * (L - 1) + 1
            rows.append((1, 1, 1, r))
            rows.append((1, 2, 1, r))
        if L % 2:
            rows.append((1, 2, 0, 8 * (L - 1) + 3))        # a2 = 0: one 0x00 byte
        if L % 3 == 0:
            rows.append((0, 2, 1, 8 * (L - 1) + 6))        # a1 = 0
    random.Random(seed).shuffle(rows)                       # neighbouring lanes of a wave get different lengths
    out = []
    for pk, s, y, r in rows:
        a1 = pow(2, r, g.q) * pk % g.q
        a2 = pow(s, r, g.q) * y % g.q
        c, ln = challenge_of(g, pk, y, a1, a2)
        assert c > 0 and O.dleq_verify(g, g.generator(), pk, s, y, c, r) is True
        out.append((pk, s, y, c, r, ln, len(g.element_to_bytes(a1)), len(g.element_to_bytes(a2))))
    return out


def run_must_verify(rows, call):
    n = len(rows)
    pk, s, y, c, r = ([row[k] for row in rows] for k in range(5))
    got = call(cat(G, pk), cat(G, s), cat(G, y), cat(G, c), cat(G, r))
    print(f"rows {n}, verified {sum(got)}")
    assert len(got) == n and [i for i in range(n) if got[i] != 1] == []
    flipped = [ci ^ (1 << (i % 255)) for i, ci in enumerate(c)]
    got = call(cat(G, pk), cat(G, s), cat(G, y), cat(G, flipped), cat(G, r))
    assert len(got) == n and [i for i in range(n) if got[i] != 0] == []


def test_modp_rows_that_must_verify_at_every_padding_residue(engine):
    rows = must_verify_rows(G, 256, seed=0x5A)
    n = len(rows)
    assert n >= 512 and n % 64 != 0
    residues = {}
    for row in rows:
        residues.setdefault(row[5] % 64, set()).add(row[5])
    assert sorted(residues) == list(range(64)) and min(len(v) for v in residues.values()) >= 4
    # the leading non-zero byte of a1 at each byte of a word, the block buffer at each alignment when a2 starts
    assert {(256 - row[6]) & 3 for row in rows} == {0, 1, 2, 3}
    assert {(8 + 1 + 8 + 1 + 8 + row[6]) & 3 for row in rows} == {0, 1, 2, 3}
    assert sum(1 for a, b in zip(rows, rows[1:]) if a[5] != b[5]) > 0.9 * n
    run_must_verify(rows, engine.verify_shares)


def test_runtime_group_rows_that_must_verify(engine):
    """mpvss_modp_group_verify_shares takes the products from the GPU and frames each share's transcript on the host, out of the
    same 256-byte fields: the reference frames the minimal bytes of the value (modp.rs:150-152), at most 32 here and never the
    field width, and hash_to_scalar reduces mod (q - 1) / 2 for real.  Same must-verify sweep, lengths 1 ... 32."""
    q = H.small_safe_primes()[256]
    g = H.RtOracleGroup(q)
    grp = ModpGroup(q)
    rows = must_verify_rows(g, 32, seed=0x5B, per_len=2)
    assert len(rows) >= 128 and len(rows) % 64 != 0
    assert max(row[5] for row in rows) <= 32 + 1 + 1 + 32 + 32 and {row[6] for row in rows} == set(range(1, 33))
    assert any(int.from_bytes(hashlib.sha256(hashlib.sha256(O.append_transcript(g, row[0], row[2], pow(2, row[4], q) * row[0] % q,
               pow(row[1], row[4], q) * row[2] % q)).digest()).digest(), "big") >= g.g for row in rows)   # the reduction bites
    run_must_verify(rows, lambda *a: engine.group_verify_shares(grp, *a))


def extract_rows(per_residue, seed, allow_zero_y):
    """extract_secret_share rows with xinv = 1, Y = 2^k (+ q for some), witness w: S = Y, a1 = 2^w, a2 = 2^(k w) mod q, pk hashed as
    given -- its length is chosen so that the message length hits a wanted residue mod 64."""
    rng = random.Random(seed)
    combos = [(k, w) for k in (0, 1, 7, 8, 15, 16, 23, 24, 31, 32, 39) for w in (0, 1, 2, 9, 17, 25, 33)]     # lengths 1 .. 5 and their products
    combos += [(k, 1) for k in (2007, 2008, 2015, 2016, 2023, 2024, 2031, 2032, 2039, 2040, 2047)]             # Y, a2: 251 ... 256 bytes
    combos += [(1, w) for w in (2007, 2008, 2016, 2024, 2032, 2040, 2047)] + [(0, 2047), (0, 2040)]            # a1 (and a2): 252 ... 256
    combos += [(k, w) for k, w in ((700, 2), (255, 8), (1000, 3), (1999, 1999), (2047, 2047), (1024, 1024))]   # a2 wraps mod q
    rows = []
    i = 0
    for rho in range(64):
        for j in range(per_residue):
            k, w = combos[i % len(combos)]
            i += 1
            y = 1 << k
            if k < 1900 and i % 5 == 0:
                y += Q                                          # an element >= q: hashed as given, 256 bytes
            if allow_zero_y and i % 41 == 0:
                y = 0
            a1, a2 = pow(2, w, Q), pow(y, w, Q)
            rest = sum(len(G.element_to_bytes(e)) for e in (y, a1, a2))
            lpk = (rho - 32 - rest) % 64
            lpk += 64 * ((j + rho) % 4)
            lpk = lpk or 64
            if lpk == 1:
                pk = (0, 1, 0x80, 0xFF)[(i // 3) % 4]
            elif lpk == 256 and i % 2:
                pk = Q + rng.randrange(1 << 1900)               # >= q
            else:
                pk = rng.randrange(1 << (8 * lpk - 8), 1 << (8 * lpk))
            rows.append((pk, y, w, a1, a2))
    for lpk in (2, 3, 4, 5, 252, 253, 254, 255, 256):         # pk at the short and the long lengths whatever the residues asked for
        rows.append((rng.randrange(1 << (8 * lpk - 8), 1 << (8 * lpk)), 1 << (lpk % 7), 3, 8, pow(8, lpk % 7, Q)))
    for idx, pk in enumerate((0, 1, 0, 1)):                    # one-byte pk: the value 0 and the value 1
        rows.append((pk, 1 << (8 * idx + 1), idx, 1 << idx, pow(2, (8 * idx + 1) * idx, Q)))
    rng.shuffle(rows)
    return rows


def check_extract(engine, rows, how):
    n = len(rows)
    pk, y, w = ([row[k] for row in rows] for k in range(3))
    args = (cat(G, pk), cat(G, y), cat(G, [1] * n), cat(G, w))
    if how == "blocks":
        assert engine.extract_shares_compute(*args) == n
        S, c = engine.extract_shares_absorb(n)
    else:
        S, c = engine.extract_shares(*args)
    got_s, got_c = split(S), split(c)
    assert len(got_s) == n and len(got_c) == n
    want_c, splits = [], {}
    for p, yy, ww, a1, a2 in rows:
        ci, ln = challenge_of(G, p, yy, a1, a2)
        want_c.append(ci)
        splits.setdefault(ln % 64, set()).add(tuple(len(G.element_to_bytes(e)) for e in (p, yy, a1, a2)))
    assert sorted(splits) == list(range(64)) and min(len(v) for v in splits.values()) >= 4
    assert got_s == [yy % Q for yy in y]
    bad = [i for i in range(n) if got_c[i] != want_c[i]]
    print(f"{how}: rows {n}, challenges equal {n - len(bad)}")
    assert bad == []
    return splits


def test_extract_shares_challenges_at_every_residue_and_split(engine):
    """K7 with c_out32: c_i = H(framed(pk) framed(Y) framed(a1) framed(a2)) for element lengths 1 (values 0 and 1), 2 ... 5, 251 ... 256,
    elements >= q, every residue of the message length with at least four different splits; below 1024 shares (two dependent
    exponentiations) through both entry points, and from 1024 shares (one chain of squarings for S and a2)."""
    small = extract_rows(5, seed=0xC0, allow_zero_y=True)
    assert len(small) == 333
    splits = check_extract(engine, small, "call")
    # the block form refuses a batch with a Y that is 0 mod q (include/mpvss_hip.h) and enqueues nothing: the same rows without one
    with pytest.raises(capi.EngineError, match="0 mod q"):
        check_extract(engine, small, "blocks")
    blocks = extract_rows(5, seed=0xC2, allow_zero_y=False)
    assert len(blocks) == 333
    check_extract(engine, blocks, "blocks")
    lens = [set(s[k] for v in splits.values() for s in v) for k in range(4)]
    assert {1, 2, 3, 4, 5} <= lens[0] and {1, 2, 3, 4, 5} <= lens[1] and {1, 2, 3, 4, 5} <= lens[2] and {1, 2, 3, 4, 5} <= lens[3]
    for k in range(4):
        assert {252, 253, 254, 255, 256} <= lens[k], k
    assert {0, 1} <= {row[0] for row in small} and 0 in {row[1] for row in small} and any(row[1] >= Q for row in small)
    # every alignment of the block buffer at the start of each element's bytes, every byte position of a leading byte
    for k in range(1, 4):
        assert {(8 * (k + 1) + sum(s[:k])) & 3 for v in splits.values() for s in v} == {0, 1, 2, 3}
    for k in range(4):
        assert {(256 - s[k]) & 3 for v in splits.values() for s in v} == {0, 1, 2, 3}
    large = extract_rows(17, seed=0xC1, allow_zero_y=False)       # (a Y that is 0 mod q would send the batch down the two-step path)
    assert len(large) == 1101 and all(row[1] % Q for row in large)
    check_extract(engine, large, "call")


@pytest.mark.parametrize("name", ["secp256k1", "ristretto255"])
def test_curve_share_proofs_all_verify_and_each_flipped_bit_is_noticed(engine, name):
    """Curve transcripts have one length (4 x 41 / 4 x 40 bytes): no sweep, but 260 honest proofs in one call -- five waves, the last
    one partial -- must all verify, and none may once a bit of c or r is flipped or pk (a1's source) / S (a2's source) is another
    valid point.  Challenges come from hashlib over the oracle's framing."""
    Gc = O.GROUPS[name]()
    gid = {"secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}[name]
    order = Gc.group_order_int()
    rng = random.Random(0xD1E0 + gid)
    B = Gc.generator()
    n, keys = 260, 4
    xs = [rng.randrange(1, order) for _ in range(keys)]
    pk = [Gc.exp(B, x) for x in xs]
    S = [Gc.exp(B, rng.randrange(1, order)) for _ in range(keys)]
    Y = [Gc.exp(s, x) for s, x in zip(S, xs)]
    w0 = [rng.randrange(1, order - n) for _ in range(keys)]
    a1 = [Gc.exp(B, w) for w in w0]
    a2 = [Gc.exp(s, w) for s, w in zip(S, w0)]
    e = Gc.element_to_bytes
    rows = []
    for i in range(n):
        j = i % keys
        msg = b"".join(len(b).to_bytes(8, "big") + b for b in (e(pk[j]), e(Y[j]), e(a1[j]), e(a2[j])))
        assert msg == O.append_transcript(Gc, pk[j], Y[j], a1[j], a2[j]) and len(msg) == 4 * (8 + Gc.elem_len)
        c = Gc.hash_to_scalar(hashlib.sha256(msg).digest())
        r = (w0[j] + i // keys - xs[j] * c) % order
        rows.append((e(pk[j]), e(S[j]), e(Y[j]), c, r))
        a1[j], a2[j] = Gc.mul(a1[j], B), Gc.mul(a2[j], S[j])                 # witness + 1
    assert O.dleq_verify(Gc, B, pk[3], S[3], Y[3], rows[n - 1][3], rows[n - 1][4]) is True
    sc = Gc.scalar_to_bytes
    col = lambda k: b"".join(row[k] for row in rows)
    cs, rs = [row[3] for row in rows], [row[4] for row in rows]

    def verdicts(pkb=None, sb=None, c=cs, r=rs):
        got = engine.ec_verify_shares(gid, pkb or col(0), sb or col(1), col(2), b"".join(map(sc, c)), b"".join(map(sc, r)))
        assert len(got) == n
        return list(got)

    assert verdicts() == [1] * n
    flip = lambda v, i: v ^ (1 << (i % 250))
    assert all(flip(v, i) < order for i, v in enumerate(cs)) and all(flip(v, i) < order for i, v in enumerate(rs))
    assert verdicts(c=[flip(v, i) for i, v in enumerate(cs)]) == [0] * n
    assert verdicts(r=[flip(v, i) for i, v in enumerate(rs)]) == [0] * n
    assert verdicts(pkb=b"".join(rows[(i + 1) % n][0] for i in range(n))) == [0] * n
    assert verdicts(sb=b"".join(rows[(i + 1) % n][1] for i in range(n))) == [0] * n
    assert verdicts() == [1] * n
