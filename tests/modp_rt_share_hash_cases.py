"""Rows for the per-share DLEQ hash of a run-time MODP group on the device (k_rt_share_verdict, verdict_kernels.hip;
mpvss_modp_group_dleq_challenges, _verify_shares and _extract_shares under mpvss_ctx_set_rt_share_hash).  Expected values come
from hashlib over oracle.append_transcript alone; tests/test_modp_rt_share_hash_cases.py holds the generator to its claims.

A transcript is framed(h1) framed(h2) framed(a1) framed(a2) with framed(b) = u64-BE(len) || the minimal big-endian bytes of the
element as given (zero: one 0x00 byte), so its length is 32 + the four element lengths.  transcript_rows() visits
  * every residue of that length mod 64 (SHA-256 padding spills into a further block at 56 .. 63) with at least four different
    splits of the four lengths,
  * element lengths 1 (the values 0 and 1), 2 .. 5 and EB - 4 .. EB in each of the four slots, hence every position of the leading
    non-zero byte within a 32-bit word and every alignment (mod 4) of the block buffer where an element's bytes start,
  * elements >= q (hashed as given: the kernel must not reduce them),
in an order in which neighbouring rows (lanes of one wave) have different lengths, with a row count that is no multiple of 64."""
import hashlib
import random

import mpvss_oracle as O

_G = O.ModpGroup()          # element_to_bytes / append_transcript do not depend on the modulus


def be_len(v):
    return len(_G.element_to_bytes(v))


def challenge(h1, h2, a1, a2):
    """(int_BE(SHA256(SHA256(transcript))), transcript length): hash_to_scalar of modp.rs:142-148 before its reduction, which is
    the identity for every modulus with (q-1)/2 >= 2^256"""
    msg = O.append_transcript(_G, h1, h2, a1, a2)
    return int.from_bytes(hashlib.sha256(hashlib.sha256(msg).digest()).digest(), "big"), len(msg)


def _value(rng, length, q, eb, k):
    """an element of exactly `length` minimal bytes; length 1 alternates the values 0, 1 and others; some full-width ones are >= q"""
    if length == 1:
        return (0, 1, 0x80, 0xFF, 1, 0)[k % 6]
    if length == eb and k % 2 and q < (1 << (8 * eb)) - 1 and q.bit_length() > 8 * eb - 8:
        return q + rng.randrange((1 << (8 * eb)) - q)
    return rng.randrange(1 << (8 * length - 8), 1 << (8 * length))


def transcript_rows(eb, q, seed, per_residue=5):
    """about 64 * per_residue + 4 * 10 rows (h1, h2, a1, a2) of integers below 2^(8 eb)"""
    rng = random.Random(seed)
    edge = [1, 2, 3, 4, 5] + list(range(eb - 4, eb + 1))
    rows, i = [], 0
    for rho in range(64):
        for j in range(per_residue):
            solved = (rho + j) % 4                              # the slot whose length makes the residue
            lens = [edge[(i * 7 + 3 * k + rho) % len(edge)] for k in range(4)]
            if (i + rho) % 3 == 0:                              # a middle length now and then
                lens[(solved + 1) % 4] = rng.randrange(6, eb - 4)
            rest = 32 + sum(lens) - lens[solved]
            span = (eb - 1) // 64                               # lengths base, base + 64, .. up to eb
            base = (rho - rest) % 64 or 64
            lens[solved] = min(base + 64 * ((j + rho) % (span + 1)), base + 64 * ((eb - base) // 64))
            assert 1 <= lens[solved] <= eb and (32 + sum(lens)) % 64 == rho
            rows.append(tuple(_value(rng, lens[k], q, eb, i + k) for k in range(4)))
            i += 1
    for slot in range(4):                                       # every edge length in every slot, whatever the residues asked for
        for length in edge:
            lens = [7 + slot, 40, eb - 9, 64]
            lens[slot] = length
            rows.append(tuple(_value(rng, lens[k], q, eb, i + slot) for k in range(4)))
            i += 1
    rng.shuffle(rows)
    if len(rows) % 64 == 0:
        rows.append((1, 0, q, 2))
    return rows


def lengths(row):
    return tuple(be_len(v) for v in row)


def must_verify_rows(g, seed, per_len=2):
    """DLEQ(2, pk, S, Y) rows with pk, Y in {0, 1}: a1 = 2^r pk^c and a2 = S^r Y^c do not depend on c > 0, so c can be the hash of the
    transcript itself (the construction of must_verify_rows in test_gpu_device_hash_edges.py, for the group g of any modulus).
    r = 8 (L - 1) + j makes a1 = 2^r an L-byte element whose leading byte is 2^j, L = 1 .. bytes of q; S = 1 / 2 makes a2 one
    byte or L bytes.  Rows (pk, s, y, c, r, transcript length, len a1, len a2), shuffled."""
    q = g.q
    rows = []
    for L in range(1, (q.bit_length() + 7) // 8 + 1):
        for j in ((L % 8), (L * 3 + 5) % 8)[:per_len]:
            r = 8 * (L - 1) + j
            if r < 1 or r >= q.bit_length() - 1:
                r = max(1, min(8 * (L - 1) + 1, q.bit_length() - 2))
            rows.append((1, 1, 1, r))
            rows.append((1, 2, 1, r))
        if L % 2:
            rows.append((1, 2, 0, min(8 * (L - 1) + 3, q.bit_length() - 2)))        # a2 = 0: one 0x00 byte
        if L % 3 == 0:
            rows.append((0, 2, 1, min(8 * (L - 1) + 6, q.bit_length() - 2)))        # a1 = 0
    random.Random(seed).shuffle(rows)
    out = []
    for pk, s, y, r in rows:
        a1 = pow(2, r, q) * pk % q
        a2 = pow(s, r, q) * y % q
        c, ln = challenge(pk, y, a1, a2)
        out.append((pk, s, y, c, r, ln, be_len(a1), be_len(a2)))
    if len(out) % 64 == 0:
        out.pop()
    return out


def cat(vals, eb):
    return b"".join(v.to_bytes(eb, "big") for v in vals)


def split(buf, eb):
    return [int.from_bytes(buf[i:i + eb], "big") for i in range(0, len(buf), eb)]
