"""The classified encodings of tests/encoding_vectors.py through the kernels of ec_kernels.hip that decode a point, reached through
the C ABI, both curves.  A rejecting vector fails exactly one decode check (tests/test_ec_encodings_host.py runs the same vectors
through the g++ build of the same header): here the point is that EVERY instantiation of Curve::decode rejects it and that the
entry point names the array and the smallest bad index, as include/mpvss_hip.h documents.

Which kernel decodes for which entry point (capi_ec.inc):
  k_*_add           mpvss_ec_batch_mul
  k_*_build_tables  everything that goes through ec_dual(): mpvss_ec_batch_exp at EVERY batch size, mpvss_ec_dleq_commitments,
                    mpvss_ec_verify_shares, the a1 / a2 legs of verify_distribution / distribute / extract_shares
  k_*_decode        the commitments of mpvss_ec_commit_eval / verify_distribution / verify_many / distribute
  dual_mul_body     ec_launch_dual_mul has no caller in the library: no entry point and no batch size reaches it, so there is nothing
                    to select and nothing observable; it is covered only as far as it shares Curve::decode with the others.
mpvss_ec_deal stages the public keys into buffers of its own and mpvss_ec_verify_many takes device-resident boxes as well: both are
here (test_deal_and_device_resident_boxes)."""
import json
import os
import random
import re

import pytest

import encoding_vectors as EV
import mpvss_oracle as O
from mpvss_rs_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GID = {"secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}
NAMES = ["secp256k1", "ristretto255"]


def setup(name):
    G = O.GROUPS[name]()
    return G, GID[name], G.elem_len, G.element_to_bytes, G.scalar_to_bytes


def good_points(G, n, seed):
    rng = random.Random(seed)
    base = [G.exp(G.generator(), rng.randrange(1, G.group_order_int())) for _ in range(6)]
    pts, acc = [], base[0]
    for i in range(n):
        acc = G.mul(acc, base[i % 6])
        pts.append(acc)
    return pts


def put(blob, L, i, enc):
    return blob[:i * L] + enc + blob[(i + 1) * L:]


def rejected(engine, call, what, index):
    """the call raises EngineError naming `what` and `element index`"""
    with pytest.raises(capi.EngineError) as ei:
        call()
    msg = str(ei.value) + " | " + engine.last_error()
    assert re.search(rf"{re.escape(what)}: element {index} is not a valid", msg), msg


def fixture_box(name):
    fx = json.load(open(os.path.join(HERE, "golden", f"{name}_n8_t4.json")))
    b = fx["box"]
    cat = lambda hs: bytes.fromhex("".join(hs))
    box = {"commitments": cat(b["commitments"]), "positions": b["positions"], "pubkeys": cat(b["publickeys"]),
           "shares": cat(b["shares"]), "responses": cat(b["responses"]), "challenge": bytes.fromhex(b["challenge"])}
    return fx, box, (True, bytes.fromhex(fx["expected"]["transcript_digest"]))


def verify_box(engine, gid, box):
    r = engine.ec_verify_distribution(gid, box["commitments"], box["positions"], box["pubkeys"], box["shares"], box["responses"],
                                      box["challenge"])
    return r["verdict"], r["digest"]


@pytest.mark.parametrize("name", NAMES)
def test_batch_mul_rejects_every_vector_in_either_operand(engine, name):
    """k_*_add: one call per rejecting vector and operand (a call reports one index), the vector at a moving index of a 70-point batch"""
    G, gid, L, e, _ = setup(name)
    n = 70
    good = b"".join(map(e, good_points(G, n, 1)))
    bad = EV.rejecting(name)
    sent = 0
    for k, (label, enc) in enumerate(bad):
        i = (k * 7) % n
        rejected(engine, lambda: engine.ec_batch_mul(gid, put(good, L, i, enc), good), "ec_batch_mul operands", i)
        rejected(engine, lambda: engine.ec_batch_mul(gid, good, put(good, L, i, enc)), "ec_batch_mul operands", i)
        sent += 2
    assert sent == 2 * len(bad) and len(bad) >= 70
    assert engine.ec_batch_mul(gid, good, good) == b"".join(e(G.mul(p, p)) for p in good_points(G, n, 1))
    fx, box, want = fixture_box(name)
    assert verify_box(engine, gid, box) == want


@pytest.mark.parametrize("name", NAMES)
def test_the_smallest_bad_index_is_named(engine, name):
    G, gid, L, e, s = setup(name)
    reps = EV.representatives(name)
    x, y = reps[0][1], reps[-1][1]
    for n, idxs in ((1, [0]), (64, [0, 63]), (65, [64]), (101, [0, 63, 64, 100]), (165, [164, 64, 63])):
        good = b"".join(map(e, good_points(G, n, n)))
        ones = s(1) * n
        for i in idxs:
            rejected(engine, lambda: engine.ec_batch_mul(gid, put(good, L, i, x), good), "ec_batch_mul operands", i)
            rejected(engine, lambda: engine.ec_batch_exp(gid, put(good, L, i, x), ones), "ec_batch_exp bases", i)
        if n > 1:
            lo, hi = min(idxs), n - 1 if min(idxs) != n - 1 else n - 2
            lo, hi = min(lo, hi), max(lo, hi)
            two = put(put(good, L, hi, x), L, lo, y)
            rejected(engine, lambda: engine.ec_batch_mul(gid, two, good), "ec_batch_mul operands", lo)
            rejected(engine, lambda: engine.ec_batch_mul(gid, put(good, L, hi, x), put(good, L, lo, y)), "ec_batch_mul operands", lo)
            rejected(engine, lambda: engine.ec_batch_exp(gid, two, ones), "ec_batch_exp bases", lo)
    fx, box, want = fixture_box(name)
    assert verify_box(engine, gid, box) == want


@pytest.mark.parametrize("name", NAMES)
def test_every_class_through_the_table_builder_and_the_commitment_decoder(engine, name):
    """k_*_build_tables (batch_exp -- at one share and at 600, the same path: see the module text --, dleq_commitments in all four arrays,
    verify_shares) and k_*_decode (commit_eval), one representative per class"""
    G, gid, L, e, s = setup(name)
    rng = random.Random(5)
    order = G.group_order_int()
    reps = EV.representatives(name)
    assert len(reps) >= 4
    pts = good_points(G, 600, 2)
    good600 = b"".join(map(e, pts))
    k600 = b"".join(s(rng.randrange(order)) for _ in range(600))
    n = 37
    good = good600[:n * L]
    ks = k600[:n * 32]
    cm = good600[:5 * L]
    gen = e(G.generator())
    other_g1 = e(pts[7])
    for k, (cls, enc) in enumerate(reps):
        i = (11 * k + 3) % n
        rejected(engine, lambda: engine.ec_batch_exp(gid, enc, s(5)), "ec_batch_exp bases", 0)
        rejected(engine, lambda: engine.ec_batch_exp(gid, put(good600, L, 599 - k, enc), k600), "ec_batch_exp bases", 599 - k)
        j = k % 5
        rejected(engine, lambda: engine.ec_commit_eval(gid, put(cm, L, j, enc), [1, 2, 3, 70000]), "commitments", j)
        args = lambda g1=gen, h1=good, g2=good, h2=good: engine.ec_dleq_commitments(gid, g1, h1, g2, h2, ks, ks, True)
        rejected(engine, lambda: args(g1=enc), "ec_dleq_commitments elements", 0)
        rejected(engine, lambda: args(h1=put(good, L, i, enc)), "ec_dleq_commitments elements", n + i)
        rejected(engine, lambda: args(g1=other_g1, g2=put(good, L, i, enc)), "ec_dleq_commitments elements", 2 * n + i)
        rejected(engine, lambda: args(h2=put(good, L, i, enc)), "ec_dleq_commitments elements", 3 * n + i)
        for which in range(3):                      # pk, S, Y of a batch of share boxes
            arrs = [good, good, good]
            arrs[which] = put(good, L, i, enc)
            rejected(engine, lambda: engine.ec_verify_shares(gid, arrs[0], arrs[1], arrs[2], ks, ks), "share boxes", i)
    fx, box, want = fixture_box(name)
    assert verify_box(engine, gid, box) == want


@pytest.mark.parametrize("name", NAMES)
def test_every_class_through_the_box_entry_points(engine, name):
    """verify_distribution, verify_many, distribute, extract_shares, reconstruct with a representative of every class as a commitment,
    a public key, an encrypted share, a decrypted share"""
    G, gid, L, e, s = setup(name)
    fx, box, want = fixture_box(name)
    n, t = fx["n"], fx["t"]
    order = G.group_order_int()
    coeffs = [int(c, 16) for c in fx["inputs"]["coefficients"]]
    wits = b"".join(s(int(x, 16)) for x in fx["inputs"]["witnesses"])
    pvals = b"".join(s(sum(c * pow(p, j, order) for j, c in enumerate(coeffs)) % order) for p in box["positions"])
    ones = s(1) * n
    malformed = (False, bytes(32))
    for k, (cls, enc) in enumerate(EV.representatives(name)):
        i, j = (3 * k + 1) % n, k % t
        for field, what, idx in (("commitments", "commitments", j), ("pubkeys", "public keys", i), ("shares", "encrypted shares", i)):
            broken = dict(box, **{field: put(box[field], L, idx, enc)})
            rejected(engine, lambda: verify_box(engine, gid, broken), what, idx)
            assert engine.ec_verify_many(gid, [box, broken, box], depth=3, hash_threads=2) == [want, malformed, want], (cls, field)
            assert f"{what}: element {idx}" in engine.last_error()
        rejected(engine, lambda: engine.ec_distribute(gid, put(box["commitments"], L, j, enc), box["positions"], box["pubkeys"], pvals, wits),
                 "commitments", j)
        rejected(engine, lambda: engine.ec_distribute(gid, box["commitments"], box["positions"], put(box["pubkeys"], L, i, enc), pvals, wits),
                 "public keys", i)
        rejected(engine, lambda: engine.ec_extract_shares(gid, box["pubkeys"], put(box["shares"], L, i, enc), ones, ones), "encrypted shares", i)
        rejected(engine, lambda: engine.ec_reconstruct(gid, box["positions"], put(box["shares"], L, i, enc)), "ec_reconstruct shares", i)
    assert verify_box(engine, gid, box) == want
    d = engine.ec_distribute(gid, box["commitments"], box["positions"], box["pubkeys"], pvals, wits)
    assert d["Y"] == box["shares"] and d["digest"] == want[1]


@pytest.mark.parametrize("name", NAMES)
def test_deal_and_device_resident_boxes(engine, name):
    """mpvss_ec_deal (its own staging of the public keys) with a representative of every class as a public key: the error names the
    array and the index, and the next deal is the fixture's box again; mpvss_ec_verify_many over MPVSS_DEVICE buffers with a broken
    box between two good ones, for a commitment, a public key and an encrypted share."""
    import ctypes as C

    import torch
    G, gid, L, e, s = setup(name)
    fx, box, want = fixture_box(name)
    n, t = fx["n"], fx["t"]
    coeffs = b"".join(s(G.scalar_from_bigint(int(c, 16))) for c in fx["inputs"]["coefficients"])
    wits = b"".join(s(int(x, 16)) for x in fx["inputs"]["witnesses"])
    reps = EV.representatives(name)
    for k, (cls, enc) in enumerate(reps):
        i = (5 * k + 2) % n
        rejected(engine, lambda: engine.ec_deal(gid, coeffs, box["positions"], put(box["pubkeys"], L, i, enc), wits), "public keys", i)
    rejected(engine, lambda: engine.ec_deal(gid, coeffs, box["positions"], put(put(box["pubkeys"], L, n - 1, reps[0][1]), L, 1, reps[-1][1]), wits),
             "public keys", 1)
    d = engine.ec_deal(gid, coeffs, box["positions"], box["pubkeys"], wits)
    assert d["Y"] == box["shares"] and d["digest"] == want[1] and d["challenge"] == box["challenge"] and d["responses"] == box["responses"]
    assert d["X"].hex() == "".join(fx["expected"]["X"])

    dev = torch.device("cuda", 0)
    keep = []

    def dptr(b):
        tns = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
        keep.append(tns)
        return tns.data_ptr()

    def device_run(boxes):
        arr = (capi.EcBox * len(boxes))()
        for k, b in enumerate(boxes):
            pos = torch.tensor(b["positions"], dtype=torch.int64, device=dev)
            ch = (C.c_uint8 * 32).from_buffer_copy(b["challenge"])
            keep.extend([pos, ch])
            arr[k] = capi.EcBox(dptr(b["commitments"]), t, pos.data_ptr(), dptr(b["pubkeys"]), dptr(b["shares"]), dptr(b["responses"]),
                                len(b["positions"]), C.cast(ch, C.c_void_p))
        torch.cuda.synchronize()
        verdicts = (C.c_int * len(boxes))()
        out = (C.c_uint8 * (32 * len(boxes)))()
        engine._check(engine.lib.mpvss_ec_verify_many(engine.ctx, gid, capi.MPVSS_DEVICE, arr, len(boxes), 3, 2, verdicts,
                                                      C.cast(out, C.c_void_p)), "ec_verify_many(device)")
        raw = bytes(out)
        return [(bool(verdicts[k]), raw[32 * k:32 * k + 32]) for k in range(len(boxes))]

    sent = 0
    for k, (cls, enc) in enumerate(reps):
        field, what, idx = (("commitments", "commitments", k % t), ("pubkeys", "public keys", (3 * k + 1) % n),
                            ("shares", "encrypted shares", (3 * k + 2) % n))[k % 3]
        broken = dict(box, **{field: put(box[field], L, idx, enc)})
        assert device_run([box, broken, box]) == [want, (False, bytes(32)), want], (cls, field)
        assert f"{what}: element {idx}" in engine.last_error(), (cls, engine.last_error())
        sent += 1
    assert sent == len(reps) and len(reps) >= 4
    assert device_run([box]) == [want]


@pytest.mark.parametrize("name", NAMES)
def test_valid_vectors_give_the_oracles_results(engine, name):
    G, gid, L, e, s = setup(name)
    rng = random.Random(9)
    order = G.group_order_int()
    vs = EV.valid(name)
    n = len(vs)
    encs = [b for _, b, _ in vs]
    pts = [p for _, _, p in vs]
    blob = b"".join(encs)
    ident = e(G.identity())
    assert ident == bytes(L) and ident in encs
    # decode -> + identity -> encode gives the input back, from either operand (ristretto255: results re-encode canonically)
    for out in (engine.ec_batch_mul(gid, blob, ident * n), engine.ec_batch_mul(gid, ident * n, blob)):
        assert len(out) == n * L and [out[i * L:(i + 1) * L] for i in range(n)] == encs
    rot = pts[1:] + pts[:1]
    out = engine.ec_batch_mul(gid, blob, b"".join(encs[1:] + encs[:1]))
    assert [out[i * L:(i + 1) * L] for i in range(n)] == [e(G.mul(a, b)) for a, b in zip(pts, rot)]
    ks = [1, order - 1, 2, 0] + [rng.randrange(order) for _ in range(n - 4)]
    out = engine.ec_batch_exp(gid, blob, b"".join(map(s, ks)))
    assert len(out) == n * L and [out[i * L:(i + 1) * L] for i in range(n)] == [e(G.exp(p, k)) for p, k in zip(pts, ks)]
    # the identity as a commitment, a public key (h1), g1, Y (h2): the oracle's bytes
    cm = [pts[3], G.identity(), pts[5]]
    xs = engine.ec_commit_eval(gid, b"".join(map(e, cm)), [1, 2, 9])
    assert [xs[i * L:(i + 1) * L] for i in range(3)] == [e(O.commitment_eval(G, cm, i)) for i in (1, 2, 9)]
    # every valid vector as a commitment (k_*_decode) and in each array of dleq_commitments (k_*_build_tables), one call each
    xs = engine.ec_commit_eval(gid, blob, [1, 2])
    assert len(xs) == 2 * L and [xs[:L], xs[L:]] == [e(O.commitment_eval(G, pts, i)) for i in (1, 2)]
    rn = [rng.randrange(order) for _ in range(n)]
    cn = [rng.randrange(order) for _ in range(n)]
    a1, a2 = engine.ec_dleq_commitments(gid, e(pts[2]), blob, b"".join(encs[1:] + encs[:1]), b"".join(encs[2:] + encs[:2]),
                                        b"".join(map(s, rn)), b"".join(map(s, cn)), True)
    wantn = [O.dleq_verifier_commitments(G, pts[2], pts[i], pts[(i + 1) % n], pts[(i + 2) % n], rn[i], cn[i]) for i in range(n)]
    assert len(a1) == n * L and len(a2) == n * L
    assert [a1[i * L:(i + 1) * L] for i in range(n)] == [e(w[0]) for w in wantn]
    assert [a2[i * L:(i + 1) * L] for i in range(n)] == [e(w[1]) for w in wantn]
    m = 8
    h1 = [G.identity()] + pts[1:m]
    g2 = pts[m:2 * m]
    h2 = pts[2 * m:3 * m - 1] + [G.identity()]
    r = [rng.randrange(order) for _ in range(m)]
    c = [rng.randrange(order) for _ in range(m)]
    for g1 in (G.identity(), pts[4]):
        a1, a2 = engine.ec_dleq_commitments(gid, e(g1), b"".join(map(e, h1)), b"".join(map(e, g2)), b"".join(map(e, h2)),
                                            b"".join(map(s, r)), b"".join(map(s, c)), True)
        want = [O.dleq_verifier_commitments(G, g1, h1[i], g2[i], h2[i], r[i], c[i]) for i in range(m)]
        assert [a1[i * L:(i + 1) * L] for i in range(m)] == [e(w[0]) for w in want]
        assert [a2[i * L:(i + 1) * L] for i in range(m)] == [e(w[1]) for w in want]
    if name == "secp256k1":
        by_x = {}
        for b in encs:
            if any(b):
                by_x.setdefault(b[1:], set()).add(b[0])
        xs2 = [x for x, d in by_x.items() if d == {2, 3}]
        assert len(xs2) >= 34
        out = engine.ec_batch_mul(gid, b"".join(b"\x02" + x for x in xs2), b"".join(b"\x03" + x for x in xs2))
        assert out == bytes(33 * len(xs2))          # P and -P are different elements whose product is the identity


@pytest.mark.parametrize("name", NAMES)
def test_scalars_at_the_order(engine, name):
    """order - 1 is a scalar (oracle result); order, order + 1, 2^256 - 1 (and 2^252 + small for ristretto255) are not: the error names
    the scalar's index.  c and r alike."""
    G, gid, L, e, s = setup(name)
    order = G.group_order_int()
    raw = lambda v: v.to_bytes(32, "big" if name == "secp256k1" else "little")
    n = 9
    pts = good_points(G, 3 * n, 3)
    good = b"".join(map(e, pts[:n]))
    rng = random.Random(12)
    ks = [rng.randrange(order) for _ in range(n)]
    ks[4] = order - 1
    out = engine.ec_batch_exp(gid, good, b"".join(map(s, ks)))
    assert [out[i * L:(i + 1) * L] for i in range(n)] == [e(G.exp(p, k)) for p, k in zip(pts, ks)]
    h1, g2, h2 = (b"".join(map(e, pts[a:a + n])) for a in (0, n, 2 * n))
    a1, a2 = engine.ec_dleq_commitments(gid, e(G.generator()), h1, g2, h2, b"".join(map(s, ks)), b"".join(map(s, reversed(ks))), True)
    want = [O.dleq_verifier_commitments(G, G.generator(), pts[i], pts[n + i], pts[2 * n + i], ks[i], ks[n - 1 - i]) for i in range(n)]
    assert a1 == b"".join(e(w[0]) for w in want) and a2 == b"".join(e(w[1]) for w in want)
    too_big = [order, order + 1, (1 << 256) - 1] + ([(1 << 252) + (1 << 130), 1 << 253, 1 << 255] if name == "ristretto255" else [])
    kb = b"".join(map(s, ks))
    for k, v in enumerate(too_big):
        i = (2 * k + 1) % n
        broken = kb[:32 * i] + raw(v) + kb[32 * (i + 1):]
        with pytest.raises(capi.EngineError, match=rf"ec_batch_exp: scalar {i} "):
            engine.ec_batch_exp(gid, good, broken)
        with pytest.raises(capi.EngineError, match=rf"responses: scalar {i} "):
            engine.ec_dleq_commitments(gid, e(G.generator()), h1, g2, h2, broken, kb, True)
        with pytest.raises(capi.EngineError, match=rf"challenge: scalar {i} "):
            engine.ec_dleq_commitments(gid, e(G.generator()), h1, g2, h2, kb, broken, True)
        with pytest.raises(capi.EngineError, match=r"challenge: scalar 0 "):
            engine.ec_dleq_commitments(gid, e(G.generator()), h1, g2, h2, kb, raw(v), False)
        for c, r in ((broken, kb), (kb, broken)):
            with pytest.raises(capi.EngineError, match=rf"response or challenge: scalar {i} "):
                engine.ec_verify_shares(gid, h1, g2, h2, c, r)
    # share boxes that MUST verify with r = order - 1: pk = Y = identity make a1 = r G, a2 = r S independent of c, so c can be the hash
    # of the transcript (c itself is a hash: order - 1 cannot be forced there; batch_exp and dleq_commitments above pin it as a scalar)
    import hashlib
    ident = G.identity()
    rows_c = []
    for i in range(n):
        a1p, a2p = G.exp(G.generator(), order - 1), G.exp(pts[n + i], order - 1)
        assert O.append_transcript(G, ident, ident, a1p, a2p)[8:8 + L] == bytes(L)
        rows_c.append(G.hash_to_scalar(hashlib.sha256(O.append_transcript(G, ident, ident, a1p, a2p)).digest()))
        assert O.dleq_verify(G, G.generator(), ident, pts[n + i], ident, rows_c[i], order - 1) is True
    got = engine.ec_verify_shares(gid, e(ident) * n, g2, e(ident) * n, b"".join(map(s, rows_c)), s(order - 1) * n)
    assert len(got) == n and list(got) == [1] * n
    got = engine.ec_verify_shares(gid, e(ident) * n, g2, e(ident) * n, b"".join(map(s, rows_c)), s(order - 2) * n)
    assert list(got) == [0] * n
    # order - 1 in c and in r of dishonest share boxes: accepted as scalars, the rows simply do not verify
    top = s(order - 1) * n
    assert list(engine.ec_verify_shares(gid, h1, g2, h2, top, kb)) == [0] * n
    assert list(engine.ec_verify_shares(gid, h1, g2, h2, kb, top)) == [0] * n
