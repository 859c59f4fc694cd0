"""Key sets of the curve groups on the GPU (include/mpvss_hip.h, "Key sets of a curve group"): the multiples over a set's rows, the
dealer's block and one-call forms, the encodings create accepts and refuses, spaces, chunks, threads and refusals.  Expected
values: the calls of the same engine that take the keys as an array (byte for byte), the plain-C reference (oracle/ec_ref.c)
and the golden fixtures."""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import threading

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":          # the chunk child (below) runs this file as a script
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
        sys.path.insert(0, p)

import torch

import ec_dual_cases as D
import ec_keyset_cases as K
import encoding_vectors as EV
import mpvss_oracle as O
from mpvss_rs_amd import capi

pytestmark = pytest.mark.gpu
GID = {"secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}
NKEYS = 523                  # neither a multiple of 64 nor of 256
MPVSS_E_INVALID = -1


def dev_u8(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")


def dbytes(t):
    return bytes(t.cpu().numpy().tobytes())


def split(b, n):
    return [b[i:i + n] for i in range(0, len(b), n)]


class SetUnderTest:
    """NKEYS keys of one curve -- G, the identity, -G, then random multiples of G -- and their set on the session's engine"""

    def __init__(self, engine, name, seed=0x5E7):
        self.name, self.kc, self.gid = name, K.cases(name), GID[name]
        kc = self.kc
        self.L, self.order = kc.L, kc.order
        rng = random.Random(seed + self.gid)
        self.key_scalars = [1, 0, kc.order - 1] + [rng.randrange(2, kc.order) for _ in range(NKEYS - 3)]
        # (the array calls of the same engine make the keys: mpvss_ec_batch_exp_generator is not under test here)
        self.keys = split(engine.ec_batch_exp_generator(self.gid, b"".join(kc.scalar(k) for k in self.key_scalars)), self.L)
        assert self.keys[:3] == kc.keys[:3] and self.keys[1] == bytes(self.L)
        self.set = engine.ec_keyset_create(self.gid, b"".join(self.keys))

    def slice(self, off, n):
        return b"".join(self.keys[off:off + n])


@pytest.fixture(scope="module", params=D.NAMES)
def sut(request, engine):
    s = SetUnderTest(engine, request.param)
    yield s
    s.set.close()


def scalars(kc, ks):
    return b"".join(kc.scalar(k) for k in ks)


# ---- 1. powers over a set ------------------------------------------------------------------------------------------------
def test_twin_exp_equals_two_batch_exp_calls_and_counts_its_powers(engine, sut):
    kc, gid, L = sut.kc, sut.gid, sut.L
    assert sut.set.n == NKEYS and sut.set.nbytes == NKEYS * engine.ec_keyset_bytes_per_key(gid)
    sampled = 0
    for n in D.SHAPES:
        for off in sorted({0, 1, 5, NKEYS - n}):
            k1, k2 = kc.lane_scalars(n, 7 * n + off), kc.lane_scalars(n, 11 * n + off + 1)
            keys = sut.slice(off, n)
            before = engine.ec_keyset_stats()
            one = off == 1                                   # e2 == NULL at one offset of every shape
            got1, got2 = engine.ec_keyset_twin_exp(gid, sut.set, off, scalars(kc, k1), None if one else scalars(kc, k2))
            after = engine.ec_keyset_stats()
            assert after[0] == before[0] and after[1] - before[1] == (n if one else 2 * n), (sut.name, n, off)
            assert got1 == engine.ec_batch_exp(gid, keys, scalars(kc, k1)), (sut.name, n, off)
            if one:
                assert got2 is None
            else:
                assert got2 == engine.ec_batch_exp(gid, keys, scalars(kc, k2)), (sut.name, n, off)
            if n == 513 and off == 0:                        # 40 results against the plain-C reference, the three special keys among them
                for i in list(range(5)) + list(range(8, 513, 14))[:35]:
                    assert got1[i * L:(i + 1) * L] == kc.mul(sut.keys[i], k1[i]), (sut.name, i)
                    sampled += 1
    assert sampled == 40


def test_every_edge_scalar_on_the_special_keys(engine, sut):
    """G, the identity and -G (keys 0, 1, 2) times every scalar of the model test's edge list, against the reference"""
    kc, gid, L = sut.kc, sut.gid, sut.L
    for key in range(3):
        for e0 in range(len(kc.edge)):
            got, _ = engine.ec_keyset_twin_exp(gid, sut.set, key, scalars(kc, [kc.edge[e0]]))
            assert got == kc.mul(sut.keys[key], kc.edge[e0]), (sut.name, key, hex(kc.edge[e0]))
    got, _ = engine.ec_keyset_twin_exp(gid, sut.set, 1, scalars(kc, [kc.order - 1]))
    assert got == bytes(L)                                   # every multiple of the identity is the identity


# ---- 2. dual_exp -------------------------------------------------------------------------------------------------------------
def test_dual_exp_equals_a2_of_dleq_commitments(engine, sut):
    kc, gid, L = sut.kc, sut.gid, sut.L
    rng = random.Random(0xD0A1 + gid)
    for n in (1, 65, 257):
        off = 2 if n < 257 else 0
        keys = sut.slice(off, n)
        e1 = [rng.randrange(kc.order) for _ in range(n)]
        e2 = [rng.randrange(kc.order) for _ in range(n)]
        h_rand = engine.ec_batch_exp_generator(gid, scalars(kc, [rng.randrange(1, kc.order) for _ in range(n)]))
        neg = engine.ec_batch_exp(gid, keys, scalars(kc, [kc.order - 1] * n))
        for tag, h2, s1, s2 in (("random h2", h_rand, e1, e2), ("h2 = the key", keys, e1, e2), ("h2 = -key, e1 = e2", neg, e1, e1),
                                ("h2 = the identity", bytes(L) * n, e1, e2)):
            # (g1, h1 of the array call feed its a1, which nobody reads here)
            want = engine.ec_dleq_commitments(gid, kc.cs.gen, h_rand, keys, h2, scalars(kc, s1), scalars(kc, s2), True)[1]
            got = engine.ec_keyset_dual_exp(gid, sut.set, off, scalars(kc, s1), h2, scalars(kc, s2), True)
            assert got == want, (sut.name, n, tag, "per-share e2")
            if tag.startswith("h2 = -key"):
                assert got == bytes(L) * n
            shared = s2[0]
            s1s = [shared] * n if tag.startswith("h2 = -key") else s1
            want = engine.ec_dleq_commitments(gid, kc.cs.gen, h_rand, keys, h2, scalars(kc, s1s), kc.scalar(shared), False)[1]
            got = engine.ec_keyset_dual_exp(gid, sut.set, off, scalars(kc, s1s), h2, kc.scalar(shared), False)
            assert got == want, (sut.name, n, tag, "one shared e2")
        before = engine.ec_keyset_stats()[1]
        assert engine.ec_keyset_dual_exp(gid, sut.set, off, scalars(kc, e1)) == engine.ec_batch_exp(gid, keys, scalars(kc, e1))
        assert engine.ec_keyset_stats()[1] - before == n


# ---- 3. encodings ------------------------------------------------------------------------------------------------------------
def put(arr, L, i, enc):
    return arr[:i * L] + enc + arr[(i + 1) * L:]


@pytest.mark.parametrize("name", D.NAMES)
def test_every_encoding_vector_as_a_key(engine, name):
    kc, gid, L = K.cases(name), GID[name], K.cases(name).L
    n, places = 70, (0, 35, 69)
    rng = random.Random(3)
    good = engine.ec_batch_exp_generator(gid, scalars(kc, [rng.randrange(1, kc.order) for _ in range(n)]))
    bad = EV.rejecting(name)
    assert len(bad) >= 70
    for label, enc in bad:
        for i in places:
            out = C.c_void_p(1)
            arr = put(good, L, i, enc)
            rc = engine.lib.mpvss_ec_keyset_create(engine.ctx, gid, capi.MPVSS_HOST, C.cast(C.c_char_p(arr), C.c_void_p), n, C.byref(out))
            assert rc == MPVSS_E_INVALID and out.value is None, (name, label, i)
            assert "element %d " % i in engine.last_error(), (name, label, i, engine.last_error())
    # the smallest bad index of two
    two = put(put(good, L, 69, bad[0][1]), L, 12, bad[-1][1])
    with pytest.raises(capi.EngineError, match="element 12 "):
        engine.ec_keyset_create(gid, two)
    one = kc.scalar(1)
    for label, enc, _ in EV.valid(name):
        arr = good
        for i in places:
            arr = put(arr, L, i, enc)
        with engine.ec_keyset_create(gid, arr) as ks:
            got, _ = engine.ec_keyset_twin_exp(gid, ks, 0, one * n)
        assert got == arr, (name, label)                      # 1 * y: the canonical encoding, which a valid vector is
    # the context works afterwards
    assert engine.ec_batch_exp(gid, good, one * n) == good


# ---- 4. dealer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.NAMES)
@pytest.mark.parametrize("shape", ["n3_t3", "n8_t4"])
def test_ec_deal_keyset_reproduces_the_golden_boxes(engine, name, shape):
    fx = json.load(open(os.path.join(HERE, "golden", f"{name}_{shape}.json")))
    G, gid = O.GROUPS[name](), GID[name]
    sb = G.scalar_to_fixed
    cat = lambda hs: bytes.fromhex("".join(hs))
    b = fx["box"]
    coeffs = b"".join(sb(int(c, 16)) for c in fx["inputs"]["coefficients"])
    wits = b"".join(sb(int(x, 16)) for x in fx["inputs"]["witnesses"])
    before = engine.ec_keyset_stats()
    with engine.ec_keyset_create(gid, cat(b["publickeys"])) as ks:
        d = engine.ec_deal_keyset(gid, coeffs, b["positions"], ks, 0, wits)
    n = len(b["positions"])
    assert engine.ec_keyset_stats() == (before[0] + n, before[1] + 2 * n)
    assert d["X"] == cat(fx["expected"]["X"]) and d["a1"] == cat(fx["expected"]["a1"]) and d["a2"] == cat(fx["expected"]["a2"])
    assert d["Y"] == cat(b["shares"]) and d["digest"] == bytes.fromhex(fx["expected"]["transcript_digest"])
    assert d["challenge"] == bytes.fromhex(b["challenge"]) and d["responses"] == cat(b["responses"])


def test_a_box_at_an_offset_in_a_larger_set(engine, sut):
    """n = 257, t = 5 at key_offset 3 of the set: mpvss_ec_deal on the key slice, the optional outputs NULL, two blocks in flight
    against mpvss_ec_deal_compute, and the box passes mpvss_ec_verify_distribution"""
    kc, gid, L = sut.kc, sut.gid, sut.L
    n, t, off = 257, 5, 3
    rng = random.Random(0xDEA1 + gid)
    cb = scalars(kc, [rng.randrange(kc.order) for _ in range(t)])
    wb = scalars(kc, [rng.randrange(1, kc.order) for _ in range(n)])
    pos = list(range(1, n + 1))
    keys = sut.slice(off, n)
    with engine.ec_keyset_create(gid, sut.slice(0, 300)) as ks:
        want = engine.ec_deal(gid, cb, pos, keys, wb)
        before = engine.ec_keyset_stats()[1]
        d = engine.ec_deal_keyset(gid, cb, pos, ks, off, wb)
        assert engine.ec_keyset_stats()[1] - before == 2 * n
        assert d == want
        lean = engine.ec_deal_keyset(gid, cb, pos, ks, off, wb, optional_outputs=False)
        assert (lean["Y"], lean["responses"]) == (want["Y"], want["responses"])
        assert lean["X"] is None and lean["a1"] is None and lean["a2"] is None and lean["digest"] is None
        # the box so dealt verifies
        cm = engine.ec_batch_exp_generator(gid, cb)
        res = engine.ec_verify_distribution(gid, cm, pos, keys, d["Y"], d["responses"], d["challenge"])
        assert res["verdict"] is True and res["digest"] == d["digest"]
        # two blocks in flight, absorbed in order, against the array form
        d_pos = torch.tensor(pos, dtype=torch.int64, device="cuda:0")
        d_pk, d_w = dev_u8(keys), dev_u8(wb)
        cb2 = scalars(kc, [rng.randrange(kc.order) for _ in range(t)])
        d_p = [torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        torch.cuda.synchronize()
        results = []
        for form in ("array", "keyset"):
            for k, c in enumerate((cb, cb2)):
                if form == "array":
                    engine.ec_deal_compute(gid, c, d_pos.data_ptr(), d_pk.data_ptr(), d_w.data_ptr(), n, d_p[k].data_ptr())
                else:
                    engine.ec_deal_compute_keyset(gid, c, d_pos.data_ptr(), ks, off, d_w.data_ptr(), n, d_p[2 + k].data_ptr())
            for k in range(2):
                st, X, Y, a1, a2 = engine.ec_distribute_absorb(gid, capi.transcript_init(), n)
                results.append((capi.ec_transcript_verdict(gid, st, bytes(32))[1], X, Y, a1, a2))
        assert results[2:] == results[:2] and results[0][0] == want["digest"] and results[1][0] != want["digest"]
        assert dbytes(d_p[2]) == dbytes(d_p[0]) and dbytes(d_p[3]) == dbytes(d_p[1])
        assert engine.blocks_in_flight() == (0, 0)


# ---- 5. spaces and chunks -------------------------------------------------------------------------------------------------------
def test_keys_from_device_memory_equal_keys_from_host_memory(engine, sut):
    kc, gid, L = sut.kc, sut.gid, sut.L
    n = 257
    d_keys = dev_u8(sut.slice(0, NKEYS))
    torch.cuda.synchronize()
    k1, k2 = kc.lane_scalars(n, 91), kc.lane_scalars(n, 92)
    want = engine.ec_keyset_twin_exp(gid, sut.set, 9, scalars(kc, k1), scalars(kc, k2))
    with engine.ec_keyset_create_device(gid, d_keys.data_ptr(), NKEYS) as ks:
        assert engine.ec_keyset_twin_exp(gid, ks, 9, scalars(kc, k1), scalars(kc, k2)) == want
        # scalars and results in device memory as well
        d1, d2 = dev_u8(scalars(kc, k1)), dev_u8(scalars(kc, k2))
        o1, o2 = (torch.zeros(n * L, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        torch.cuda.synchronize()
        engine._check(engine.lib.mpvss_ec_keyset_twin_exp(engine.ctx, gid, capi.MPVSS_DEVICE, ks.handle, 9, d1.data_ptr(), d2.data_ptr(), n,
                                                          o1.data_ptr(), o2.data_ptr()), "ec_keyset_twin_exp")
        assert (dbytes(o1), dbytes(o2)) == want


# The chunk of both create and twin_exp is MPVSS_MAX_CHUNK shares (2^18 unless the environment says otherwise; create caps it at
# 2^16 keys), read once per process.  A fresh child with MPVSS_MAX_CHUNK = 64 crosses both boundaries at the smallest sizes that
# do: a set of 65 keys is two build chunks (64 + 1), a twin_exp call of 65 shares two launch chunks.
CHUNK, CHUNK_N = 64, 65


def chunk_child(name):
    kc, gid = K.cases(name), GID[name]
    L = kc.L
    eng = capi.Engine(0)
    rng = random.Random(77 + gid)
    keys = eng.ec_batch_exp_generator(gid, scalars(kc, [1, 0, kc.order - 1] + [rng.randrange(2, kc.order) for _ in range(CHUNK_N - 3)]))
    k1, k2 = kc.lane_scalars(CHUNK_N, 5), kc.lane_scalars(CHUNK_N, 6)
    bad = EV.representatives(name)[0][1]
    try:
        eng.ec_keyset_create(gid, put(keys, L, CHUNK_N - 1, bad))         # the bad key sits in the second build chunk
        raise AssertionError("create accepted a bad key in the second chunk")
    except capi.EngineError as e:
        assert "element %d " % (CHUNK_N - 1) in str(e), str(e)
    with eng.ec_keyset_create(gid, keys) as ks:
        got = eng.ec_keyset_twin_exp(gid, ks, 0, scalars(kc, k1), scalars(kc, k2))
        assert got == (eng.ec_batch_exp(gid, keys, scalars(kc, k1)), eng.ec_batch_exp(gid, keys, scalars(kc, k2)))
        h2 = eng.ec_batch_exp_generator(gid, scalars(kc, k2))
        assert eng.ec_keyset_dual_exp(gid, ks, 0, scalars(kc, k1), h2, scalars(kc, k2), True) == \
            eng.ec_dleq_commitments(gid, kc.cs.gen, h2, keys, h2, scalars(kc, k1), scalars(kc, k2), True)[1]
        assert eng.ec_keyset_stats() == (CHUNK_N, 3 * CHUNK_N)
    eng.close()
    print("chunk child ok", name)


@pytest.mark.parametrize("name", D.NAMES)
def test_a_set_and_a_call_that_span_two_chunks(name):
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child", name],
                         capture_output=True, text=True, env=dict(os.environ, MPVSS_MAX_CHUNK=str(CHUNK)))
    assert out.returncode == 0 and "chunk child ok " + name in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])


# ---- 6. two sets and four threads -------------------------------------------------------------------------------------------------
def test_four_threads_over_two_sets_of_both_curves(engine):
    work = []                          # (name, gid, set, keys, k1, k2, coeffs, witnesses, positions)
    sets = []
    for name in D.NAMES:
        kc, gid = K.cases(name), GID[name]
        for which in range(2):
            rng = random.Random(100 * gid + which)
            n = 130 + 37 * which
            keys = engine.ec_batch_exp_generator(gid, scalars(kc, [rng.randrange(1, kc.order) for _ in range(n)]))
            ks = engine.ec_keyset_create(gid, keys)
            sets.append(ks)
            work.append((name, gid, ks, keys, scalars(kc, kc.lane_scalars(n, which)), scalars(kc, kc.lane_scalars(n, 50 + which)),
                         scalars(kc, [rng.randrange(kc.order) for _ in range(4)]), scalars(kc, [rng.randrange(1, kc.order) for _ in range(n)]),
                         list(range(1, n + 1))))

    def run(item):
        name, gid, ks, keys, k1, k2, cb, wb, pos = item
        return engine.ec_keyset_twin_exp(gid, ks, 0, k1, k2), engine.ec_deal_keyset(gid, cb, pos, ks, 0, wb)

    single = [run(item) for item in work]
    for item, (twin, deal) in zip(work, single):                       # the single-threaded results are the array calls'
        name, gid, ks, keys, k1, k2, cb, wb, pos = item
        assert twin == (engine.ec_batch_exp(gid, keys, k1), engine.ec_batch_exp(gid, keys, k2))
        assert deal == engine.ec_deal(gid, cb, pos, keys, wb)
    failures = []

    def worker(tid):
        try:
            for rep in range(3):
                for j in range(len(work)):
                    i = (j + tid) % len(work)
                    if run(work[i]) != single[i]:
                        failures.append((tid, rep, work[i][0], i))
        except Exception as e:      # noqa: BLE001
            failures.append((tid, repr(e)))

    threads = [threading.Thread(target=worker, args=(tid,)) for tid in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for ks in sets:
        ks.close()
    assert not failures, failures[:5]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(engine, sut):
    kc, gid, L = sut.kc, sut.gid, sut.L
    lib, n = engine.lib, 8
    other_gid = capi.GROUP_RISTRETTO255 if gid == capi.GROUP_SECP256K1 else capi.GROUP_SECP256K1
    ks_ok = scalars(kc, kc.lane_scalars(n, 1))
    e_ok = (C.c_uint8 * (n * 32)).from_buffer_copy(ks_ok)
    with_order = bytearray(ks_ok)
    with_order[5 * 32:6 * 32] = kc.order.to_bytes(32, "big" if sut.name == "secp256k1" else "little")
    e_bad = (C.c_uint8 * (n * 32)).from_buffer_copy(bytes(with_order))
    pattern = bytes([0xA5]) * (n * L)

    def fresh():
        return (C.c_uint8 * (n * L)).from_buffer_copy(pattern)

    def refused(call, needle):
        o1, o2 = fresh(), fresh()
        assert call(o1, o2) == MPVSS_E_INVALID
        assert needle in engine.last_error(), engine.last_error()
        assert bytes(o1) == pattern and bytes(o2) == pattern

    h = sut.set.handle
    twin = lambda ctx, g, hs, off, e: (lambda o1, o2: lib.mpvss_ec_keyset_twin_exp(ctx, g, capi.MPVSS_HOST, hs, off, e, e, n, o1, o2))
    dual = lambda ctx, g, hs, off, e: (lambda o1, o2: lib.mpvss_ec_keyset_dual_exp(ctx, g, capi.MPVSS_HOST, hs, off, e, None, None, 1, n, o1))
    other = capi.Engine(0)
    try:
        for mk in (twin, dual):
            o1, o2 = fresh(), fresh()
            assert mk(other.ctx, gid, h, 0, e_ok)(o1, o2) == MPVSS_E_INVALID and "another context" in other.last_error()
            assert bytes(o1) == pattern and bytes(o2) == pattern
            refused(mk(engine.ctx, other_gid, h, 0, e_ok), "other curve")
            refused(mk(engine.ctx, gid, h, NKEYS - n + 1, e_ok), "beyond the set")
            refused(mk(engine.ctx, gid, h, NKEYS + 1, e_ok), "beyond the set")
            refused(mk(engine.ctx, gid, None, 0, e_ok), "none given")
            refused(mk(engine.ctx, gid, h, 0, e_bad), "scalar 5 ")
    finally:
        other.close()
    # the dealer's forms: a set of the other curve, an offset beyond the set
    pos = (C.c_int64 * n)(*range(1, n + 1))
    cb = (C.c_uint8 * 64).from_buffer_copy(scalars(kc, [3, 4]))
    y, r = fresh(), (C.c_uint8 * (n * 32))()
    assert lib.mpvss_ec_deal_keyset(engine.ctx, other_gid, cb, 2, pos, h, 0, e_ok, n, None, y, None, None, None, None, r) == MPVSS_E_INVALID
    assert lib.mpvss_ec_deal_keyset(engine.ctx, gid, cb, 2, pos, h, NKEYS - 1, e_ok, n, None, y, None, None, None, None, r) == MPVSS_E_INVALID
    assert bytes(y) == pattern and bytes(r) == bytes(n * 32)
    d_w = dev_u8(ks_ok)
    d_pos = torch.tensor(list(range(1, n + 1)), dtype=torch.int64, device="cuda:0")
    d_p = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.mpvss_ec_deal_compute_keyset(engine.ctx, gid, cb, 2, d_pos.data_ptr(), h, NKEYS, d_w.data_ptr(), n, d_p.data_ptr(), None, None,
                                            None, None) == MPVSS_E_INVALID
    assert engine.blocks_in_flight() == (0, 0)
    # create: n == 0, a null pointer
    keys = (C.c_uint8 * (n * L)).from_buffer_copy(sut.slice(0, n))
    for args in ((keys, 0), (None, n)):
        out = C.c_void_p(1)
        assert lib.mpvss_ec_keyset_create(engine.ctx, gid, capi.MPVSS_HOST, args[0], args[1], C.byref(out)) == MPVSS_E_INVALID
        assert out.value is None
    assert lib.mpvss_ec_keyset_create(engine.ctx, gid, capi.MPVSS_HOST, keys, n, None) == MPVSS_E_INVALID
    # n == 0 of the powers: nothing to do, as in the array calls
    assert lib.mpvss_ec_keyset_twin_exp(engine.ctx, gid, capi.MPVSS_HOST, h, 0, None, None, 0, None, None) == 0
    # the context works afterwards
    got, _ = engine.ec_keyset_twin_exp(gid, sut.set, 0, ks_ok)
    assert got == engine.ec_batch_exp(gid, sut.slice(0, n), ks_ok)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "child":
    chunk_child(sys.argv[2])
