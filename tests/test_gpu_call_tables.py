"""Call tables (mpvss_ctx_set_call_tables, on by default): the boxes of one mpvss_modp_verify_many call that present the same
device-resident key array share two rows of 64 powers per key, built once per call; their a2 = y^r * Y^c takes
k_modp_rows2_dual_exp_pair.  Verdicts, digests and a2 bytes must be those of the plain path; the counters say which boxes were served.
Smallest boxes that reach the path: n = 16 385 and 16 415 (n % 32 != 0), t = 8 (Horner X path, fixed windows of c) and t = 64
(forward differences, the host's sliding-window schedule of c)."""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import pytest

import mpvss_oracle as O
from helpers import EB
from mpvss_rs_amd import capi

pytestmark = pytest.mark.gpu
Q = O.ModpGroup().q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fx(v):
    return v.to_bytes(EB, "big")


def flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


class Deck:
    """dealers' boxes against key arrays in HBM; run(specs) -> [(verdict, digest)] through mpvss_modp_verify_many"""

    def __init__(self, engine, n, t, seed):
        import torch
        self.torch, self.engine, self.n, self.t = torch, engine, n, t
        self.rng = random.Random(seed)
        self.pos = list(range(3, 3 + n))
        self.d_pos = torch.tensor(self.pos, dtype=torch.int64, device="cuda:0")
        self.keep = []

    def sc(self, k):
        return b"".join(self.rng.randrange(1, 1 << 2040).to_bytes(EB, "big") for _ in range(k))

    def dev(self, b):
        d = self.torch.frombuffer(bytearray(b), dtype=self.torch.uint8).to("cuda:0")
        self.keep.append(d)
        return d

    def keys(self):
        pk = self.engine.batch_exp_fixed_base(fx(2), self.sc(self.n))
        return dict(host=pk, dev=self.dev(pk))

    def deal(self, keys):
        coeffs = self.sc(self.t)
        d = self.engine.deal(coeffs, self.pos, keys["host"], self.sc(self.n))
        return dict(keys=keys, cm=self.engine.batch_exp_fixed_base(fx(4), coeffs), Y=d["Y"], r=d["responses"], c=d["challenge"],
                    digest=d["digest"])

    def array(self, specs):
        arr = (capi.ModpBox * len(specs))()
        for i, b in enumerate(specs):
            bufs = [self.dev(b[k]) for k in ("cm", "Y", "r")]
            ch = (C.c_uint8 * EB).from_buffer_copy(b["c"])
            self.keep.append(ch)
            arr[i] = capi.ModpBox(bufs[0].data_ptr(), self.t, self.d_pos.data_ptr(), b["keys"]["dev"].data_ptr(), bufs[1].data_ptr(),
                                  bufs[2].data_ptr(), self.n, C.cast(ch, C.c_void_p), None, 0)
        self.torch.cuda.synchronize()
        return arr

    def run(self, arr, depth=4, threads=3, chained=False, engine=None):
        eng = engine or self.engine
        k = len(arr)
        verdicts, digests = (C.c_int * k)(), (C.c_uint8 * (32 * k))()
        if chained:
            rc = eng.lib.mpvss_modp_verify_many_chained(eng.ctx, capi.MPVSS_DEVICE, arr, k, depth, threads, None, capi.CHAIN_CB(0), capi.CHAIN_CB(0),
                                                        None, verdicts, C.cast(digests, C.c_void_p))
        else:
            rc = eng.lib.mpvss_modp_verify_many(eng.ctx, capi.MPVSS_DEVICE, arr, k, depth, threads, verdicts, C.cast(digests, C.c_void_p))
        eng._check(rc, "verify_many")
        raw = bytes(digests)
        return [(bool(verdicts[i]), raw[32 * i:32 * i + 32]) for i in range(k)]


def served(engine, fn):
    b0, s0 = engine.call_tables_stats()
    out = fn()
    b1, s1 = engine.call_tables_stats()
    return out, (b1 - b0, s1 - s0)


@pytest.fixture(scope="module", params=[(16385, 8), (16415, 64)], ids=["n16385_t8_horner", "n16415_t64_fd"])
def deck(request, engine):
    n, t = request.param
    dk = Deck(engine, n, t, seed=n + t)
    dk.A, dk.B = dk.keys(), dk.keys()
    dk.d = [dk.deal(dk.A) for _ in range(4)]
    dk.dB = dk.deal(dk.B)
    assert engine.set_call_tables(3) in (0, 3)
    yield dk
    engine.set_call_tables(3)


def test_dealers_against_one_key_array(engine, deck):
    """three and four dealers' boxes: same verdicts and digests off and on; one build per call, every box served; two boxes: no build"""
    for k in (3, 4):
        arr = deck.array(deck.d[:k])
        assert engine.set_call_tables(0) == 3
        plain, st = served(engine, lambda: deck.run(arr))
        assert st == (0, 0)
        assert plain == [(True, b["digest"]) for b in deck.d[:k]]
        assert engine.set_call_tables(3) == 0
        fd0 = engine.fd_stats()
        on, st = served(engine, lambda: deck.run(arr))
        assert on == plain and st == (1, k)
        if deck.t >= 16:
            fd1 = engine.fd_stats()
            assert (fd1[0] - fd0[0], fd1[1] - fd0[1]) == (k, 0)          # the X path is the plain path's: forward differences, held
    two, st = served(engine, lambda: deck.run(deck.array(deck.d[:2])))
    assert st == (0, 0) and two == [(True, b["digest"]) for b in deck.d[:2]]
    assert engine.blocks_in_flight() == (0, 0)


def test_mixed_call_keeps_verdicts_digests_and_paths(engine, deck):
    """a flipped response bit, a flipped share bit, a challenge above 256 bits and a second key array carried by one box, inside a
    served call: verdicts and digests of the plain path; the wide challenge and the second array go the plain way (not served)"""
    d = deck.d
    n = deck.n
    specs = [d[0], dict(d[1], r=flip(d[1]["r"], (n - 1) * EB + 255)), d[1], deck.dB, dict(d[2], Y=flip(d[2]["Y"], 77 * EB + 3)),
             dict(d[0], c=fx((1 << 300) + 5)), d[2]]
    arr = deck.array(specs)
    engine.set_call_tables(0)
    plain, st = served(engine, lambda: deck.run(arr))
    assert st == (0, 0)
    assert [v for v, _ in plain] == [True, False, True, True, False, False, True]
    assert plain[0][1] == d[0]["digest"] and plain[3][1] == deck.dB["digest"]
    engine.set_call_tables(3)
    on, st = served(engine, lambda: deck.run(arr))
    assert on == plain
    assert st == (1, 5)                     # all of A's boxes but the one with the wide challenge; B's box is alone with its array
    chained, st = served(engine, lambda: deck.run(arr, chained=True))
    assert chained == plain and st == (1, 5)


def test_a2_bytes_of_edge_exponents(engine, deck):
    """responses 0, 1, q - 2, 2^B - 1, 2^B, 2^B + 1, 2^(2048 - B), all ones, all-zero rows (B = 1024), keys 1 and q - 1, in the first
    wave, across the 16 384 boundary and in the ragged last wave.  The one-box block entry point is the only one that hands a2 out, and
    it never gets call rows: the bytes compared with Python's pow are the PLAIN kernel's.  The new kernel's a2 is pinned through the
    served call's digest, the SHA-256 over every X, Y, a1, a2 byte of the box, which must be the digest of exactly those bytes (and
    of the same call with the feature off) -- sound, but a mismatch names the box, not the share."""
    n, B = deck.n, 1024
    ones = (1 << 2048) - 1
    edge = [0, 1, Q - 2, (1 << B) - 1, 1 << B, (1 << B) + 1, 1 << (2048 - B), ones, ((1 << B) - 1) << B, 1 << 2047,
            sum(63 << (12 * k) for k in range(170)), (1 << 1020) - 1, 1 << 1020, 63 << 1020]
    at = [0, 1, 2, 31, 32, 33, 63, 64, 65, 8191, 16383, 16384, n - 2, n - 1]
    rng = random.Random(n)
    keys = [pow(2, rng.randrange(Q - 1), Q) for _ in range(40)]
    keys = [keys[rng.randrange(40)] * pow(2, i, Q) % Q for i in range(n)]
    keys[5], keys[6], keys[n - 3] = 1, Q - 1, Q - 1
    pk = b"".join(map(fx, keys))
    K = dict(host=pk, dev=deck.dev(pk))
    resp = bytearray(rng.randbytes(EB * n))
    for i, e in zip(at, edge):
        resp[i * EB:(i + 1) * EB] = fx(e)
    resp[5 * EB:6 * EB] = fx(Q - 2)
    resp[6 * EB:7 * EB] = fx(ones)
    shares = rng.randbytes(EB * n)
    cm = b"".join(fx(pow(4, rng.randrange(Q - 1), Q)) for _ in range(deck.t))
    boxes = [dict(keys=K, cm=cm, Y=shares, r=bytes(resp), c=fx(c)) for c in (rng.randrange(1 << 256), (1 << 256) - 1, 1)]
    arr = deck.array(boxes)
    engine.set_call_tables(3)
    on, st = served(engine, lambda: deck.run(arr))
    assert st == (1, 3)
    engine.set_call_tables(0)
    assert deck.run(arr) == on
    engine.set_call_tables(3)
    for b, (_, digest) in zip(boxes, on):
        engine.verify_block_compute(cm, deck.pos, pk, shares, b["r"], b["c"])
        st_, _, _, A2 = engine.verify_block_absorb_dump(capi.transcript_init(), n)
        assert capi.transcript_verdict(st_, b["c"])[1] == digest
        c = int.from_bytes(b["c"], "big")
        for i in at + [5, 6, n - 3]:
            Y = int.from_bytes(shares[i * EB:(i + 1) * EB], "big")
            r = int.from_bytes(b["r"][i * EB:(i + 1) * EB], "big")
            assert int.from_bytes(A2[i * EB:(i + 1) * EB], "big") == pow(keys[i], r, Q) * pow(Y, c, Q) % Q, i


def test_two_threads_on_one_context(engine, deck):
    arr = [deck.array(deck.d[:3]), deck.array(deck.d[1:4])]
    want = [[(True, b["digest"]) for b in deck.d[:3]], [(True, b["digest"]) for b in deck.d[1:4]]]
    res = [None, None]

    def work(k):
        res[k] = [deck.run(arr[k]) for _ in range(2)]
    ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [th.start() for th in ths]
    [th.join() for th in ths]
    assert res[0] == [want[0]] * 2 and res[1] == [want[1]] * 2
    assert engine.blocks_in_flight() == (0, 0)


def test_switches(engine, deck):
    """mpvss_ctx_set_call_tables(ctx, 0): no build, the buffer is given back; 1 and negatives are refused; MPVSS_CALL_TABLES=0 in the
    environment: off for a fresh context of a fresh process (default there: 0, here: 3)"""
    arr = deck.array(deck.d[:3])
    torch = deck.torch
    _, st = served(engine, lambda: deck.run(arr))
    assert st == (1, 3)
    torch.cuda.synchronize()
    held = torch.cuda.mem_get_info()[0]
    assert engine.set_call_tables(0) == 3
    assert torch.cuda.mem_get_info()[0] - held > 0.9 * deck.n * 2 * 64 * 288        # two rows of 64 entries of 288 bytes per key
    _, st = served(engine, lambda: deck.run(arr))
    assert st == (0, 0)
    with pytest.raises(capi.EngineError):
        engine.set_call_tables(1)
    with pytest.raises(capi.EngineError):
        engine.set_call_tables(-2)
    assert engine.set_call_tables(3) == 0
    if deck.t != 8:
        return                              # one child process is enough
    code = ("import sys; [sys.path.insert(0, p) for p in %r]\n"
            "import torch\n"
            "from mpvss_rs_amd import Engine\n"
            "from test_gpu_call_tables import Deck, served\n"
            "e = Engine(0)\n"
            "dk = Deck(e, 16385, 8, 1)\n"
            "A = dk.keys()\n"
            "boxes = [dk.deal(A) for _ in range(3)]\n"
            "arr = dk.array(boxes)\n"
            "out, st = served(e, lambda: dk.run(arr))\n"
            "assert out == [(True, b['digest']) for b in boxes], out\n"
            "print('default', e.set_call_tables(3), 'stats', st)\n" % [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")])
    for env, want in (({"MPVSS_CALL_TABLES": "0"}, "default 0 stats (0, 0)"), ({}, "default 3 stats (1, 3)")):
        full = dict(os.environ, **env)
        if not env:
            full.pop("MPVSS_CALL_TABLES", None)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=full)
        assert out.returncode == 0 and want in out.stdout, out.stdout + out.stderr[-2000:]
