"""The tail of a large box AMONG OTHERS -- X's table, a1 = g^r X^c, the output copies and the slot's completion event -- runs on the
slot's second stream behind an event recorded after the last kernel of the X path (verify_block_compute_locked in mpvss_capi.cpp);
a box that has the chip to itself keeps everything on its first stream.  Only the schedule differs, so every case here is compared
byte for byte with the same box verified ALONE by mpvss_modp_verify_distribution (the unchanged path, which the rest of the suite
pins to the oracle): verdict and digest for the calls that return those (the digest is the SHA-256 over every X, Y, a1 and a2 byte
of the box), X, a1 and a2 themselves where the entry point hands them out (the block API with three and more blocks in flight, the
one-box callers beside a pipeline).

Shapes: n = 16 400, t = 16 is the smallest box that is not grouped (n > 16 384) and takes the forward differences; 16 400 is neither
a multiple of 32 (ragged last pair wave) nor of 16 S = 64 (ragged last chain).  n = 20 000, t = 17 is the second shape of the slot
reuse case."""
import os
import pickle
import subprocess
import sys
import threading

import pytest

from helpers import EB
from mpvss_rs_amd import capi
from test_gpu_call_tables import Deck, fx, flip, served

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 16400, 16
NOTHING = (False, bytes(32))          # a malformed box: no transcript


@pytest.fixture(scope="module")
def deck(engine):
    dk = Deck(engine, N, T, seed=N + T)
    dk.A = dk.keys()
    dk.d = [dk.deal(dk.A) for _ in range(5)]
    dk.lone = {}
    assert engine.set_call_tables(3) in (0, 3)
    yield dk
    engine.set_call_tables(3)
    engine.set_key_cache_lru(0)


def alone(engine, dk, b):
    """the box by itself through mpvss_modp_verify_distribution: (verdict, digest, X, a1, a2), computed once per box"""
    key = (b["cm"], b["Y"], b["r"], b["c"])
    if key not in dk.lone:
        assert engine.blocks_in_flight() == (0, 0)
        r = engine.verify_distribution(b["cm"], dk.pos, b["keys"]["host"], b["Y"], b["r"], b["c"], dump=True)
        dk.lone[key] = (r["verdict"], r["digest"], r["X"], r["a1"], r["a2"])
    return dk.lone[key]


def edges(d):
    """challenge edges: 0 (no schedule: the number_tables branch), 1, the top bit of 256 set, more than 256 bits (512 windows)"""
    return [dict(d[0], c=fx(0)), dict(d[1], c=fx(1)), dict(d[2], c=fx((1 << 255) | 0x1234567)), dict(d[3], c=fx((1 << 300) + 12345))]


def test_large_boxes_among_others_with_and_without_call_tables(engine, deck):
    specs = deck.d[:4] + edges(deck.d)
    want = [alone(engine, deck, b)[:2] for b in specs]
    assert want[:4] == [(True, b["digest"]) for b in deck.d[:4]] and [v for v, _ in want[4:]] == [False] * 4
    arr = deck.array(specs)
    f0 = engine.fd_stats()
    on, st = served(engine, lambda: deck.run(arr, depth=4))
    assert on == want
    assert st == (1, 6)          # rows for the four dealers' boxes, c = 1 and the top bit; c = 0 and the wide c take the plain kernels
    engine.set_call_tables(len(specs) + 1)          # fewer boxes than the threshold: the plain w6 kernel and tab1
    plain, st = served(engine, lambda: deck.run(arr, depth=4))
    engine.set_call_tables(3)
    assert plain == want and st == (0, 0)
    f1 = engine.fd_stats()
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (2 * len(specs), 0)
    assert engine.blocks_in_flight() == (0, 0)


def test_tampered_and_malformed_boxes_leave_their_neighbours_alone(engine, deck):
    d = deck.d
    specs = [d[0], dict(d[1], r=flip(d[1]["r"], (N - 1) * EB + 255)), d[2], d[3], dict(d[3], Y=flip(d[3]["Y"], 77 * EB + 3)), d[4]]
    want = [alone(engine, deck, b)[:2] for b in specs]
    assert [v for v, _ in want] == [True, False, True, True, False, True]
    arr = deck.array(specs)
    arr[3].t = 0                                     # malformed, in the middle of the call
    lone_bad = deck.array([d[3]])
    lone_bad[0].t = 0
    assert deck.run(lone_bad) == [NOTHING]
    want[3] = NOTHING
    assert deck.run(arr, depth=4) == want
    assert engine.blocks_in_flight() == (0, 0)


def blocks_among_others(engine, dk, specs):
    """the block API with every block enqueued before the first is absorbed: from the third on a block is a box among others.
    specs: (box, key set or None).  Returns (verdict, digest, X, a1, a2) per block."""
    for b, ks in specs:
        if ks is None:
            engine.verify_block_compute(b["cm"], dk.pos, b["keys"]["host"], b["Y"], b["r"], b["c"])
        else:
            engine.verify_block_compute_keyset(b["cm"], dk.pos, ks, 0, b["Y"], b["r"], b["c"])
    out = []
    for b, _ in specs:
        st, X, a1, a2 = engine.verify_block_absorb_dump(capi.transcript_init(), dk.n)
        out.append(tuple(capi.transcript_verdict(st, b["c"])) + (X, a1, a2))
    return out


def test_x_a1_a2_bytes_of_blocks_among_others(engine, deck):
    specs = [deck.d[4], deck.d[3]] + deck.d[:3] + edges(deck.d)
    want = [alone(engine, deck, b) for b in specs]
    got = blocks_among_others(engine, deck, [(b, None) for b in specs])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[:2] == w[:2], i
        for k, name in ((2, "X"), (3, "a1"), (4, "a2")):
            assert g[k] == w[k], (i, name)
    assert engine.blocks_in_flight() == (0, 0)


def test_registered_keys_among_others(engine, deck):
    """registered keys take the pair-layout tail (short_tail): through a key set handed in, and through the cross-call key cache of
    the one-box entry point (mpvss_ctx_set_key_cache_lru) beside a pipeline"""
    d = deck.d
    want = [alone(engine, deck, b) for b in d[:4]]
    ks = engine.keyset_create(deck.A["host"])
    try:
        got = blocks_among_others(engine, deck, [(d[0], None), (d[1], ks), (d[2], ks), (d[3], ks)])
    finally:
        engine.keyset_destroy(ks)
    assert got == want
    arr = deck.array(d[:4])
    assert engine.set_key_cache_lru(2, 1) == 0
    res = {}

    def caller():
        res["one"] = [engine.verify_distribution(b["cm"], deck.pos, b["keys"]["host"], b["Y"], b["r"], b["c"], dump=True) for b in d[:4]]

    def pipeline():
        res["many"] = deck.run(arr, depth=3)
    try:
        ths = [threading.Thread(target=f) for f in (caller, pipeline)]
        [th.start() for th in ths]
        [th.join() for th in ths]
    finally:
        engine.set_key_cache_lru(0)
    assert [(r["verdict"], r["digest"], r["X"], r["a1"], r["a2"]) for r in res["one"]] == want
    assert res["many"] == [w[:2] for w in want]
    assert engine.blocks_in_flight() == (0, 0)


def test_slots_are_reused_with_two_shapes(engine, deck):
    """21 boxes through depth 3, the shapes alternating: every slot's streams and workspaces are reused, and grow, several times"""
    big = Deck(engine, 20000, 17, seed=20017)
    big.lone = {}
    kb = big.keys()
    db = [big.deal(kb) for _ in range(3)]
    a_small, a_big = deck.array(deck.d[:3]), big.array(db)
    count = 21
    arr = (capi.ModpBox * count)()
    want = []
    for i in range(count):
        src, boxes = ((a_small, deck.d), (a_big, db))[i % 2]
        arr[i] = src[(i // 2) % 3]
        want.append((True, boxes[(i // 2) % 3]["digest"]))
    assert alone(engine, big, db[0])[:2] == want[1]
    engine.pipeline_stats(reset=True)
    f0 = engine.fd_stats()
    assert deck.run(arr, depth=3) == want
    f1 = engine.fd_stats()
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (count, 0)
    assert engine.pipeline_stats()["blocks"] == count
    assert engine.blocks_in_flight() == (0, 0)


def test_one_box_callers_beside_a_pipeline(engine, deck):
    """two threads of one-box callers beside a verify_many call on one context: whether a box finds others in flight changes from
    box to box; every result is the sequential one, dumps included"""
    d = deck.d
    seq = [d[0], dict(d[1], r=flip(d[1]["r"], 9 * EB + 1)), d[2], edges(d)[3]]
    want = [alone(engine, deck, b) for b in seq]
    arr = deck.array([d[3], d[4], d[0], d[1], d[2], d[3]])
    want_many = [alone(engine, deck, b)[:2] for b in (d[3], d[4], d[0], d[1], d[2], d[3])]
    res, errs = {}, []

    def caller(k):
        def run():
            try:
                out = []
                for b in (seq if k == 0 else seq[::-1]):
                    r = engine.verify_distribution(b["cm"], deck.pos, b["keys"]["host"], b["Y"], b["r"], b["c"], dump=True)
                    out.append((r["verdict"], r["digest"], r["X"], r["a1"], r["a2"]))
                res[k] = out
            except BaseException as exc:  # noqa: BLE001 - reported below
                errs.append(exc)
        return run

    def pipeline():
        try:
            res["many"] = [deck.run(arr, depth=4) for _ in range(2)]
        except BaseException as exc:  # noqa: BLE001
            errs.append(exc)
    ths = [threading.Thread(target=f) for f in (caller(0), caller(1), pipeline)]
    [th.start() for th in ths]
    [th.join() for th in ths]
    assert not errs, errs
    assert res[0] == want and res[1] == want[::-1]
    assert res["many"] == [want_many] * 2
    assert engine.blocks_in_flight() == (0, 0)


# what a child process does with three of the deck's boxes (dealt by the parent, handed over in a file): one verify_many call, then
# each box in a call of its own
CHILD = r'''
import pickle, sys
[sys.path.insert(0, p) for p in %r]
import torch
from mpvss_rs_amd import Engine
from test_gpu_call_tables import Deck
e = Engine(0)
dk = Deck(e, 16400, 16, 7)
data = pickle.load(open(sys.argv[1], "rb"))
A = dict(host=data["pk"], dev=dk.dev(data["pk"]))
boxes = [dict(b, keys=A) for b in data["boxes"]]
arr = dk.array(boxes)
f0 = e.fd_stats()
together = dk.run(arr, depth=4)
f1 = e.fd_stats()
lone = [dk.run(dk.array([b]))[0] for b in boxes]
assert together == lone, "among others against alone"
assert together == [(True, b["digest"]) for b in boxes], "verdicts / dealers' digests"
assert e.blocks_in_flight() == (0, 0)
print("fd", f1[0] - f0[0], f1[1] - f0[1])
'''


@pytest.fixture(scope="module")
def handed_over(deck, tmp_path_factory):
    path = tmp_path_factory.mktemp("closing") / "boxes.pickle"
    with open(path, "wb") as f:
        pickle.dump(dict(pk=deck.A["host"], boxes=[{k: b[k] for k in ("cm", "Y", "r", "c", "digest")} for b in deck.d[:3]]), f)
    return str(path)


def child(path, env):
    code = CHILD % [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    out = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    return out.stdout.strip().split("\n")[-1]


@pytest.mark.parametrize("level", ["1", "2"])
def test_tail_reads_the_gated_horner_fallback(handed_over, level):
    """a stage of the stepping gives up (MPVSS_FD_TEST_FAULT): the gated Horner kernel writes X on the first stream, ahead of the
    event the tail waits for; verdicts and digests are the dealers', the fall-back counter moves"""
    assert child(handed_over, {"MPVSS_FD_TEST_FAULT": level}) == "fd 3 3"


def test_box_of_several_chunks_among_others(handed_over):
    """MPVSS_MAX_CHUNK=8192: 16 400 shares are three chunks (8 192, 8 192 and 16, the last one below the forward differences'
    minimum, so the box closes on both streams in turn); the chunks synchronise on the stream that closed them"""
    assert child(handed_over, {"MPVSS_MAX_CHUNK": "8192"}) == "fd 3 0"
