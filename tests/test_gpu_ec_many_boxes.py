"""mpvss_ec_verify_many over runs of small boxes (one dense batch, k_*_commit_eval_tiles): every (verdict, digest) against
mpvss_ec_verify_distribution box by box on the same engine, honest boxes against the dealer's digest from mpvss_ec_deal as well.
Both curves.  The shapes and the model of the run rule are in tests/ec_many_boxes_cases.py.

(1) every edge of a tile in one call, t = 1 .. 17, mixed shapes in one run; (2) positions 0, 1, scattered, 2^40, negative;
(3) what splits a run, and the stats; (4) tampers inside a run cost only their box, with the one-box call's message; (5) every
box's arrays in HBM at odd addresses (k_ec_gather_segments); (6) mode 0; (7) pass boundaries in a fresh child process with
MPVSS_MAX_CHUNK=32 (read once per process) -- this file is its own child: `python test_gpu_ec_many_boxes.py child <curve>
<boxes.json>`; (8) a one-box call of n = 513 and a grouped call over the same workspace, in both orders.

Measured on an MI355X: 16 tests in 3.4 s; pass_boundaries (two children) 1.4 s, every other test below 0.5 s."""
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import ec_many_boxes_cases as MB
import encoding_vectors as EV
import mpvss_oracle as O

pytestmark = pytest.mark.gpu
CURVES = ["secp256k1", "ristretto255"]
GID = {"secp256k1": 1, "ristretto255": 2}
STATS = ("passes", "grouped_boxes", "single_boxes")
FIELDS = ("commitments", "pubkeys", "shares", "responses")
REFUSED = (False, bytes(32))
_BOXES = {}


def deal(engine, name, n, t, seed, positions=None):
    """(box, dealer's digest): an honest box of (n, t) made by the engine's dealer from seeded randomness (made once per shape)"""
    key = (name, n, t, seed, tuple(positions) if positions is not None else None)
    if key not in _BOXES:
        G, gid = O.GROUPS[name](), GID[name]
        rng = random.Random(seed)
        order = G.group_order_int()
        sc = lambda k: b"".join(G.scalar_to_fixed(rng.randrange(1, order)) for _ in range(k))
        coeffs, privs, ws = sc(t), sc(n), sc(n)
        pubkeys = engine.ec_batch_exp_generator(gid, privs)
        pos = list(positions) if positions is not None else list(range(1, n + 1))
        d = engine.ec_deal(gid, coeffs, pos, pubkeys, ws)
        box = dict(commitments=engine.ec_batch_exp_generator(gid, coeffs), positions=pos, pubkeys=pubkeys, shares=d["Y"],
                   responses=d["responses"], challenge=d["challenge"])
        _BOXES[key] = (box, d["digest"])
    return _BOXES[key]


def one(engine, name, box):
    """the one-box call as the many-box call reports it: (verdict, digest), or the refusal with the message"""
    from mpvss_rs_amd import capi
    try:
        r = engine.ec_verify_distribution(GID[name], box["commitments"], box["positions"], box["pubkeys"], box["shares"],
                                          box["responses"], box["challenge"])
    except capi.EngineError as e:
        assert "rc=-1" in str(e)
        return REFUSED, str(e)
    return (r["verdict"], r["digest"]), None


def delta(engine, fn):
    s0 = engine.ec_verify_many_stats()
    out = fn()
    s1 = engine.ec_verify_many_stats()
    return out, tuple(s1[k] - s0[k] for k in STATS)


def honest(engine, name, shapes, seed0):
    boxes, want = [], []
    for k, s in enumerate(shapes):
        box, digest = deal(engine, name, s.n, s.t, seed0 + k)
        boxes.append(box)
        want.append((True, digest))
    return boxes, want


def flip(data, byte, bit=1):
    b = bytearray(data)
    b[byte] ^= bit
    return bytes(b)


# ---- (1) tile edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_tile_edges_in_one_call(engine, name):
    boxes, want = honest(engine, name, MB.TILE_SHAPES, 100)
    assert [one(engine, name, b)[0] for b in boxes] == want
    got, d = delta(engine, lambda: engine.ec_verify_many(GID[name], boxes))
    assert got == want, [k for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert d == (1, len(boxes), 0)
    assert engine.ec_verify_many(GID[name], boxes[::-1]) == want[::-1]
    for depth, threads in ((1, 1), (4, 2), (16, 64), (0, 0)):
        assert engine.ec_verify_many(GID[name], boxes, depth=depth, hash_threads=threads) == want


# ---- (2) positions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_positions(engine, name):
    boxes, want = [], []
    for k, (pos, t) in enumerate(zip(MB.POSITION_LISTS, MB.POSITION_T)):
        box, digest = deal(engine, name, len(pos), t, 200 + k, pos)
        boxes.append(box)
        want.append((True, digest))
    assert [one(engine, name, b)[0] for b in boxes] == want
    got, d = delta(engine, lambda: engine.ec_verify_many(GID[name], boxes))
    assert got == want and d == (1, len(boxes), 0)
    # the positions are part of the statement: another list under the same proof is answered as the one-box call answers it
    moved = dict(boxes[1], positions=boxes[1]["positions"][::-1])
    w = one(engine, name, moved)[0]
    assert w[0] is False and w[1] != want[1][1]
    assert engine.ec_verify_many(GID[name], [boxes[0], moved, boxes[3]]) == [want[0], w, want[3]]


# ---- (3) what splits a run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_what_splits_a_run(engine, name):
    G, gid = O.GROUPS[name](), GID[name]
    (a, b, c, e), want = honest(engine, name, [MB.Shape(5, 3), MB.Shape(7, 2), MB.Shape(5, 3), MB.Shape(66, 3)], 300)
    empty = dict(commitments=a["commitments"], positions=[], pubkeys=b"", shares=b"", responses=b"", challenge=a["challenge"])
    w_empty = one(engine, name, empty)[0]
    assert w_empty[1] != bytes(32)                                              # the empty transcript has a digest
    got, d = delta(engine, lambda: engine.ec_verify_many(gid, [a, b, empty, c, e]))
    assert got == [want[0], want[1], w_empty, want[2], want[3]] and d == (2, 4, 0)
    null = dict(b, pubkeys=None)
    got, d = delta(engine, lambda: engine.ec_verify_many(gid, [a, b, null, c, e]))
    assert got == [want[0], want[1], REFUSED, want[2], want[3]] and d == (2, 4, 0)
    big = G.group_order_int().to_bytes(32, "big" if name == "secp256k1" else "little")
    got, d = delta(engine, lambda: engine.ec_verify_many(gid, [a, b, dict(c, challenge=big), e]))
    assert got == [want[0], want[1], REFUSED, want[3]] and d == (1, 2, 1)      # e is a run of one
    assert "challenge: scalar 0" in engine.last_error()
    assert delta(engine, lambda: engine.ec_verify_many(gid, [e])) == ([want[3]], (0, 0, 1))
    assert delta(engine, lambda: engine.ec_verify_many(gid, [empty, null])) == ([w_empty, REFUSED], (0, 0, 0))
    assert delta(engine, lambda: engine.ec_verify_many(gid, [])) == ([], (0, 0, 0))


# ---- (4) tampers inside a run ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_tampers_cost_only_their_box(engine, name):
    G, gid = O.GROUPS[name](), GID[name]
    L = G.elem_len
    (a, b, c), want = honest(engine, name, [MB.Shape(5, 3), MB.Shape(70, 4), MB.Shape(9, 2)], 400)
    bad_enc = EV.rejecting(name)[0][1]
    assert len(bad_enc) == L
    put = lambda data, i, e, w: data[:i * w] + e + data[(i + 1) * w:]
    big = G.group_order_int().to_bytes(32, "big" if name == "secp256k1" else "little")
    # (a flipped share bit may leave the encoding: then the one-box call names the share, and so must the run)
    tampers = [("response bit", dict(b, responses=flip(b["responses"], 32 * 66 + 31 if name == "secp256k1" else 32 * 66)), None),
               ("share bit", dict(b, shares=flip(b["shares"], 65 * L + 5)), "encrypted shares: element 65"),
               ("commitment", dict(b, commitments=put(b["commitments"], 2, bad_enc, L)), "commitments: element 2"),
               ("public key", dict(b, pubkeys=put(b["pubkeys"], 64, bad_enc, L)), "public keys: element 64"),
               ("share", dict(b, shares=put(b["shares"], 69, bad_enc, L)), "encrypted shares: element 69"),
               ("response >= order", dict(b, responses=put(b["responses"], 1, big, 32)), "responses: scalar 1")]
    for what, box, msg in tampers:
        w, err = one(engine, name, box)
        assert what.endswith("bit") or w == REFUSED, what
        got, d = delta(engine, lambda: engine.ec_verify_many(gid, [a, box, c]))
        assert got == [want[0], w, want[2]], what
        if w == REFUSED:
            assert msg in err and msg in engine.last_error(), (what, err, engine.last_error())
            assert d == (1, 2, 0), what
        else:
            assert w[0] is False and w[1] != want[1][1] and d == (1, 3, 0), what
    # several boxes turned down in one run: the message is that of the last in box order
    got = engine.ec_verify_many(gid, [tampers[3][1], a, tampers[2][1], c])
    assert got == [REFUSED, want[0], REFUSED, want[2]] and "commitments: element 2" in engine.last_error()
    got = engine.ec_verify_many(gid, [tampers[2][1], a, tampers[3][1]], hash_threads=3)
    assert got == [REFUSED, want[0], REFUSED] and "public keys: element 64" in engine.last_error()
    # a box with a bad response AND a bad public key: the response is named, as by the absorbing call
    both = dict(tampers[5][1], pubkeys=tampers[3][1]["pubkeys"])
    assert "responses: scalar 1" in one(engine, name, both)[1]
    assert engine.ec_verify_many(gid, [a, both]) == [want[0], REFUSED] and "responses: scalar 1" in engine.last_error()


# ---- (5) device space --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_boxes_in_hbm(engine, name):
    import numpy as np
    import torch
    G, gid = O.GROUPS[name](), GID[name]
    L = G.elem_len
    shapes = [MB.Shape(5, 3), MB.Shape(65, 17), MB.Shape(1, 1), MB.Shape(128, 2), MB.Shape(63, 3)]
    boxes, want = honest(engine, name, shapes, 500)
    boxes[3] = dict(boxes[3], shares=flip(boxes[3]["shares"], 100 * L + 7))
    boxes.append(dict(boxes[0], pubkeys=boxes[0]["pubkeys"][:L] + EV.rejecting(name)[0][1] + boxes[0]["pubkeys"][2 * L:]))
    host = engine.ec_verify_many(gid, boxes)
    assert host == [one(engine, name, b)[0] for b in boxes]
    assert host[:3] == want[:3] and host[4] == want[4] and host[5] == REFUSED
    dev = torch.device("cuda", 0)
    keep, dboxes = [], []
    for b in boxes:
        d = dict(t=len(b["commitments"]) // L, n=len(b["positions"]), challenge=b["challenge"])
        # every array in an allocation of its own; the byte arrays one byte in (odd addresses), positions aligned
        for k in FIELDS:
            data = bytes(1) + b[k]
            buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            keep.append((buf, data))
            d[k + "_ptr"] = buf.data_ptr() + 1
        pos = torch.from_numpy(np.array(b["positions"], dtype=np.int64)).to(dev)
        keep.append((pos, None))
        d["positions_ptr"] = pos.data_ptr()
        dboxes.append(d)
    torch.cuda.synchronize()
    got, d = delta(engine, lambda: engine.ec_verify_many_device(gid, dboxes))
    assert got == host and d == (1, sum(h != REFUSED for h in host), 0)
    assert "public keys: element 1" in engine.last_error()
    assert delta(engine, lambda: engine.ec_verify_many_device(gid, dboxes[:1])) == (host[:1], (0, 0, 1))     # the one-box path
    null = dict(dboxes[1], shares_ptr=0)
    assert engine.ec_verify_many_device(gid, dboxes[:2] + [null] + dboxes[2:4]) == host[:2] + [REFUSED] + host[2:4]
    torch.cuda.synchronize()
    for buf, data in keep:
        if data is not None:
            assert buf.cpu().numpy().tobytes() == data, "an input buffer in HBM changed"


# ---- (6) mode 0 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_mode_0_is_the_path_of_every_box_on_its_own(engine, name):
    from mpvss_rs_amd import capi
    boxes, want = honest(engine, name, MB.TILE_SHAPES[:6], 100)
    boxes.append(dict(boxes[2], responses=flip(boxes[2]["responses"], 40)))
    want.append(one(engine, name, boxes[-1])[0])
    try:
        engine.set_ec_box_groups(0)
        got, d = delta(engine, lambda: engine.ec_verify_many(GID[name], boxes))
        assert got == want and d == (0, 0, len(boxes))
    finally:
        engine.set_ec_box_groups(1)
    got, d = delta(engine, lambda: engine.ec_verify_many(GID[name], boxes))
    assert got == want and d == (1, len(boxes), 0)
    for mode in (2, -1):
        with pytest.raises(capi.EngineError):
            engine.set_ec_box_groups(mode)


# ---- (7) pass boundaries, in a fresh child -----------------------------------------------------------------------------
def child(name, path):
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(MB.CHUNK)
    with open(path) as fh:
        boxes = [dict(positions=b["positions"], challenge=bytes.fromhex(b["challenge"]), **{k: bytes.fromhex(b[k]) for k in FIELDS})
                 for b in json.load(fh)]
    eng = Engine(0)
    eng.set_ec_box_groups(1)
    got = eng.ec_verify_many(GID[name], boxes)
    print("RESULT " + json.dumps(dict(got=[[v, dg.hex()] for v, dg in got], stats=eng.ec_verify_many_stats(),
                                      in_flight=list(eng.blocks_in_flight()))))
    eng.close()


def test_pass_boundaries_in_a_fresh_process(engine, tmp_path):
    """one child after another, each under its own timeout, stopping at the first that fails"""
    assert MB.stats(MB.CHUNK_SHAPES, MB.CHUNK) == MB.CHUNK_STATS
    for name in CURVES:
        boxes, want = [], []
        for k, s in enumerate(MB.CHUNK_SHAPES):
            if s.n == 0:
                src = deal(engine, name, 5, 3, 700)[0]
                box = dict(src, positions=[], pubkeys=b"", shares=b"", responses=b"")
                boxes.append(box)
                want.append(one(engine, name, box)[0])
            else:
                box, digest = deal(engine, name, s.n, s.t, 700 + k)
                boxes.append(box)
                want.append((True, digest))
        boxes[4] = dict(boxes[4], responses=flip(boxes[4]["responses"], 7))      # a box answered `false` inside the pass of 32
        want[4] = one(engine, name, boxes[4])[0]
        assert want[4][0] is False
        path = str(tmp_path / f"boxes_{name}.json")
        with open(path, "w") as fh:
            json.dump([dict(positions=b["positions"], challenge=b["challenge"].hex(), **{k: b[k].hex() for k in FIELDS}) for b in boxes], fh)
        env = dict(os.environ, MPVSS_MAX_CHUNK=str(MB.CHUNK))
        out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child", name, path],
                             capture_output=True, text=True, env=env)
        assert out.returncode == 0, f"curve {name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
        res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert [(bool(v), bytes.fromhex(dg)) for v, dg in res["got"]] == want
        assert res["stats"] == MB.CHUNK_STATS and res["in_flight"] == [0, 0]


# ---- (8) workspace reuse -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVES)
def test_workspace_reuse_in_both_orders(engine, name):
    big, big_digest = deal(engine, name, 513, 5, 800)
    boxes, want = honest(engine, name, MB.TILE_SHAPES[:7], 100)
    assert one(engine, name, big)[0] == (True, big_digest)
    assert engine.ec_verify_many(GID[name], boxes) == want
    assert delta(engine, lambda: engine.ec_verify_many(GID[name], [big])) == ([(True, big_digest)], (0, 0, 1))
    assert engine.ec_verify_many(GID[name], boxes[::-1]) == want[::-1]
    assert one(engine, name, big)[0] == (True, big_digest)
    # 513 shares are a small box too: between others it travels in their run (nine tiles of its own)
    got, d = delta(engine, lambda: engine.ec_verify_many(GID[name], boxes[:3] + [big] * 2 + boxes[3:]))
    assert got == want[:3] + [(True, big_digest)] * 2 + want[3:] and d == (1, 9, 0)


def test_nothing_is_left_in_flight(engine):
    assert engine.blocks_in_flight() == (0, 0)


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    child(sys.argv[2], sys.argv[3])
