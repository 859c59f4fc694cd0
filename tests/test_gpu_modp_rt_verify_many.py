"""mpvss_modp_group_verify_many on the GPU (include/mpvss_hip.h, "Many boxes in one call"; DESIGN section 13, "Many boxes in
one call"): the boxes of a whole round in one call, runs of small boxes as one batch through k_rt_commit_eval_tiles, the
challenge-spreading kernel and the per-share-c launches of a1 and a2.

The boxes are the oracle's (modp_rt_many_helpers: make_instance over RtOracleGroup) and so is their validity; the digests are
the one-box call's, byte for byte, on the same engine.  Groups: 40 and 256 bits (5 limbs per lane), 1024 (9), 2048 (18), 3072
(27, wide).

(7) runs in a fresh child process with MPVSS_MAX_CHUNK=32 (read once per process).  This file is its own child:
`python test_gpu_modp_rt_verify_many.py child <group> <boxes.json>`."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_many_helpers as M

pytestmark = pytest.mark.gpu

ALL = list(M.GROUPS)
ZERO = (False, bytes(32))


def make_group(name):
    from mpvss_rs_amd import ModpGroup
    q, eb, lpl = M.GROUPS[name][0](), M.GROUPS[name][1], M.GROUPS[name][2]
    grp = ModpGroup(q, elem_bytes=eb) if eb != 256 else ModpGroup(q)
    assert (grp.elem_bytes, grp.limbs_per_lane) == (eb, lpl)
    return q, eb, grp


def one_box(engine, grp, b):
    """the one-box call on the same engine: (verdict, digest)"""
    if b.get("keyset") is not None:
        r = engine.group_verify_distribution_keyset(grp, b["commitments"], b["positions"], b["keyset"], b["key_offset"], b["shares"],
                                                    b["responses"], b["challenge"])
    else:
        r = engine.group_verify_distribution(grp, b["commitments"], b["positions"], b["pubkeys"], b["shares"], b["responses"],
                                             b["challenge"])
    return r["verdict"], r["digest"]


def empty_box(engine, grp):
    """n == 0: the empty transcript, with the challenge that verifies it"""
    return dict(commitments=b"", positions=[], pubkeys=b"", shares=b"", responses=b"",
                challenge=engine.group_deal(grp, b"", [], b"", b"")["challenge"])


def delta(engine, fn):
    s0 = engine.group_verify_many_stats()
    out = fn()
    s1 = engine.group_verify_many_stats()
    return out, tuple(s1[k] - s0[k] for k in ("groups", "grouped_boxes", "single_boxes"))


def mixed_with_empty(engine, name, grp):
    boxes = list(M.case(name)["mixed"])
    boxes.insert(3, empty_box(engine, grp))          # in the middle: it must not end the run
    return boxes


# ---- (1) mixed shapes in one call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_mixed_shapes_in_one_call(engine, name):
    q, eb, grp = make_group(name)
    assert [(len(b["positions"]), len(b["commitments"]) // eb) for b in M.case(name)["mixed"]] == M.SHAPES
    assert all(M.case(name)["mixed_valid"])                                   # the oracle decides validity
    boxes = mixed_with_empty(engine, name, grp)
    got, d = delta(engine, lambda: engine.group_verify_many(grp, boxes))
    assert d == (1, 7, 0)                                                     # one run; the empty box in neither count
    assert [v for v, _ in got] == [True] * 8
    assert got == [one_box(engine, grp, b) for b in boxes]
    assert got[3][1] == hashlib.sha256(b"").digest()
    for threads in (1, 3, 64):                                                # clamped to 1 .. 16, same bytes
        assert engine.group_verify_many(grp, boxes, hash_threads=threads) == got


# ---- (2) tampers inside a run ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_tampers_inside_a_run(engine, name):
    q, eb, grp = make_group(name)
    c = M.case(name)
    assert all(c["run_valid"]) and not any(c["tampered_valid"])               # the oracle: each clean box holds, each tampered one fails
    boxes = []
    for b, kind in zip(c["run"], M.TAMPERS):                                  # clean, tampered, clean, tampered, ...
        boxes += [b, M.tampered(b, eb, kind)]
    got, d = delta(engine, lambda: engine.group_verify_many(grp, boxes))
    assert d == (1, 10, 0)
    assert [v for v, _ in got] == [True, False] * 5                           # a box's challenge does not leak into the next tile
    assert got == [one_box(engine, grp, b) for b in boxes]                    # the tampered digests too
    # every box tampered, in the reverse order
    bad = [M.tampered(b, eb, kind) for b, kind in zip(c["run"], M.TAMPERS)][::-1]
    got = engine.group_verify_many(grp, bad)
    assert [v for v, _ in got] == [False] * 5 and got == [one_box(engine, grp, b) for b in bad]


# ---- (3) operand edges through the tile kernel -------------------------------------------------------------------------
def test_operand_edges_through_the_tile_kernel(engine):
    q, eb, grp = make_group("40")
    rng = random.Random(40)
    top = (1 << (8 * eb)) - 1
    val = lambda: rng.randrange(1 << (8 * eb))

    def box(positions, commitments, keys=(), shares=()):
        n = len(positions)
        y, Y = [val() for _ in range(n)], [val() for _ in range(n)]
        for i, v in keys:
            y[i] = v
        for i, v in shares:
            Y[i] = v
        return dict(commitments=M.cat(commitments, eb), positions=positions, pubkeys=M.cat(y, eb), shares=M.cat(Y, eb),
                    responses=M.cat([rng.randrange(q - 1) for _ in range(n)], eb), challenge=M.cat([rng.getrandbits(256)], eb))

    boxes = [
        # positions 0, q - 1, q, 2^62, scattered and repeated, across two tiles; a commitment that is 0 mod q and one >= q
        box([0, q - 1, q, 1 << 62, 7, 7, 7, 3, 1 << 40, q - 2, q + 1, 2, 2, (1 << 63) - 1, 9, 5, 0], [3 * q, q + 5, val()],
            keys=[(1, q), (16, top)], shares=[(0, q), (15, top)]),
        box([0] * 16, [val()]),                                                # every position of a wave 0, t = 1
        box([q - 1, 0, 1], [0, val(), top, q]),                                 # a zero commitment, an all-ones one, t > n
        box([1 << 62] * 5, [val(), val()], keys=[(4, q)], shares=[(4, top)]),
    ]
    got, d = delta(engine, lambda: engine.group_verify_many(grp, boxes))
    assert d == (1, 4, 0)
    assert got == [one_box(engine, grp, b) for b in boxes]                    # validity is not the point: the same bytes


# ---- (4) key sets ----------------------------------------------------------------------------------------------------------
NKEYS = 40
KEY_BOXES = ((0, 5), (7, 16), (23, 17))                                       # (key offset, n)


def keyset_boxes(engine, name):
    """40 keys and one box of t = 3 for each of KEY_BOXES, dealt and judged by the oracle"""
    q, eb, grp = make_group(name)
    rng = random.Random(int(name) + 4)
    boxes = []
    with M.libcrypto_pow(name):
        g = H.RtOracleGroup(q)
        pks = []
        while len(pks) < NKEYS:
            pk = g.generate_public_key(H.keygen(g, rng))
            if pk not in pks:
                pks.append(pk)
        for off, n in KEY_BOXES:
            mine = pks[off:off + n]
            box = O.distribute_secret(g, 0x1234, mine, 3, [rng.randrange(g.q - 1) for _ in range(3)], [H.keygen(g, rng) for _ in mine])
            boxes.append(M.flat_box(g, mine, box, eb))
            assert O.verify_distribution_shares(g, box)
    return grp, eb, pks, boxes


@pytest.mark.parametrize("name", ["256", "1024", "2048", "3072"])
def test_boxes_over_one_key_set(engine, name):
    grp, eb, pks, arrays = keyset_boxes(engine, name)
    with engine.group_keyset_create(grp, M.cat(pks, eb)) as ks:
        keyed = [dict(b, pubkeys=None, keyset=ks, key_offset=off) for b, (off, _) in zip(arrays, KEY_BOXES)]
        want = [one_box(engine, grp, b) for b in keyed]                       # group_verify_distribution_keyset, box by box
        assert [v for v, _ in want] == [True] * 3 and want == [one_box(engine, grp, b) for b in arrays]
        got, d = delta(engine, lambda: engine.group_verify_many(grp, keyed))
        assert got == want and d == (1, 3, 0)
        # key-set and key-array boxes in turn: every alternation ends a run, so every box is a run of one
        turn = [keyed[0], arrays[1], keyed[2], arrays[0], keyed[1]]
        got, d = delta(engine, lambda: engine.group_verify_many(grp, turn))
        assert got == [want[0], want[1], want[2], want[0], want[1]] and d == (0, 0, 5)
        # key_offset + n beyond the set costs that box alone
        beyond = dict(keyed[2], key_offset=NKEYS - 16)
        got, d = delta(engine, lambda: engine.group_verify_many(grp, [keyed[0], beyond, keyed[1]]))
        assert got == [want[0], ZERO, want[1]] and d == (1, 2, 0)
        # a tampered share in a key-set run, and the same keys at another offset fail
        bad = dict(keyed[1], shares=M.flip(keyed[1]["shares"], 15, eb))
        moved = dict(keyed[0], key_offset=1)
        got = engine.group_verify_many(grp, [keyed[0], bad, moved, keyed[2]])
        assert [v for v, _ in got] == [True, False, False, True] and got == [one_box(engine, grp, b) for b in (keyed[0], bad, moved, keyed[2])]
        # a set of another modulus is that box's own fault
        other = make_group("40")[2]
        with engine.group_keyset_create(other, M.cat([3, 5, 7, 11, 13], 256)) as wrong:
            if eb == 256:
                got = engine.group_verify_many(grp, [keyed[0], dict(keyed[0], keyset=wrong, key_offset=0), keyed[1]])
                assert got == [want[0], ZERO, want[1]]


# ---- (5) malformed and degenerate ------------------------------------------------------------------------------------------
def test_malformed_and_degenerate(engine):
    from mpvss_rs_amd import capi
    q, eb, grp = make_group("256")
    v = M.case("256")["run"]
    want = [one_box(engine, grp, b) for b in v[:3]]
    no_shares = dict(v[3], shares=None)
    no_t = dict(v[4], commitments=b"")                                        # t == 0 with n > 0
    no_challenge = dict(v[3], challenge=None)
    got, d = delta(engine, lambda: engine.group_verify_many(grp, [v[0], no_shares, v[1], no_t, no_challenge, v[2]]))
    assert got == [want[0], ZERO, want[1], ZERO, ZERO, want[2]] and d == (1, 3, 0)
    # n above 0x7fffffff
    arr = (capi.GroupBox * 2)()
    keep = [capi._buf(x) for x in (v[0]["commitments"], v[0]["pubkeys"], v[0]["challenge"])]
    arr[0] = capi.GroupBox(keep[0][1], 3, keep[1][1], keep[1][1], keep[1][1], keep[1][1], 1 << 31, keep[2][1], None, 0)
    arr[1] = capi.GroupBox(keep[0][1], 1 << 31, keep[1][1], keep[1][1], keep[1][1], keep[1][1], 5, keep[2][1], None, 0)
    verdicts, digests = (C.c_int * 2)(7, 7), (C.c_uint8 * 64)(*([1] * 64))
    lib, ctx = engine.lib, engine.ctx
    assert lib.mpvss_modp_group_verify_many(ctx, grp.handle, 0, arr, 2, 0, verdicts, C.cast(digests, C.c_void_p)) == 0
    assert list(verdicts) == [0, 0] and bytes(digests) == bytes(64)
    # count == 0, with and without the other pointers; no group; no verdicts; no boxes
    assert engine.group_verify_many(grp, []) == []
    assert lib.mpvss_modp_group_verify_many(ctx, grp.handle, 0, None, 0, 0, None, None) == 0
    assert lib.mpvss_modp_group_verify_many(ctx, None, 0, arr, 2, 0, verdicts, None) == -1
    assert lib.mpvss_modp_group_verify_many(ctx, grp.handle, 0, arr, 2, 0, None, None) == -1
    assert lib.mpvss_modp_group_verify_many(ctx, grp.handle, 0, None, 2, 0, verdicts, None) == -1
    assert lib.mpvss_modp_group_verify_many(None, grp.handle, 0, arr, 2, 0, verdicts, None) == -1
    assert lib.mpvss_modp_group_verify_many_stats(None, None, None, None) == -1
    assert lib.mpvss_modp_group_verify_many_stats(ctx, None, None, None) == 0
    # digests are optional, and the context still works
    verdicts = (C.c_int * 2)(7, 7)
    assert lib.mpvss_modp_group_verify_many(ctx, grp.handle, 0, arr, 2, 0, verdicts, None) == 0 and list(verdicts) == [0, 0]
    assert engine.group_verify_many(grp, v[:3]) == want
    # a negative position ends the call as it ends the one-box call
    from mpvss_rs_amd import EngineError
    neg = dict(v[1], positions=[1, 2, -3, 4, 5])
    with pytest.raises(EngineError, match="rc=-1"):
        engine.group_verify_many(grp, [v[0], neg, v[2]])
    with pytest.raises(EngineError, match="rc=-1"):
        one_box(engine, grp, neg)
    assert engine.group_verify_many(grp, v[:3]) == want


# ---- (6) device space ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_device_space_equals_host_space(engine, name):
    import torch
    q, eb, grp = make_group(name)
    boxes = mixed_with_empty(engine, name, grp)
    host = engine.group_verify_many(grp, boxes)
    keep, dev = [], []
    for b in boxes:
        n = len(b["positions"])
        d = dict(t=len(b["commitments"]) // eb, n=n, challenge=b["challenge"])
        if n:
            ts = [torch.frombuffer(bytearray(b[k]), dtype=torch.uint8).cuda() for k in ("commitments", "pubkeys", "shares", "responses")]
            ts.append(torch.tensor(b["positions"], dtype=torch.int64).cuda())
            keep.append(ts)
            d.update(commitments_ptr=ts[0].data_ptr(), pubkeys_ptr=ts[1].data_ptr(), shares_ptr=ts[2].data_ptr(),
                     responses_ptr=ts[3].data_ptr(), positions_ptr=ts[4].data_ptr())
        dev.append(d)
    torch.cuda.synchronize()
    got, d = delta(engine, lambda: engine.group_verify_many_device(grp, dev))
    assert got == host and d == (1, 7, 0)
    for ts, b in zip(keep, [b for b in boxes if b["positions"]]):             # the caller's arrays are left as they were
        assert bytes(ts[2].cpu().numpy()) == b["shares"] and ts[4].cpu().tolist() == b["positions"]


# ---- (7) several runs and the one-box path, in a fresh child ---------------------------------------------------------------
CHUNK = 32


def child_boxes(name):
    """ten boxes of (5, 3) -- at least two runs under MPVSS_MAX_CHUNK=32 -- then one of (33, 2), which fits no run and is chunked"""
    c = M.case(name)
    assert M.SHAPES[5] == (33, 2) and M.TAMPER_SHAPE == (5, 3)
    return c["run"] + c["run"][::-1] + [c["mixed"][5]]


def child(name, path):
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(CHUNK)
    with open(path) as fh:
        boxes = [{k: (v if k == "positions" else bytes.fromhex(v)) for k, v in b.items()} for b in json.load(fh)]
    eng = Engine(0)
    grp = make_group(name)[2]
    got = eng.group_verify_many(grp, boxes)
    print("RESULT " + json.dumps(dict(got=[[v, d.hex()] for v, d in got], stats=eng.group_verify_many_stats())))
    eng.close()


def test_several_runs_and_the_one_box_path_in_a_fresh_process(engine, tmp_path):
    """one child after another, each under its own timeout, stopping at the first that fails"""
    for name in ("256", "1024"):
        q, eb, grp = make_group(name)
        boxes = child_boxes(name)
        want = engine.group_verify_many(grp, boxes)                           # this process: no MPVSS_MAX_CHUNK
        assert [v for v, _ in want] == [True] * 11 and want[10] == one_box(engine, grp, boxes[10])
        path = str(tmp_path / f"boxes_{name}.json")
        with open(path, "w") as fh:
            json.dump([{k: (v if k == "positions" else v.hex()) for k, v in b.items()} for b in boxes], fh)
        env = dict(os.environ, MPVSS_MAX_CHUNK=str(CHUNK))
        out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child", name, path],
                             capture_output=True, text=True, env=env)
        assert out.returncode == 0, f"group {name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
        res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert [(v, bytes.fromhex(d)) for v, d in res["got"]] == want
        assert res["stats"]["single_boxes"] == 1 and res["stats"]["groups"] >= 2 and res["stats"]["grouped_boxes"] == 10


# ---- (8) set_rt_fd modes ---------------------------------------------------------------------------------------------------
def test_forward_difference_modes_give_the_same_bytes(engine):
    q, eb, grp = make_group("1024")
    boxes = mixed_with_empty(engine, "1024", grp)
    try:
        res = {}
        for mode in (2, 0):
            engine.set_rt_fd(mode, 0)
            res[mode], d = delta(engine, lambda: engine.group_verify_many(grp, boxes))
            assert d == (1, 7, 0)
            assert res[mode] == [one_box(engine, grp, b) for b in boxes]      # the one-box call under the same mode
        assert res[2] == res[0] and [v for v, _ in res[0]] == [True] * 8
    finally:
        engine.set_rt_fd(1, 0)


# ---- (9) two threads on one context ------------------------------------------------------------------------------------------
def test_two_threads_on_one_context(engine):
    q, eb, grp = make_group("1024")
    jobs = [mixed_with_empty(engine, "1024", grp), M.case("1024")["run"]]
    want = [engine.group_verify_many(grp, j) for j in jobs]
    assert want[1] == [one_box(engine, grp, b) for b in jobs[1]]
    got, errors = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                got[i] = engine.group_verify_many(grp, jobs[i])
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors and got == want


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    child(sys.argv[2], sys.argv[3])
