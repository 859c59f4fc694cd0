"""Pins for the call frame of the run-time MODP entry points (capi_modp_rt.inc): what every entry point of a
run-time group computes when a call runs as several chunks, when its arrays live on the device, and how many kernels it
launches.

(a) One fresh child process per group width (5, 9, 18 and 27 limbs per lane) with MPVSS_MAX_CHUNK=16 -- the variable is read once
    per process -- runs a box of 45 shares, t = 3, as chunks of 16, 16 and 13 through every chunked entry point, against the oracle
    over RtOracleGroup(q) or Python's pow.  This file is its own child: `python test_gpu_modp_rt_frame.py <group>`.
(b) In-process, 33 shares: each entry point that takes a `space` is called with MPVSS_DEVICE on torch tensors and with MPVSS_HOST on
    the same bytes; outputs, verdicts and digests must be equal.
(c) The kernel launches per timer id after each call of (a), for the 2048-bit group, as literals."""
import ctypes as C
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

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_wide_helpers as WH

pytestmark = pytest.mark.gpu

N, T, CHUNK = 45, 3, 16                   # chunks of 16, 16 and 13 shares
GROUPS = {                                # name -> (q, element bytes, limbs per lane)
    "64": (lambda: H.small_safe_primes()[64], 256, 5),
    "1024": (lambda: H.rfc_prime(1024), 256, 9),
    "2048": (lambda: H.rfc_prime(2048), 256, 18),
    "group15": (WH.group15, WH.EB, 27),
}


def cat(vals, eb):
    return b"".join(v.to_bytes(eb, "big") for v in vals)


def split(b, eb):
    return [int.from_bytes(b[i:i + eb], "big") for i in range(0, len(b), eb)]


def flip(buf, row, eb, byte=None):
    b = bytearray(buf)
    b[row * eb + (eb - 1 if byte is None else byte)] ^= 1
    return bytes(b)


def make_group(name):
    from mpvss_rs_amd import ModpGroup
    q, eb, lpl = GROUPS[name][0](), GROUPS[name][1], GROUPS[name][2]
    grp = ModpGroup(q, elem_bytes=eb) if eb != 256 else ModpGroup(q)
    assert (grp.elem_bytes, grp.limbs_per_lane) == (eb, lpl)
    return q, eb, grp


def instance(q, n, t, seed):
    """a box of the oracle's own dealer over the group of q, with the randomness kept (_instance of test_gpu_modp_rt_protocol.py)"""
    g = H.RtOracleGroup(q)
    rng = random.Random(seed)
    privs, pks, seen = [], [], set()
    while len(pks) < n:
        k = H.keygen(g, rng)
        pk = g.generate_public_key(k)
        if pk not in seen:
            seen.add(pk)
            privs.append(k)
            pks.append(pk)
    coeffs = [rng.randrange(1, g.q - 1) for _ in range(t)]
    ws = [H.keygen(g, rng) for _ in range(n)]
    box = O.distribute_secret(g, 0x1234, pks, t, coeffs, ws)
    return g, privs, pks, coeffs, ws, box


# ---- (a) and (c): the child ------------------------------------------------------------------------------------------------
def child(name):
    """every chunked entry point of one group in this process (MPVSS_MAX_CHUNK=16); prints the launch counts and the paths taken"""
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(CHUNK)
    q, eb, grp = make_group(name)
    eng = Engine(0)
    counts, paths = {}, {}

    def call(label, fn):
        out = fn()
        counts[label] = [eng.kernel_launches(i) for i in range(5)]
        return out

    g, privs, pks, coeffs, ws, box = instance(q, N, T, seed=7)
    keys = [g.element_to_bytes(p) for p in pks]
    positions = list(range(1, N + 1))
    assert [box["positions"][k] for k in keys] == positions
    rng = random.Random(3)
    ct = lambda vals: cat(vals, eb)
    sp = lambda b: split(b, eb)
    Y = [box["shares"][k] for k in keys]
    R = [box["responses"][k] for k in keys]
    Cm, ch = ct(box["commitments"]), ct([box["challenge"]])

    # group_batch_exp, _fixed_base, _twin_exp, _scalar_mul against pow
    e2 = [rng.randrange(q - 1) for _ in range(N)]
    assert sp(call("batch_exp", lambda: eng.group_batch_exp(grp, ct(pks), ct(ws)))) == [pow(b, e, q) for b, e in zip(pks, ws)]
    assert sp(call("batch_exp_fixed_base", lambda: eng.group_batch_exp_fixed_base(grp, ct([3]), ct(ws)))) == [pow(3, e, q) for e in ws]
    o1, o2 = call("batch_twin_exp", lambda: eng.group_batch_twin_exp(grp, ct(pks), ct(ws), ct(e2)))
    assert sp(o1) == [pow(b, e, q) for b, e in zip(pks, ws)] and sp(o2) == [pow(b, e, q) for b, e in zip(pks, e2)]
    assert sp(call("batch_scalar_mul", lambda: eng.group_batch_scalar_mul(grp, ct(ws), ct(e2)))) == [a * b % (q - 1) for a, b in zip(ws, e2)]

    # group_commit_eval
    assert sp(call("commit_eval", lambda: eng.group_commit_eval(grp, Cm, positions))) == box["_X"]

    # group_dleq_commitments with a shared and with a per-share challenge
    h1, g2, h2 = box["_X"], pks, Y
    c1 = box["challenge"]
    a1, a2 = call("dleq_commitments_shared", lambda: eng.group_dleq_commitments(grp, ct([g.g_gen]), ct(h1), ct(g2), ct(h2), ct(R), ch, False))
    assert sp(a1) == [pow(g.g_gen, r, q) * pow(x, c1, q) % q for x, r in zip(h1, R)] == box["_a1"]
    assert sp(a2) == [pow(y, r, q) * pow(s, c1, q) % q for y, s, r in zip(g2, h2, R)] == box["_a2"]
    a1, a2 = call("dleq_commitments_per_share", lambda: eng.group_dleq_commitments(grp, ct([g.g_gen]), ct(h1), ct(g2), ct(h2), ct(R), ct(e2), True))
    assert sp(a1) == [pow(g.g_gen, r, q) * pow(x, c, q) % q for x, r, c in zip(h1, R, e2)]
    assert sp(a2) == [pow(y, r, q) * pow(s, c, q) % q for y, s, r, c in zip(g2, h2, R, e2)]

    # group_verify_distribution: honest, and one bit of a response of the third chunk flipped
    verify = lambda resp: eng.group_verify_distribution(grp, Cm, positions, ct(pks), ct(Y), resp, ch, dump=True)
    v = call("verify_distribution", lambda: verify(ct(R)))
    assert v["verdict"] is True and v["digest"] == box["_digest"]
    assert sp(v["X"]) == box["_X"] and sp(v["a1"]) == box["_a1"] and sp(v["a2"]) == box["_a2"]
    bad = verify(flip(ct(R), 40, eb))
    assert bad["verdict"] is False and bad["digest"] != box["_digest"]
    assert bad["X"] == v["X"] and bad["a1"][: 40 * eb] == v["a1"][: 40 * eb] and bad["a1"][40 * eb:41 * eb] != v["a1"][40 * eb:41 * eb]
    assert bad["a1"][41 * eb:] == v["a1"][41 * eb:]

    # group_distribute and group_deal
    P = [O.poly_get_value(coeffs, i) % (q - 1) for i in positions]
    d = call("distribute", lambda: eng.group_distribute(grp, Cm, positions, ct(pks), ct(P), ct(ws)))
    assert sp(d["X"]) == box["_X"] and sp(d["Y"]) == Y and sp(d["a1"]) == box["_a1"] and sp(d["a2"]) == box["_a2"]
    assert d["digest"] == box["_digest"]
    deal = call("deal", lambda: eng.group_deal(grp, ct(coeffs), positions, ct(pks), ct(ws)))
    assert all(deal[k] == d[k] for k in ("X", "Y", "a1", "a2", "digest"))
    assert deal["challenge"] == ch and sp(deal["responses"]) == R

    # group_extract_shares; then Y of row 20 is q (0 mod q): chunk 2 alone takes the two dependent chains
    w2 = [H.keygen(g, rng) for _ in privs]
    xinv = [O.mod_inverse(k, q - 1) for k in privs]
    sbs = [O.extract_secret_share(g, box, k, w) for k, w in zip(privs, w2)]
    S, Cs = call("extract_shares", lambda: eng.group_extract_shares(grp, ct(pks), ct(Y), ct(xinv), ct(w2)))
    assert sp(S) == [sb["share"] for sb in sbs] and sp(Cs) == [sb["challenge"] for sb in sbs]
    box0 = dict(box, shares=dict(box["shares"]))
    box0["shares"][keys[20]] = q
    Y0 = [box0["shares"][k] for k in keys]
    sbs0 = [O.extract_secret_share(g, box0, k, w) for k, w in zip(privs, w2)]
    assert sbs0[20]["share"] == 0
    S0, Cs0 = call("extract_shares_zero_row", lambda: eng.group_extract_shares(grp, ct(pks), ct(Y0), ct(xinv), ct(w2)))
    assert sp(S0) == [sb["share"] for sb in sbs0] and sp(Cs0) == [sb["challenge"] for sb in sbs0]

    # group_verify_shares with one tampered row in the second chunk
    Rs = ct([sb["response"] for sb in sbs])
    assert list(call("verify_shares", lambda: eng.group_verify_shares(grp, ct(pks), S, ct(Y), Cs, Rs))) == [1] * N
    assert list(eng.group_verify_shares(grp, ct(pks), flip(S, 20, eb), ct(Y), Cs, Rs)) == [int(i != 20) for i in range(N)]

    # the scalar ring on the host (0) and on the device (2): the same bytes
    for mode in (0, 2):
        eng.set_rt_scalar(mode)
        s0 = eng.group_scalar_stats()
        assert call(f"deal_scalar{mode}", lambda: eng.group_deal(grp, ct(coeffs), positions, ct(pks), ct(ws))) == deal
        assert call(f"extract_shares_scalar{mode}", lambda: eng.group_extract_shares(grp, ct(pks), ct(Y), ct(xinv), ct(w2))) == (S, Cs)
        assert call(f"extract_shares_zero_row_scalar{mode}",
                    lambda: eng.group_extract_shares(grp, ct(pks), ct(Y0), ct(xinv), ct(w2))) == (S0, Cs0)
        s1 = eng.group_scalar_stats()
        paths[f"scalar{mode}"] = [s1["device"] - s0["device"], s1["host"] - s0["host"]]
    eng.set_rt_scalar(1)

    # Horner's rule (0) and forward differences whenever admissible (2): the same bytes
    for mode in (0, 2):
        eng.set_rt_fd(mode, 0)
        s0 = eng.group_fd_stats()
        assert call(f"commit_eval_fd{mode}", lambda: eng.group_commit_eval(grp, Cm, positions)) == ct(box["_X"])
        s1 = eng.group_fd_stats()
        assert call(f"verify_distribution_fd{mode}", lambda: verify(ct(R))) == v
        s2 = eng.group_fd_stats()
        paths[f"fd{mode}"] = [s1["fd"] - s0["fd"], s1["horner"] - s0["horner"], s2["fd"] - s1["fd"], s2["horner"] - s1["horner"]]
    eng.set_rt_fd(1, 0)
    eng.close()
    print("COUNTS " + json.dumps(counts, sort_keys=True))
    print("PATHS " + json.dumps(paths, sort_keys=True))
    print("frame child ok")


# Kernel launches per timer id (0: X, 1: a1 / fixed base, 2: tables and combs, 3: a2 / twin / exp, 4: scalar ring) of each call of
# the child for the 2048-bit group, read from mpvss_last_kernel_launches on commit 1a2aeda ("Run-time MODP groups: the scalar
# ring Z/(q-1) on the device"), before the entry points were rewritten over RtCall.
LAUNCHES_2048 = {
    "batch_exp": [0, 0, 3, 3, 0],
    "batch_exp_fixed_base": [0, 3, 3, 0, 0],
    "batch_scalar_mul": [0, 0, 0, 0, 3],
    "batch_twin_exp": [0, 0, 3, 3, 0],
    "commit_eval": [1, 0, 0, 0, 0],
    "commit_eval_fd0": [1, 0, 0, 0, 0],
    "commit_eval_fd2": [1, 0, 0, 0, 0],
    "deal": [3, 3, 9, 3, 0],
    "deal_scalar0": [3, 3, 9, 3, 0],
    "deal_scalar2": [3, 3, 9, 3, 2],
    "distribute": [3, 3, 6, 3, 0],
    "dleq_commitments_per_share": [0, 3, 12, 3, 0],
    "dleq_commitments_shared": [0, 3, 12, 3, 0],
    "extract_shares": [0, 3, 6, 3, 0],
    "extract_shares_scalar0": [0, 3, 6, 3, 0],
    "extract_shares_scalar2": [0, 3, 6, 3, 3],
    "extract_shares_zero_row": [0, 3, 7, 4, 0],
    "extract_shares_zero_row_scalar0": [0, 3, 7, 4, 0],
    "extract_shares_zero_row_scalar2": [0, 3, 7, 4, 2],
    "verify_distribution": [3, 3, 12, 3, 0],
    "verify_distribution_fd0": [3, 3, 12, 3, 0],
    "verify_distribution_fd2": [3, 3, 12, 3, 0],
    "verify_shares": [0, 3, 12, 3, 0],
}

# What the same commit reports for these chunk sizes: [device calls, host calls] of the scalar ring over one deal and two
# extract_shares, and [fd, horner] chunks of commit_eval followed by [fd, horner] chunks of verify_distribution.
# The same at all four widths: commit_eval is one pass of 45 positions, verify_distribution three chunks.
PATHS = {"fd0": [0, 1, 0, 3], "fd2": [1, 0, 3, 0], "scalar0": [0, 3], "scalar2": [3, 0]}


def run_child(name, timeout):
    env = dict(os.environ, MPVSS_MAX_CHUNK=str(CHUNK))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, env=env, timeout=timeout)
    assert out.returncode == 0, f"group {name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
    assert "frame child ok" in out.stdout
    lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in out.stdout.splitlines() if l.startswith(("COUNTS ", "PATHS "))}
    return json.loads(lines["COUNTS"]), json.loads(lines["PATHS"])


def test_multi_chunk_calls_in_a_fresh_process_per_group():
    """(a) and (c): one child after another, stopping at the first that fails"""
    for name, timeout in (("64", 120), ("1024", 120), ("2048", 180), ("group15", 240)):
        counts, paths = run_child(name, timeout)
        print(name, "launches", json.dumps(counts, sort_keys=True))
        print(name, "paths", json.dumps(paths, sort_keys=True))
        assert paths == PATHS, name
        if name == "2048":
            assert counts == LAUNCHES_2048


# ---- (b): device space equals host space --------------------------------------------------------------------------------
NB = 33


class Dev:
    """torch tensors on the device for one call: the pointers the C ABI takes, and the outputs read back"""

    def __init__(self):
        import torch
        self.torch, self.keep = torch, []

    def inp(self, b):
        t = self.torch.frombuffer(bytearray(b), dtype=self.torch.uint8).cuda()
        self.keep.append(t)
        return C.c_void_p(t.data_ptr())

    def out(self, nbytes):
        t = self.torch.zeros(nbytes, dtype=self.torch.uint8, device="cuda")
        self.keep.append(t)
        return t

    def pos(self, positions):
        t = self.torch.tensor(positions, dtype=self.torch.int64).cuda()
        self.keep.append(t)
        return C.c_void_p(t.data_ptr())

    def sync(self):
        self.torch.cuda.synchronize()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def back(t):
    return bytes(t.cpu().numpy())


_BOXES = {}


def device_case(name):
    """group, box and share boxes of NB shares, computed once per group and left unchanged"""
    if name not in _BOXES:
        q, eb, grp = make_group(name)
        g, privs, pks, coeffs, ws, box = instance(q, NB, T, seed=11)
        keys = [g.element_to_bytes(p) for p in pks]
        _BOXES[name] = dict(q=q, eb=eb, grp=grp, g=g, privs=privs, pks=pks, coeffs=coeffs, ws=ws, box=box,
                            Y=[box["shares"][k] for k in keys], R=[box["responses"][k] for k in keys])
    return _BOXES[name]


def host_buf(b):
    arr = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
    return arr


DEVICE = 1


@pytest.mark.parametrize("name", ["64", "2048"])
def test_device_space_equals_host_space_group_ops(engine, name):
    from mpvss_rs_amd import capi
    assert capi.MPVSS_DEVICE == DEVICE
    k = device_case(name)
    q, eb, grp, lib = k["q"], k["eb"], k["grp"], engine.lib
    ct = lambda vals: cat(vals, eb)
    rng = random.Random(5)
    e2 = [rng.randrange(q - 1) for _ in range(NB)]
    B, E1, E2 = ct(k["pks"]), ct(k["ws"]), ct(e2)
    d = Dev()
    # batch_exp
    o = d.out(NB * eb)
    d.sync()
    assert lib.mpvss_modp_group_batch_exp(engine.ctx, grp.handle, DEVICE, d.inp(B), d.inp(E1), NB, ptr(o)) == 0
    want = engine.group_batch_exp(grp, B, E1)
    assert back(o) == want and split(want, eb) == [pow(b, e, q) for b, e in zip(k["pks"], k["ws"])]
    # batch_exp_fixed_base (the base is host bytes in either space)
    o = d.out(NB * eb)
    base = host_buf(ct([3]))
    d.sync()
    assert lib.mpvss_modp_group_batch_exp_fixed_base(engine.ctx, grp.handle, DEVICE, base, d.inp(E1), NB, ptr(o)) == 0
    assert back(o) == engine.group_batch_exp_fixed_base(grp, ct([3]), E1)
    # batch_twin_exp
    o1, o2 = d.out(NB * eb), d.out(NB * eb)
    d.sync()
    assert lib.mpvss_modp_group_batch_twin_exp(engine.ctx, grp.handle, DEVICE, d.inp(B), d.inp(E1), d.inp(E2), NB, ptr(o1), ptr(o2)) == 0
    assert (back(o1), back(o2)) == engine.group_batch_twin_exp(grp, B, E1, E2)
    # dleq_commitments: a shared challenge is host bytes in either space, a per-share one lives with the other arrays
    g1, h1, g2, h2, r = ct([k["g"].g_gen]), ct(k["box"]["_X"]), B, ct(k["Y"]), ct(k["R"])
    for per_share, c in ((0, ct([k["box"]["challenge"]])), (1, E2)):
        o1, o2 = d.out(NB * eb), d.out(NB * eb)
        cp = d.inp(c) if per_share else host_buf(c)
        d.sync()
        assert lib.mpvss_modp_group_dleq_commitments(engine.ctx, grp.handle, DEVICE, host_buf(g1), d.inp(h1), d.inp(g2), d.inp(h2),
                                                     d.inp(r), cp, per_share, NB, ptr(o1), ptr(o2)) == 0
        assert (back(o1), back(o2)) == engine.group_dleq_commitments(grp, g1, h1, g2, h2, r, c, bool(per_share)), per_share


@pytest.mark.parametrize("name", ["64", "2048", "group15"])
def test_device_space_equals_host_space_verify_distribution_and_distribute(engine, name):
    k = device_case(name)
    q, eb, grp, lib, box = k["q"], k["eb"], k["grp"], engine.lib, k["box"]
    ct = lambda vals: cat(vals, eb)
    positions = list(range(1, NB + 1))
    Cm, ch, pk = ct(box["commitments"]), ct([box["challenge"]]), ct(k["pks"])
    d = Dev()
    for resp, verdict in ((ct(k["R"]), True), (flip(ct(k["R"]), NB - 2, eb), False)):
        want = engine.group_verify_distribution(grp, Cm, positions, pk, ct(k["Y"]), resp, ch, dump=True)
        assert want["verdict"] is verdict and (want["digest"] == box["_digest"]) is verdict
        v = C.c_int(-1)
        dg, x, a1, a2 = host_buf(bytes(32)), host_buf(bytes(NB * eb)), host_buf(bytes(NB * eb)), host_buf(bytes(NB * eb))
        args = (d.inp(Cm), T, d.pos(positions), d.inp(pk), d.inp(ct(k["Y"])), d.inp(resp))
        d.sync()
        assert lib.mpvss_modp_group_verify_distribution(engine.ctx, grp.handle, DEVICE, *args, NB, host_buf(ch), C.byref(v), dg, x, a1,
                                                        a2) == 0
        assert {"verdict": bool(v.value), "digest": bytes(dg), "X": bytes(x), "a1": bytes(a1), "a2": bytes(a2)} == want
    P = [O.poly_get_value(k["coeffs"], i) % (q - 1) for i in positions]
    want = engine.group_distribute(grp, Cm, positions, pk, ct(P), ct(k["ws"]))
    assert want["digest"] == box["_digest"] and split(want["Y"], eb) == k["Y"]
    outs = [d.out(NB * eb) for _ in range(4)]
    dg = host_buf(bytes(32))
    args = (d.inp(Cm), T, d.pos(positions), d.inp(pk), d.inp(ct(P)), d.inp(ct(k["ws"])))
    d.sync()
    assert lib.mpvss_modp_group_distribute(engine.ctx, grp.handle, DEVICE, *args, NB, *(ptr(o) for o in outs), dg) == 0
    assert dict(zip(("X", "Y", "a1", "a2"), (back(o) for o in outs)), digest=bytes(dg)) == want


@pytest.mark.parametrize("name", ["64", "2048"])
def test_device_space_equals_host_space_share_boxes(engine, name):
    k = device_case(name)
    q, eb, grp, lib, g, box = k["q"], k["eb"], k["grp"], engine.lib, k["g"], k["box"]
    ct = lambda vals: cat(vals, eb)
    rng = random.Random(9)
    w2 = [H.keygen(g, rng) for _ in k["privs"]]
    xinv = [O.mod_inverse(x, q - 1) for x in k["privs"]]
    pk, xi, w = ct(k["pks"]), ct(xinv), ct(w2)
    d = Dev()
    # extract_shares: an honest box, and one whose Y of row 20 is 0 mod q (the two dependent chains)
    for Y in (ct(k["Y"]), ct(k["Y"][:20] + [q] + k["Y"][21:])):
        S, Cs = engine.group_extract_shares(grp, pk, Y, xi, w)
        s_out, c_out = d.out(NB * eb), host_buf(bytes(NB * eb))
        d.sync()
        assert lib.mpvss_modp_group_extract_shares(engine.ctx, grp.handle, DEVICE, d.inp(pk), d.inp(Y), d.inp(xi), d.inp(w), NB, ptr(s_out),
                                                   c_out) == 0
        assert (back(s_out), bytes(c_out)) == (S, Cs)
    S, Cs = engine.group_extract_shares(grp, pk, ct(k["Y"]), xi, w)
    sbs = [O.extract_secret_share(g, box, x, ww) for x, ww in zip(k["privs"], w2)]
    assert split(S, eb) == [sb["share"] for sb in sbs]
    # verify_shares with one tampered row
    Rs = ct([sb["response"] for sb in sbs])
    for s, want in ((S, [1] * NB), (flip(S, 17, eb), [int(i != 17) for i in range(NB)])):
        assert list(engine.group_verify_shares(grp, pk, s, ct(k["Y"]), Cs, Rs)) == want
        vd = host_buf(bytes(NB))
        args = (d.inp(pk), d.inp(s), d.inp(ct(k["Y"])), d.inp(Cs), d.inp(Rs))
        d.sync()
        assert lib.mpvss_modp_group_verify_shares(engine.ctx, grp.handle, DEVICE, *args, NB, vd) == 0
        assert list(bytes(vd)) == want
    # reconstruct from all shares and from T spread ones (positions are host memory in either space)
    for pick in (list(range(NB)), [0, NB // 2, NB - 1]):
        pos = [i + 1 for i in pick]
        sh = ct([sbs[i]["share"] for i in pick])
        want = engine.group_reconstruct(grp, pos, sh)
        gs, mask = host_buf(bytes(eb)), host_buf(bytes(32))
        parr = (C.c_int64 * len(pos))(*pos)
        dsh = d.inp(sh)
        d.sync()
        assert lib.mpvss_modp_group_reconstruct(engine.ctx, grp.handle, DEVICE, C.cast(parr, C.c_void_p), dsh, len(pos), gs, mask) == 0
        assert (bytes(gs), bytes(mask)) == want
        assert int.from_bytes(want[1], "big") == g.secret_mask(int.from_bytes(want[0], "big"))


if __name__ == "__main__":
    child(sys.argv[1])
