"""The per-share DLEQ hash of a run-time MODP group on the device (k_rt_share_verdict; mpvss_modp_group_dleq_challenges,
mpvss_modp_group_verify_shares and mpvss_modp_group_extract_shares under mpvss_ctx_set_rt_share_hash), against hashlib over the
oracle's framing and against the oracle's own extract_secret_share / dleq_verify -- never against the library's host path alone.

Handles: the 512-bit safe prime (5 limbs per lane), RFC 1024 (9), RFC 2048 (18), RFC 3526 group 15 on a wide handle (27, 384-byte
elements), the odd 258-bit modulus 2^257 + 1 (the narrowest admitted) and a 256-bit safe prime (not admitted: host path).

The chunk edges run in a fresh child process with MPVSS_MAX_CHUNK=16 (read once per process); this file is its own child:
`python test_gpu_modp_rt_share_hash.py <group>`."""
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

import modp_rt_helpers as H
import modp_rt_share_hash_cases as SH
import modp_rt_wide_helpers as WH
import mpvss_oracle as O

pytestmark = pytest.mark.gpu

GROUPS = {                                # name -> (q, element bytes, limbs per lane)
    "512": (lambda: H.small_safe_primes()[512], 256, 5),
    "1024": (lambda: H.rfc_prime(1024), 256, 9),
    "2048": (lambda: H.rfc_prime(2048), 256, 18),
    "group15": (WH.group15, WH.EB, 27),
    "2^257+1": (lambda: 2 ** 257 + 1, 256, 5),
    "256": (lambda: H.small_safe_primes()[256], 256, 5),
}
DEVICE = 1
_GROUPS, _CASES = {}, {}


def group(name):
    """(q, element bytes, handle), made once per name"""
    if name not in _GROUPS:
        from mpvss_rs_amd import ModpGroup
        q, eb, lpl = GROUPS[name][0](), GROUPS[name][1], GROUPS[name][2]
        grp = ModpGroup(q, elem_bytes=eb) if eb != 256 else ModpGroup(q)
        assert (grp.elem_bytes, grp.limbs_per_lane) == (eb, lpl)
        assert grp.has_device_share_hash is (name != "256")
        _GROUPS[name] = (q, eb, grp)
    return _GROUPS[name]


class modes:
    """the session's engine under a share-hash (and scalar-ring) mode, put back to automatic on the way out"""

    def __init__(self, engine, share_hash, scalar=1):
        self.engine, self.share_hash, self.scalar = engine, share_hash, scalar

    def __enter__(self):
        self.engine.set_rt_share_hash(self.share_hash)
        self.engine.set_rt_scalar(self.scalar)
        self.before = self.engine.group_share_hash_stats()
        return self

    def moved(self):
        now = self.engine.group_share_hash_stats()
        return now["device"] - self.before["device"], now["host"] - self.before["host"]

    def __exit__(self, *exc):
        self.engine.set_rt_share_hash(1)
        self.engine.set_rt_scalar(1)


class Dev:
    """torch tensors on the device for one call: the pointers the C ABI takes"""

    def __init__(self):
        import torch
        self.torch, self.keep = torch, []

    def inp(self, b):
        t = self.torch.frombuffer(bytearray(b), dtype=self.torch.uint8).cuda()
        self.keep.append(t)
        return t.data_ptr()

    def out(self, nbytes):
        t = self.torch.full((nbytes,), 0xA5, dtype=self.torch.uint8, device="cuda")
        self.keep.append(t)
        return t

    def sync(self):
        self.torch.cuda.synchronize()


def back(t):
    return bytes(t.cpu().numpy())


def host_buf(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")


# ---- 1: the challenges of the generator's rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2048", "group15"])
def test_dleq_challenges_over_the_generator_rows(engine, name):
    q, eb, grp = group(name)
    rows = SH.transcript_rows(eb, q, seed=0xA0 + eb)
    n = len(rows)
    assert n >= 320 and n % 64 != 0
    want = [SH.challenge(*row)[0] for row in rows]
    cols = [SH.cat([row[k] for row in rows], eb) for k in range(4)]
    got = SH.split(engine.group_dleq_challenges(grp, *cols), eb)
    bad = [i for i in range(n) if got[i] != want[i]]
    print(f"{name}: rows {n}, challenges equal {n - len(bad)}, timer 5 {engine.kernel_ms(5):.3f} ms")
    assert len(got) == n and bad == []
    assert engine.kernel_launches(5) == 1 and [engine.kernel_launches(i) for i in range(5)] == [0] * 5
    for m in (1, 63, 64, 65):
        assert SH.split(engine.group_dleq_challenges(grp, *(c[: m * eb] for c in cols)), eb) == want[:m], m
    assert engine.group_dleq_challenges(grp, b"", b"", b"", b"") == b""
    # device space: the kernel writes the caller's own array, elem_bytes per challenge
    d = Dev()
    out = d.out(n * eb)
    ptrs = [d.inp(c) for c in cols]
    d.sync()
    engine.group_dleq_challenges_device(grp, *ptrs, n, out.data_ptr())
    assert back(out) == SH.cat(want, eb)


def test_dleq_challenges_refuses_a_handle_without_the_device_hash(engine):
    from mpvss_rs_amd import capi
    q, eb, grp = group("256")
    one = SH.cat([1], eb)
    with pytest.raises(capi.EngineError, match="device share hash"):
        engine.group_dleq_challenges(grp, one, one, one, one)
    assert engine.group_dleq_challenges(grp, b"", b"", b"", b"") == b""          # n == 0 is MPVSS_OK for every handle


# ---- 2: verify_shares on rows that must verify -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["512", "1024", "2048", "group15", "2^257+1"])
def test_verify_shares_device_hash_on_must_verify_rows(engine, name):
    q, eb, grp = group(name)
    g = H.RtOracleGroup(q)
    rows = SH.must_verify_rows(g, seed=0xB0)
    n = len(rows)
    assert n % 64 != 0 and all(0 < row[3] < (q - 1) // 2 for row in rows)
    pk, s, y, c, r = (SH.cat([row[k] for row in rows], eb) for k in range(5))
    cs = [row[3] for row in rows]
    variants = {
        "honest": (cs, 1),
        "a bit of c flipped": ([ci ^ (1 << (i % 255)) for i, ci in enumerate(cs)], 0),
        "c + 2^256": ([ci + 2 ** 256 for ci in cs], 0),                 # the leading elem_bytes - 32 bytes are checked
        "c + (q-1)/2": ([ci + (q - 1) // 2 for ci in cs], 0),           # an unreduced challenge does not match on the host either
    }
    for mode in (2, 0):
        with modes(engine, mode) as m:
            for what, (cc, want) in variants.items():
                got = engine.group_verify_shares(grp, pk, s, y, SH.cat(cc, eb), r)
                wrong = [i for i in range(n) if got[i] != want]
                print(f"{name} mode {mode} {what}: rows {n}, as expected {n - len(wrong)}")
                assert len(got) == n and wrong == [], (mode, what)
                assert engine.kernel_launches(5) == (1 if mode == 2 else 0)
            assert m.moved() == ((len(variants), 0) if mode == 2 else (0, len(variants)))


# ---- 3: honest proofs of the oracle's extract_secret_share --------------------------------------------------------------
NB = 33


def share_case(name, n=NB, seed=21):
    """n honest share boxes of the oracle over the group `name` (computed once, left unchanged), and the same with Y of row 20
    replaced by q (0 mod q: S = 0, the two dependent chains)"""
    if (name, n) not in _CASES:
        q, eb, grp = group(name)
        g = H.RtOracleGroup(q)
        rng = random.Random(seed)
        # Python's pow is the cost of this fixture (0.1 s at 3072 bits), and the oracle's S_i = Y_i^(1/x_i) is one per row whatever
        # the key: rows after the first take 64-bit keys, 128-bit witnesses and Y_i = (4^s)^x_i, so that it is the only one.  1/x_i,
        # the responses and e2 = w / x stay as long as q - 1 in every row.
        import math
        privs, pks = [H.keygen(g, rng)], []
        while len(privs) < n:
            x = rng.getrandbits(64) | 1
            if math.gcd(x, q - 1) == 1 and x not in privs:
                privs.append(x)
        pks = [g.generate_public_key(x) for x in privs]
        assert len(set(pks)) == n
        Y = [pow(pks[0], rng.randrange(1, q - 1), q)] + [pow(pow(4, rng.getrandbits(64), q), x, q) for x in privs[1:]]
        w = [H.keygen(g, rng)] + [rng.getrandbits(128) | 1 for _ in privs[1:]]
        box = {"shares": {g.element_to_bytes(p): yy for p, yy in zip(pks, Y)}}
        sbs = [O.extract_secret_share(g, box, k, ww) for k, ww in zip(privs, w)]
        Y0 = Y[:20] + [q] + Y[21:]
        box0 = {"shares": {g.element_to_bytes(pks[20]): q}}
        sbs0 = sbs[:20] + [O.extract_secret_share(g, box0, privs[20], w[20])] + sbs[21:]
        assert sbs0[20]["share"] == 0
        sb = sbs[5]
        assert O.dleq_verify(g, g.generator(), pks[5], sb["share"], Y[5], sb["challenge"], sb["response"]) is True
        _CASES[name, n] = dict(g=g, privs=privs, pks=pks, Y=Y, Y0=Y0, w=w, xinv=[O.mod_inverse(k, q - 1) for k in privs], sbs=sbs,
                               sbs0=sbs0)
    return _CASES[name, n]


def flip(buf, row, eb):
    b = bytearray(buf)
    b[row * eb + eb - 1] ^= 1
    return bytes(b)


@pytest.mark.parametrize("name", ["512", "1024", "2048", "group15"])
def test_honest_proofs_extract_and_verify_under_both_hash_paths(engine, name):
    q, eb, grp = group(name)
    k = share_case(name)
    ct = lambda vals: SH.cat(vals, eb)
    pk, xi, w = ct(k["pks"]), ct(k["xinv"]), ct(k["w"])
    lib = engine.lib
    for Yv, sbs in ((k["Y"], k["sbs"]), (k["Y0"], k["sbs0"])):
        Y = ct(Yv)
        want = (ct([sb["share"] for sb in sbs]), ct([sb["challenge"] for sb in sbs]))
        for scalar in (0, 2):
            for mode in (2, 0):
                with modes(engine, mode, scalar) as m:
                    assert engine.group_extract_shares(grp, pk, Y, xi, w) == want, (scalar, mode)
                    assert engine.kernel_launches(5) == (1 if mode == 2 else 0)
                    assert m.moved() == ((1, 0) if mode == 2 else (0, 1))
        # device space under the device hash: S into the caller's tensor, the challenges to the host
        with modes(engine, 2):
            d = Dev()
            s_out, c_out = d.out(NB * eb), host_buf(bytes(NB * eb))
            args = [C.c_void_p(d.inp(b)) for b in (pk, Y, xi, w)]
            d.sync()
            assert lib.mpvss_modp_group_extract_shares(engine.ctx, grp.handle, DEVICE, *args, NB, C.c_void_p(s_out.data_ptr()), c_out) == 0
            assert (back(s_out), bytes(c_out)) == want
    S, Cs = ct([sb["share"] for sb in k["sbs"]]), ct([sb["challenge"] for sb in k["sbs"]])
    Rs, Y = ct([sb["response"] for sb in k["sbs"]]), ct(k["Y"])
    cases = ((pk, S, [1] * NB), (pk, flip(S, 17, eb), [int(i != 17) for i in range(NB)]),
             (flip(pk, 30, eb), S, [int(i != 30) for i in range(NB)]))
    for mode in (2, 0):
        with modes(engine, mode):
            for p, s, want in cases:
                assert list(engine.group_verify_shares(grp, p, s, Y, Cs, Rs)) == want, mode
    with modes(engine, 2):
        for p, s, want in cases:
            d = Dev()
            vd = host_buf(bytes([7] * NB))
            args = [C.c_void_p(d.inp(b)) for b in (p, s, Y, Cs, Rs)]
            d.sync()
            assert lib.mpvss_modp_group_verify_shares(engine.ctx, grp.handle, DEVICE, *args, NB, vd) == 0
            assert list(bytes(vd)) == want


# ---- 4: a handle that is not admitted keeps the host path --------------------------------------------------------------------
def test_a_256_bit_modulus_keeps_the_host_path_under_mode_2(engine):
    q, eb, grp = group("256")
    g = H.RtOracleGroup(q)
    rows = SH.must_verify_rows(g, seed=0xB1)
    # the reduction mod (q-1)/2 bites for some rows: c is the unreduced hash, so those must NOT verify, on either setting
    want = [int(O.dleq_verify(g, g.generator(), row[0], row[1], row[2], row[3], row[4])) for row in rows]
    assert 0 in want and 1 in want
    pk, s, y, c, r = (SH.cat([row[k] for row in rows], eb) for k in range(5))
    for mode in (2, 0):
        with modes(engine, mode) as m:
            assert list(engine.group_verify_shares(grp, pk, s, y, c, r)) == want, mode
            assert m.moved() == (0, 1) and engine.kernel_launches(5) == 0


# ---- 5: chunk edges, in a fresh process ------------------------------------------------------------------------------------
N, CHUNK = 45, 16                          # chunks of 16, 16 and 13 shares


def child(name):
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(CHUNK)
    q, eb, grp = group(name)
    k = share_case(name, n=N, seed=23)
    ct = lambda vals: SH.cat(vals, eb)
    eng = Engine(0)
    eng.set_rt_share_hash(2)
    counts = {}
    pk, Y, xi, w = ct(k["pks"]), ct(k["Y"]), ct(k["xinv"]), ct(k["w"])
    S, Cs = eng.group_extract_shares(grp, pk, Y, xi, w)
    counts["extract_shares"] = [eng.kernel_launches(i) for i in range(6)]
    assert SH.split(S, eb) == [sb["share"] for sb in k["sbs"]] and SH.split(Cs, eb) == [sb["challenge"] for sb in k["sbs"]]
    S0, Cs0 = eng.group_extract_shares(grp, pk, ct(k["Y0"]), xi, w)
    assert SH.split(S0, eb) == [sb["share"] for sb in k["sbs0"]] and SH.split(Cs0, eb) == [sb["challenge"] for sb in k["sbs0"]]
    Rs = ct([sb["response"] for sb in k["sbs"]])
    assert list(eng.group_verify_shares(grp, pk, S, Y, Cs, Rs)) == [1] * N
    counts["verify_shares"] = [eng.kernel_launches(i) for i in range(6)]
    assert list(eng.group_verify_shares(grp, pk, flip(S, 20, eb), Y, Cs, Rs)) == [int(i != 20) for i in range(N)]
    assert list(eng.group_verify_shares(grp, pk, S, Y, flip(Cs, 31, eb), Rs)) == [int(i != 31) for i in range(N)]
    assert eng.group_share_hash_stats() == {"device": 5, "host": 0}
    eng.close()
    print("COUNTS " + json.dumps(counts, sort_keys=True))
    print("share hash child ok")


@pytest.mark.parametrize("name", ["2048", "group15"])
def test_chunk_edges_in_a_fresh_process(name):
    import test_gpu_modp_rt_frame as F
    env = dict(os.environ, MPVSS_MAX_CHUNK=str(CHUNK))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, f"group {name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
    assert "share hash child ok" in out.stdout
    counts = json.loads([l for l in out.stdout.splitlines() if l.startswith("COUNTS ")][0].split(" ", 1)[1])
    print(name, "launches", json.dumps(counts, sort_keys=True))
    for call in ("extract_shares", "verify_shares"):
        assert counts[call][5] == 3, call                          # one hash launch per chunk
        assert counts[call][:5] == F.LAUNCHES_2048[call], call     # ids 0..4 as the frame's pins list them


if __name__ == "__main__":
    child(sys.argv[1])
