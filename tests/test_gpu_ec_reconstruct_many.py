"""mpvss_ec_reconstruct_many: the secrets of a whole round in one call, against the one-secret call on the same engine, byte for
byte (G^s in the group's encoding, the 32-byte mask, the status), and against the closed form of tests/reconstruct_cases.py
(Builder.expected, Builder.mask) as well.  The cases are in tests/ec_reconstruct_many_cases.py, held to the oracle's
ref_reconstruct by tests/test_ec_reconstruct_many_cases.py.  Both curves.

(1) every boundary of k_*_sum_segments (one wave per secret) in one call, ascending and descending; (2) 1, 2, 9, 65 and 513
secrets and what the stats say; (3) coefficients shared by equal position lists only; (4) refused secrets between good ones;
(5) signs, degenerate shares and the identity on chosen lanes of m = 257; (6) shares in HBM, each secret in a buffer of its own
at an odd address (k_ec_gather_segments); (7) pass boundaries in a fresh child process with MPVSS_MAX_CHUNK=32 (read once per
process) -- this file is its own child: `python test_gpu_ec_reconstruct_many.py child <curve> <secrets.json>`; (8) after a
one-secret call of m = 513 over the same workspace.

Measured on an MI355X: 25 tests in 6.3 s.  Seconds: secret_counts[513] 1.24 / 1.02 (secp256k1 / ristretto255: 513 one-secret
calls beside the one call), pass_boundaries (two children) 1.19, refused_secrets 0.07 / 0.38, secret_counts[65] 0.36 / 0.20,
signs_and_degenerate 0.20 / 0.09; every other test below 0.2."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import ec_reconstruct_many_cases as MC
import reconstruct_cases as K

pytestmark = pytest.mark.gpu
GID = {"secp256k1": 1, "ristretto255": 2}
_KITS = {}
STATS = ("passes", "grouped_secrets", "single_secrets")


def kit(engine, name):
    """(builder whose shares come from the engine's fixed-base call, memo of the reference's factors) of a curve"""
    if name not in _KITS:
        G = K.O.GROUPS[name]()

        def power(exps):
            out = engine.ec_batch_exp_generator(GID[name], b"".join(G.scalar_to_fixed(e) for e in exps))
            return [out[k:k + G.elem_len] for k in range(0, len(out), G.elem_len)]

        _KITS[name] = (K.Builder(name, power), {})
    return _KITS[name]


def refusal(name):
    return (-1, bytes(33 if name == "secp256k1" else 32), bytes(32))


def one(engine, name, case):
    """the one-secret call on the same engine as the many-secret call reports it: (0, G^s, mask), or a refusal"""
    from mpvss_rs_amd import capi
    try:
        gs, mask = engine.ec_reconstruct(GID[name], case.positions, None if case.shares is None else b"".join(case.shares))
    except capi.EngineError as e:
        assert "rc=-1" in str(e), case.id
        return refusal(name)
    return (0, gs, mask)


def many(engine, name, cases, **kw):
    return engine.ec_reconstruct_many(GID[name], [MC.as_secret(c) for c in cases], **kw)


def delta(engine, fn):
    s0 = engine.ec_reconstruct_many_stats()
    out = fn()
    s1 = engine.ec_reconstruct_many_stats()
    return out, tuple(s1[k] - s0[k] for k in STATS)


def wanted(engine, name, cases, memo=None):
    """the one-secret call's answers, every one the builder's closed form (or its reference) with the mask of that"""
    b = kit(engine, name)[0]
    want = [one(engine, name, c) for c in cases]
    for w, c in zip(want, cases):
        assert w[0] == 0 and w[1] == b.expected(c, memo) and w[2] == b.mask(w[1]), (name, c.id)
    return want


# ---- (1) segment shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CURVES)
def test_segment_shapes_in_one_call(engine, name):
    b, _ = kit(engine, name)
    cases = MC.segment_cases(b)
    assert len(cases) == 13
    want = wanted(engine, name, cases)
    got, d = delta(engine, lambda: many(engine, name, cases))
    assert got == want, [c.id for c, g, w in zip(cases, got, want) if g != w]
    assert d == (1, 13, 0)
    assert many(engine, name, cases[::-1]) == want[::-1]
    assert many(engine, name, cases, want_masks=False) == [(s, gs, None) for s, gs, _ in want]


# ---- (2) secret counts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CURVES)
@pytest.mark.parametrize("count", MC.SECRET_COUNTS)
def test_secret_counts_and_stats(engine, name, count):
    b, _ = kit(engine, name)
    cases = MC.small_cases(b, count)
    # the one-secret call for every secret; G^P(0) of all of them by one fixed-base call, and of the first 65 -- every position
    # list many times over -- by the oracle, with the oracle's mask
    want = [one(engine, name, c) for c in cases]
    assert [w[0] for w in want] == [0] * count
    assert [w[1] for w in want] == b.power([c.expect[1] for c in cases])
    for w, c in zip(want[:65], cases[:65]):
        assert w[1] == b.expected(c) and w[2] == b.mask(w[1]), (name, c.id)
    got, d = delta(engine, lambda: many(engine, name, cases))
    assert got == want, [c.id for c, g, w in zip(cases, got, want) if g != w]
    assert d == ((0, 0, 1) if count == 1 else (1, count, 0))
    assert delta(engine, lambda: many(engine, name, []))[1] == (0, 0, 0)
    for threads in (1, 3, 64):
        assert many(engine, name, cases, host_threads=threads) == want


# ---- (3) coefficient sharing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CURVES)
def test_coefficients_are_shared_by_equal_lists_only(engine, name):
    b, _ = kit(engine, name)
    cases = MC.sharing_cases(b)
    want = wanted(engine, name, cases)
    assert want[8] == want[0]                                               # the permuted list: another list, the same secret
    assert many(engine, name, cases) == want
    assert many(engine, name, cases[::-1]) == want[::-1]


# ---- (4) refused secrets between good ones -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CURVES)
def test_refused_secrets_cost_only_themselves(engine, name):
    b, _ = kit(engine, name)
    pairs = MC.refused_between_good(b)
    cases = [c for c, _ in pairs]
    want = [one(engine, name, c) for c in cases]
    assert [w == refusal(name) for w in want] == [r for _, r in pairs]
    assert all(w[0] == 0 and w[1] == b.expected(c) and w[2] == b.mask(w[1]) for w, (c, r) in zip(want, pairs) if not r)
    got, d = delta(engine, lambda: many(engine, name, cases))
    assert got == want
    assert d == (1, sum(not r for _, r in pairs), 0)                        # refused secrets count nowhere
    # a null position list, and refusals alone
    got = engine.ec_reconstruct_many(GID[name], [MC.as_secret(cases[0]), dict(positions=None, shares=b"".join(cases[0].shares)),
                                                 MC.as_secret(cases[2])])
    assert got == [want[0], refusal(name), want[2]]
    bad = [c for c, r in pairs if r]
    assert delta(engine, lambda: many(engine, name, bad)) == ([refusal(name)] * len(bad), (0, 0, 0))
    # the rejected encoding alone with one good secret: its pass has one good secret left, which is counted
    enc = [c for c in bad if c.id == "R-encoding"]
    got, d = delta(engine, lambda: many(engine, name, enc + cases[:1]))
    assert got == [refusal(name), want[0]] and d == (1, 1, 0)
    assert delta(engine, lambda: many(engine, name, enc + enc)) == ([refusal(name)] * 2, (0, 0, 0))
    assert many(engine, name, cases[:1]) == want[:1]


# ---- (5) signs, degenerate shares, the identity on chosen lanes --------------------------------------------------------
@pytest.mark.parametrize("name", K.CURVES)
def test_signs_and_degenerate_shares(engine, name):
    b, memo = kit(engine, name)
    cases = MC.sign_and_degenerate_cases(b)
    want = wanted(engine, name, cases, memo)
    got, d = delta(engine, lambda: many(engine, name, cases))
    assert got == want, [c.id for c, g, w in zip(cases, got, want) if g != w]
    assert d == (1, len(cases), 0)


@pytest.mark.parametrize("name", K.CURVES)
def test_identity_on_the_lanes_of_257(engine, name):
    b, _ = kit(engine, name)
    cases = MC.lane_cases(b)
    want = [one(engine, name, c) for c in cases]
    for w, lane in zip(want, K.LANES_257):
        assert w[0] == 0 and w[1] == MC.identity_lane_expected(b, 257, lane) and w[2] == b.mask(w[1]), (name, lane)
    assert len({w[1] for w in want}) == len(cases)
    got, d = delta(engine, lambda: many(engine, name, cases))
    assert got == want and d == (1, len(cases), 0)


# ---- (6) device space --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CURVES)
def test_shares_in_hbm(engine, name):
    import torch
    b, _ = kit(engine, name)
    cases = MC.segment_cases(b) + [c for c, _ in MC.refused_between_good(b) if c.shares is not None and len(c.positions) > 0]
    host = many(engine, name, cases)
    assert host == [one(engine, name, c) for c in cases]
    assert sum(h == refusal(name) for h in host) == 3                       # position 0, duplicate, the rejected encoding
    # every secret in an allocation of its own, one byte in: 33-byte elements at odd addresses
    off = 1 if name == "secp256k1" else 0
    datas = [bytes(off) + b"".join(c.shares) for c in cases]
    bufs = [torch.frombuffer(bytearray(d), dtype=torch.uint8).to(torch.device("cuda", 0)) for d in datas]
    torch.cuda.synchronize()
    secrets = [dict(positions=list(c.positions), shares_ptr=buf.data_ptr() + off, m=len(c.positions)) for c, buf in zip(cases, bufs)]
    got, d = delta(engine, lambda: engine.ec_reconstruct_many_device(GID[name], secrets))
    torch.cuda.synchronize()
    assert got == host and d == (1, len(cases) - 3, 0)
    assert engine.ec_reconstruct_many_device(GID[name], secrets[:1]) == host[:1]                     # the one-secret path
    null = dict(positions=list(cases[2].positions), shares_ptr=0, m=3)
    assert engine.ec_reconstruct_many_device(GID[name], secrets[:2] + [null] + secrets[2:4]) == host[:2] + [refusal(name)] + host[2:4]
    assert engine.ec_reconstruct_many_device(GID[name], secrets, want_masks=False) == [(s, gs, None) for s, gs, _ in host]
    torch.cuda.synchronize()
    for buf, data in zip(bufs, datas):
        assert buf.cpu().numpy().tobytes() == data, "a share buffer in HBM changed"


# ---- (7) pass boundaries, in a fresh child -----------------------------------------------------------------------------
def child(name, path):
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(MC.CHUNK)
    with open(path) as fh:
        secrets = [dict(positions=s["positions"], shares=bytes.fromhex(s["shares"])) for s in json.load(fh)]
    eng = Engine(0)
    got = eng.ec_reconstruct_many(GID[name], secrets)
    print("RESULT " + json.dumps(dict(got=[[s, gs.hex(), mask.hex()] for s, gs, mask in got], stats=eng.ec_reconstruct_many_stats())))
    eng.close()


def test_pass_boundaries_in_a_fresh_process(engine, tmp_path):
    """one child after another, each under its own timeout, stopping at the first that fails"""
    for name in K.CURVES:
        b, _ = kit(engine, name)
        cases = MC.chunk_cases(b)
        want = wanted(engine, name, cases)
        path = str(tmp_path / f"secrets_{name}.json")
        with open(path, "w") as fh:
            json.dump([dict(positions=list(c.positions), shares=b"".join(c.shares).hex()) for c in cases], fh)
        env = dict(os.environ, MPVSS_MAX_CHUNK=str(MC.CHUNK))
        out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child", name, path],
                             capture_output=True, text=True, env=env)
        assert out.returncode == 0, f"curve {name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
        res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert [(s, bytes.fromhex(gs), bytes.fromhex(mask)) for s, gs, mask in res["got"]] == want
        assert res["stats"] == MC.CHUNK_STATS


# ---- (8) after a larger one-secret call on the same workspace ----------------------------------------------------------
@pytest.mark.parametrize("name", K.CURVES)
def test_after_a_larger_call_on_the_same_workspace(engine, name):
    b, _ = kit(engine, name)
    big = b.shape_case(513)
    cases = MC.small_cases(b, 5) + MC.segment_cases(b)[:6]
    want = wanted(engine, name, cases)
    assert one(engine, name, big)[1] == b.expected(big)                     # w.p1 holds 513 stale points afterwards
    assert many(engine, name, cases) == want
    assert one(engine, name, cases[3]) == want[3]                           # a plain one-secret call still gives its bytes
    assert many(engine, name, cases[::-1]) == want[::-1]


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    child(sys.argv[2], sys.argv[3])
