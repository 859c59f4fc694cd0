"""mpvss_modp_group_reconstruct_many: the secrets of a whole round in one call, against the one-secret call on the same engine,
byte for byte (G^s at the handle's element width, the 32-byte mask, the status), and at 40 and 1024 bits against the oracle's
ref_reconstruct as well.  The cases are in tests/modp_rt_reconstruct_many_cases.py, held to the oracle at 40 bits by
tests/test_modp_rt_reconstruct_many_host.py.  Groups: 40 bits (5 limbs per lane), 1024 (9), 2048 (18), 3072 (27, wide).

(1) every boundary of k_rt_product_segments' fold over 16 quads in one call, ascending and descending; (2) 1, 2, 17 and 64
workgroups and what the stats say; (3) coefficients shared by equal position lists only; (4) refused secrets between good ones;
(5) shares in HBM; (6) pass boundaries in a fresh child process with MPVSS_MAX_CHUNK=32 (read once per process) -- this file is
its own child: `python test_gpu_modp_rt_reconstruct_many.py child <group> <secrets.json>`; (7) after other calls over the same
workspace.

Measured on an MI355X: 19 tests in 6.5 s.  Seconds: segment_shapes 0.12 / 0.17 / 0.56 / 1.60 (40, 1024, 2048, 3072 bits);
pass_boundaries (two children) 1.12; workgroup_counts[rfc2048-17] 0.79; shares_in_hbm 0.76 / 0.22 at 3072 / 2048 bits;
after_other_calls 0.33; every other test below 0.1."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import modp_rt_reconstruct_cases as K
import modp_rt_reconstruct_many_cases as MC

pytestmark = pytest.mark.gpu
_KITS = {}
STATS = ("passes", "grouped_secrets", "single_secrets")


def make_group(key):
    from mpvss_rs_amd import ModpGroup
    q, eb = K.modulus(key), K.GROUPS[key][1]
    grp = ModpGroup(q, elem_bytes=eb)
    assert grp.limbs_per_lane == K.GROUPS[key][2] and grp.elem_bytes == eb, key
    return grp


def kit(engine, key):
    """(handle, builder whose shares come from the handle's fixed-base call, memo of the reference's factors) of a group"""
    if key not in _KITS:
        grp, eb = make_group(key), K.GROUPS[key][1]

        def power(base, exps):
            out = engine.group_batch_exp_fixed_base(grp, base.to_bytes(eb, "big"), b"".join(e.to_bytes(eb, "big") for e in exps))
            return [out[k:k + eb] for k in range(0, len(out), eb)]

        _KITS[key] = (grp, K.RtBuilder(key, power), {})
    return _KITS[key]


def refusal(eb):
    return (-1, bytes(eb), bytes(32))


def one(engine, grp, case):
    """the one-secret call on the same engine as the many-secret call reports it: (0, G^s, mask), or a refusal"""
    from mpvss_rs_amd import capi
    try:
        gs, mask = engine.group_reconstruct(grp, case.positions, None if case.shares is None else b"".join(case.shares))
    except capi.EngineError as e:
        assert "rc=-1" in str(e), case.id
        return refusal(grp.elem_bytes)
    return (0, gs, mask)


def many(engine, grp, cases, **kw):
    return engine.group_reconstruct_many(grp, [MC.as_secret(c) for c in cases], **kw)


def delta(engine, fn):
    s0 = engine.group_reconstruct_many_stats()
    out = fn()
    s1 = engine.group_reconstruct_many_stats()
    return out, tuple(s1[k] - s0[k] for k in STATS)


# ---- (1) segment shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.WIDTHS)
def test_segment_shapes_in_one_call(engine, key):
    grp, b, memo = kit(engine, key)
    cases = MC.segment_cases(b)
    want = [one(engine, grp, c) for c in cases]
    assert [w[0] for w in want] == [0] * len(cases)
    for w, c in zip(want, cases):
        assert w[1] == b.expected(c) and w[2] == b.mask(w[1]), (key, c.id)
        if key in ("b40", "rfc1024"):
            assert w[1] == b.reference(c, memo), (key, c.id)
    got, d = delta(engine, lambda: many(engine, grp, cases))
    assert got == want, [c.id for c, g, w in zip(cases, got, want) if g != w]
    assert d == (1, len(cases), 0)
    assert many(engine, grp, cases[::-1]) == want[::-1]
    assert many(engine, grp, cases, want_masks=False) == [(s, gs, None) for s, gs, _ in want]


# ---- (2) workgroup counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,count", [("b40", n) for n in MC.WORKGROUP_COUNTS] + [("rfc2048", 17)])
def test_workgroup_counts_and_stats(engine, key, count):
    grp, b, _ = kit(engine, key)
    cases = MC.small_cases(b, count)
    want = [one(engine, grp, c) for c in cases]
    assert all(w[0] == 0 and w[1] == b.expected(c) for w, c in zip(want, cases))
    got, d = delta(engine, lambda: many(engine, grp, cases))
    assert got == want
    assert d == ((0, 0, 1) if count == 1 else (1, count, 0))
    assert delta(engine, lambda: many(engine, grp, []))[1] == (0, 0, 0)
    for threads in (1, 3, 64):
        assert many(engine, grp, cases, host_threads=threads) == want


# ---- (3) coefficient sharing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["b40", "rfc1024"])
def test_coefficients_are_shared_by_equal_lists_only(engine, key):
    grp, b, _ = kit(engine, key)
    cases = MC.sharing_cases(b)
    want = [one(engine, grp, c) for c in cases]
    assert all(w[0] == 0 and w[1] == b.expected(c) for w, c in zip(want, cases))
    assert want[8] == want[0]                                               # the permuted list: another list, the same secret
    assert many(engine, grp, cases) == want
    assert many(engine, grp, cases[::-1]) == want[::-1]


# ---- (4) refused secrets between good ones -----------------------------------------------------------------------------
def test_refused_secrets_cost_only_themselves(engine):
    grp, b, _ = kit(engine, "b40")
    pairs = MC.refused_between_good(b)
    cases = [c for c, _ in pairs]
    want = [one(engine, grp, c) for c in cases]
    assert [w == refusal(256) for w in want] == [r for _, r in pairs]
    assert all(w[1] == b.expected(c) for w, (c, r) in zip(want, pairs) if not r)
    got, d = delta(engine, lambda: many(engine, grp, cases))
    assert got == want
    assert d == (1, sum(not r for _, r in pairs), 0)                        # refused secrets count nowhere
    # a null position list, and refusals alone
    got = engine.group_reconstruct_many(grp, [MC.as_secret(cases[0]), dict(positions=None, shares=b"".join(cases[0].shares)),
                                              MC.as_secret(cases[2])])
    assert got == [want[0], refusal(256), want[2]]
    bad = [c for c, r in pairs if r]
    assert delta(engine, lambda: many(engine, grp, bad)) == ([refusal(256)] * len(bad), (0, 0, 0))
    assert many(engine, grp, cases[:1]) == want[:1]


def test_a_denominator_without_inverse_at_q23(engine):
    grp, b, memo = kit(engine, "q23")
    pairs = MC.tiny_refused_between_good(b, lambda c: b.reference(c, memo))
    cases = [c for c, _ in pairs]
    want = [one(engine, grp, c) for c in cases]
    assert [w == refusal(256) for w in want] == [r for _, r in pairs]
    assert all(w[1] == b.reference(c, memo) for w, (c, r) in zip(want, pairs) if not r)
    assert many(engine, grp, cases) == want


def test_even_subgroup_order_refuses_every_secret(engine):
    from mpvss_rs_amd import ModpGroup
    grp = ModpGroup(K.Q_1_MOD_4)
    fix = lambda v: v.to_bytes(256, "big")
    secrets = [dict(positions=[1, 2], shares=fix(3) + fix(5)), dict(positions=[3, 1, 2], shares=fix(3) + fix(5) + fix(7)),
               dict(positions=[2, 5], shares=fix(9) + fix(4))]
    got, d = delta(engine, lambda: engine.group_reconstruct_many(grp, secrets))
    assert got == [refusal(256)] * 3 and d == (0, 0, 0)
    g40, b, _ = kit(engine, "b40")
    cases = MC.small_cases(b, 2)
    assert many(engine, g40, cases) == [one(engine, g40, c) for c in cases]


# ---- (5) device space --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.DEVICE_KEYS)
def test_shares_in_hbm(engine, key):
    import torch
    grp, b, _ = kit(engine, key)
    eb = grp.elem_bytes
    cases = [c for c in MC.segment_cases(b) if len(c.positions) in (1, 3, 16, 17, 33)] + MC.small_cases(b, 3)
    zero_neg = [c for c in b.sign_cases(5) if c.id.endswith("zero-neg")][0]
    cases.insert(2, zero_neg)                                               # shown by the pass's one copy back
    host = many(engine, grp, cases)
    assert host == [one(engine, grp, c) for c in cases] and host[2] == refusal(eb)
    data = b"".join(b"".join(c.shares) for c in cases)
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    secrets, at = [], 0
    for c in cases:
        secrets.append(dict(positions=list(c.positions), shares_ptr=buf.data_ptr() + at, m=len(c.positions)))
        at += len(c.positions) * eb
    got, d = delta(engine, lambda: engine.group_reconstruct_many_device(grp, secrets))
    torch.cuda.synchronize()
    assert got == host and d == (1, len(cases) - 1, 0)
    assert engine.group_reconstruct_many_device(grp, secrets[:1]) == host[:1]                      # the one-secret path
    assert engine.group_reconstruct_many_device(grp, secrets, want_masks=False) == [(s, gs, None) for s, gs, _ in host]
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == data, "the share buffers in HBM changed"


# ---- (6) pass boundaries, in a fresh child -----------------------------------------------------------------------------
def child(key, path):
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(MC.CHUNK)
    with open(path) as fh:
        secrets = [dict(positions=s["positions"], shares=bytes.fromhex(s["shares"])) for s in json.load(fh)]
    eng = Engine(0)
    got = eng.group_reconstruct_many(make_group(key), secrets)
    print("RESULT " + json.dumps(dict(got=[[s, gs.hex(), mask.hex()] for s, gs, mask in got], stats=eng.group_reconstruct_many_stats())))
    eng.close()


def test_pass_boundaries_in_a_fresh_process(engine, tmp_path):
    """one child after another, each under its own timeout, stopping at the first that fails"""
    for key in ("b40", "rfc1024"):
        grp, b, _ = kit(engine, key)
        cases = MC.chunk_cases(b)
        want = [one(engine, grp, c) for c in cases]
        assert all(w[0] == 0 and w[1] == b.expected(c) for w, c in zip(want, cases))
        path = str(tmp_path / f"secrets_{key}.json")
        with open(path, "w") as fh:
            json.dump([dict(positions=list(c.positions), shares=b"".join(c.shares).hex()) for c in cases], fh)
        env = dict(os.environ, MPVSS_MAX_CHUNK=str(MC.CHUNK))
        out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child", key, path],
                             capture_output=True, text=True, env=env)
        assert out.returncode == 0, f"group {key}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
        res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert [(s, bytes.fromhex(gs), bytes.fromhex(mask)) for s, gs, mask in res["got"]] == want
        assert res["stats"] == MC.CHUNK_STATS


# ---- (7) after other calls on the same workspace -----------------------------------------------------------------------
def test_after_other_calls_on_the_same_workspace(engine):
    import modp_rt_many_helpers as M
    from mpvss_rs_amd import ModpGroup
    grp, b, _ = kit(engine, "b40")
    cases = MC.segment_cases(b)[:9] + MC.small_cases(b, 5)
    want = [one(engine, grp, c) for c in cases]
    boxes = M.case("256")["run"]                                            # rt_run_boxes holds a box table afterwards
    g256 = ModpGroup(M.GROUPS["256"][0]())
    assert [v for v, _ in engine.group_verify_many(g256, boxes)] == [True] * len(boxes)
    wide, bw, _ = kit(engine, "rfc3072")
    big = bw.shape_case(33)
    assert one(engine, wide, big)[1] == bw.expected(big)
    assert many(engine, grp, cases) == want
    assert one(engine, grp, cases[8]) == want[8]                            # a plain one-secret call still gives its bytes
    assert many(engine, wide, [big, bw.shape_case(3)]) == [one(engine, wide, big), one(engine, wide, bw.shape_case(3))]
    assert many(engine, grp, cases) == want


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    child(sys.argv[2], sys.argv[3])
