"""The Lagrange exponents of the run-time MODP groups on the device (k_rt_lagrange_terms, the denominators' Fermat powers,
k_rt_lagrange_finish; mpvss_ctx_set_rt_lagrange, mpvss_modp_group_lagrange_exponents, mpvss_modp_group_lagrange_stats), against
Python integers (tests/modp_rt_lagrange_cases.py) and against the host path of the same engine, byte for byte, at every width.

(1) the exponents on their own under mode 2 over every case: the reference, mode 0, and what the stats say; (2) refusals under mode
2; (3) fallbacks: q = 23 and a composite (q-1)/2; (4) group_reconstruct under modes 0 and 2, in host and device space; (5)
group_reconstruct_many under both modes: thirteen lists in ONE pass of launches, shared lists counted once, refused and fallback
lists between good ones, shares in HBM; (6) pass boundaries in a fresh child process with MPVSS_MAX_CHUNK=32 -- this file is its own
child: `python test_gpu_modp_rt_lagrange.py child <group> <secrets.json>`; (7) 4097 positions at 40 bits.  Every test leaves the
engine in the mode it found.

Measured on an MI355X: 24 tests in 14.9 s.  Seconds: exponents_on_the_device 0.24 / 1.54 / 3.37 / 0.82 / 1.81 (40, 1024, 2048, 3072,
4096 bits; at 1024 and 2048 bits most of it the Python reference), four_thousand_and_ninety_seven_positions 1.59, pass_boundaries
(two children) 1.27, one_secret_under_both_modes 0.01 / 0.25 / 0.60 / 1.20, segment_lists_at_the_other_widths 0.04 / 0.24 / 0.78;
every other test below 0.2."""
import contextlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import modp_rt_lagrange_cases as LC
import modp_rt_reconstruct_cases as K
import modp_rt_reconstruct_many_cases as MC

pytestmark = pytest.mark.gpu
_GROUPS = {}
_KITS = {}
MANY_STATS = ("passes", "grouped_secrets", "single_secrets")


@contextlib.contextmanager
def mode(engine, m):
    before = engine.set_rt_lagrange(m)
    try:
        yield
    finally:
        assert engine.set_rt_lagrange(before) == m


def group(key):
    """the handle of a key of LC.HANDLES, or of a modulus given as an integer (256-byte elements)"""
    from mpvss_rs_amd import ModpGroup
    if key not in _GROUPS:
        if isinstance(key, int):
            _GROUPS[key] = ModpGroup(key)
        else:
            q, eb, lpl = LC.modulus(key), LC.HANDLES[key][1], LC.HANDLES[key][2]
            _GROUPS[key] = ModpGroup(q, elem_bytes=eb)
            assert _GROUPS[key].limbs_per_lane == lpl and _GROUPS[key].elem_bytes == eb, key
    return _GROUPS[key]


def kit(engine, key):
    """(handle, builder whose shares come from the handle's fixed-base call) of a group of modp_rt_reconstruct_cases"""
    if key not in _KITS:
        from mpvss_rs_amd import ModpGroup
        eb = K.GROUPS[key][1]
        grp = ModpGroup(K.modulus(key), elem_bytes=eb)

        def power(base, exps):
            out = engine.group_batch_exp_fixed_base(grp, base.to_bytes(eb, "big"), b"".join(e.to_bytes(eb, "big") for e in exps))
            return [out[k:k + eb] for k in range(0, len(out), eb)]

        _KITS[key] = (grp, K.RtBuilder(key, power))
    return _KITS[key]


def lag_delta(engine, fn):
    s0 = engine.group_lagrange_stats()
    out = fn()
    s1 = engine.group_lagrange_stats()
    return out, tuple(s1[k] - s0[k] for k in ("device", "host", "fallback"))


def differing(got, want, eb):
    return [k for k in range(len(want) // eb) if got[eb * k:eb * k + eb] != want[eb * k:eb * k + eb]][:8]


def refusal(eb):
    return (-1, bytes(eb), bytes(32))


def one(engine, grp, case):
    from mpvss_rs_amd import capi
    try:
        gs, mask = engine.group_reconstruct(grp, case.positions, None if case.shares is None else b"".join(case.shares))
    except capi.EngineError as e:
        assert "rc=-1" in str(e), case.id
        return refusal(grp.elem_bytes)
    return (0, gs, mask)


def many(engine, grp, cases, **kw):
    return engine.group_reconstruct_many(grp, [MC.as_secret(c) for c in cases], **kw)


def both_modes(engine, fn):
    """(result, Lagrange stats delta, reconstruct_many stats delta) of fn under mode 0 and under mode 2"""
    out = []
    for m in (0, 2):
        s0 = engine.group_reconstruct_many_stats()
        with mode(engine, m):
            got, d = lag_delta(engine, fn)
        s1 = engine.group_reconstruct_many_stats()
        out.append((got, d, tuple(s1[k] - s0[k] for k in MANY_STATS)))
    return out


# ---- (1) the exponents on their own ------------------------------------------------------------------------------------
def test_the_default_mode_is_automatic(engine):
    from mpvss_rs_amd import capi
    assert engine.set_rt_lagrange(1) == 1
    with pytest.raises(capi.EngineError):
        engine.set_rt_lagrange(3)
    with pytest.raises(capi.EngineError):
        engine.set_rt_lagrange(-1)
    assert engine.set_rt_lagrange(1) == 1


@pytest.mark.parametrize("key", LC.KEYS)
def test_exponents_on_the_device_equal_the_reference_and_the_host(engine, key):
    grp, eb = group(key), LC.HANDLES[key][1]
    for cid, xs in LC.cases(key):
        want = LC.expected_of(key, cid, xs)
        with mode(engine, 2):
            got, d = lag_delta(engine, lambda: engine.group_lagrange_exponents(grp, xs))
        assert d == (1, 0, 0), (key, cid)
        assert got == want, (key, cid, differing(got, want, eb))
        with mode(engine, 0):
            host, d = lag_delta(engine, lambda: engine.group_lagrange_exponents(grp, xs))
        assert d == (0, 1, 0) and host == want, (key, cid)


# ---- (2) refusals ------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_path(engine):
    import ctypes as C
    grp, eb = group("b40"), 256
    long_list = list(range(1, 601))
    bad = {"empty": [],
           "position-0": [3, 0, 5],
           "negative": [3, -7, 5],
           "duplicate-ends": [4, 2, 9, 4],
           "duplicate-in-two-tiles": long_list[:100] + [long_list[400]] + long_list[101:]}       # indices 100 and 400: tiles 6 and 25
    assert bad["duplicate-in-two-tiles"][100] == bad["duplicate-in-two-tiles"][400] and 100 // LC.TILE != 400 // LC.TILE
    with mode(engine, 2):
        for what, xs in bad.items():
            pos = (C.c_int64 * max(len(xs), 1))(*xs)
            out = (C.c_uint8 * (eb * max(len(xs), 1)))(*([0xA5] * (eb * max(len(xs), 1))))

            def call():
                return engine.lib.mpvss_modp_group_lagrange_exponents(engine.ctx, grp.handle, C.cast(pos, C.c_void_p), len(xs),
                                                                      C.cast(out, C.c_void_p))

            rc, d = lag_delta(engine, call)
            assert rc == -1 and d == (0, 0, 0), what
            assert bytes(out) == b"\xa5" * len(out), what
        out = (C.c_uint8 * eb)()
        pos = (C.c_int64 * 1)(1)
        assert engine.lib.mpvss_modp_group_lagrange_exponents(engine.ctx, grp.handle, None, 1, C.cast(out, C.c_void_p)) == -1
        assert engine.lib.mpvss_modp_group_lagrange_exponents(engine.ctx, grp.handle, C.cast(pos, C.c_void_p), 1, None) == -1
        # and the engine goes on
        assert engine.group_lagrange_exponents(grp, [3, 1, 2]) == LC.expected(LC.modulus("b40"), eb, [3, 1, 2])


# ---- (3) fallbacks -----------------------------------------------------------------------------------------------------
def test_fallbacks_at_q23(engine):
    import ctypes as C
    from mpvss_rs_amd import capi
    grp = group(LC.Q23)
    with mode(engine, 0):
        host_value = engine.group_lagrange_exponents(grp, LC.Q23_VALUE)
        host_device = engine.group_lagrange_exponents(grp, LC.Q23_ON_DEVICE)
    assert host_value == LC.expected(LC.Q23, 256, LC.Q23_VALUE) and host_device == LC.expected(LC.Q23, 256, LC.Q23_ON_DEVICE)
    assert LC.expected(LC.Q23, 256, LC.Q23_REFUSED) is None
    with mode(engine, 2):
        got, d = lag_delta(engine, lambda: engine.group_lagrange_exponents(grp, LC.Q23_VALUE))
        assert got == host_value and d == (0, 1, 1)                      # a value through the reduced fraction
        pos = (C.c_int64 * 2)(*LC.Q23_REFUSED)
        out = (C.c_uint8 * 512)(*([0xA5] * 512))
        rc, d = lag_delta(engine, lambda: engine.lib.mpvss_modp_group_lagrange_exponents(engine.ctx, grp.handle, C.cast(pos, C.c_void_p),
                                                                                         2, C.cast(out, C.c_void_p)))
        assert rc == -1 and d == (0, 0, 0) and bytes(out) == b"\xa5" * 512   # a refusal: in none of the counts
        with pytest.raises(capi.EngineError, match="no inverse"):
            engine.group_lagrange_exponents(grp, LC.Q23_REFUSED)
        got, d = lag_delta(engine, lambda: engine.group_lagrange_exponents(grp, LC.Q23_ON_DEVICE))
        assert got == host_device and d == (1, 0, 0)                     # units throughout, magnitudes 0: stays on the device
        ints = [int.from_bytes(got[256 * k:256 * k + 256], "big") for k in range(3)]
        assert ints == [1, 0, 0] and LC.signs(LC.Q23_ON_DEVICE) == [False, True, False]   # 0 under a negative sign stays 0


def test_a_composite_subgroup_order_falls_back(engine):
    grp = group(LC.COMPOSITE_Q)
    assert grp.limbs_per_lane == LC.COMPOSITE_LPL
    for xs in LC.COMPOSITE_LISTS:
        want = LC.expected(LC.COMPOSITE_Q, 256, xs)
        with mode(engine, 0):
            host, dh = lag_delta(engine, lambda: engine.group_lagrange_exponents(grp, xs))
        with mode(engine, 2):
            dev, dd = lag_delta(engine, lambda: engine.group_lagrange_exponents(grp, xs))
        assert host == want and dev == want, differing(dev, want, 256)
        assert dh == (0, 1, 0) and dd == (0, 1, 1)


# ---- (4) one secret ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.WIDTHS)
def test_one_secret_under_both_modes(engine, key):
    import torch
    from mpvss_rs_amd import capi
    grp, b = kit(engine, key)
    for m in ([1, 3, 17, 65] if key in LC.WIDE else [1, 2, 3, 16, 17, 257]):
        case = b.shape_case(m)
        shares = b"".join(case.shares)
        with mode(engine, 0):
            host, dh = lag_delta(engine, lambda: engine.group_reconstruct(grp, case.positions, shares))
        with mode(engine, 2):
            dev, dd = lag_delta(engine, lambda: engine.group_reconstruct(grp, case.positions, shares))
        assert dh == (0, 1, 0) and dd == (1, 0, 0), (key, m)
        assert dev == host and host[0] == b.expected(case) and host[1] == b.mask(host[0]), (key, m)
        if m in (3, 17):
            buf = torch.frombuffer(bytearray(shares), dtype=torch.uint8).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            for md in (0, 2):
                with mode(engine, md):
                    assert engine.group_reconstruct_device(grp, case.positions, buf.data_ptr(), m) == host, (key, m, md)
            torch.cuda.synchronize()
            assert buf.cpu().numpy().tobytes() == shares, "the share buffer in HBM changed"
    three = b.shape_case(3)
    zero_neg = [c for c in b.sign_cases(5) if c.id.endswith("zero-neg")][0] if key in K.SIGN_KEYS else None
    with mode(engine, 2):
        for xs in ([1, 2, 1], [1, 0, 2]):
            with pytest.raises(capi.EngineError, match="rc=-1"):
                engine.group_reconstruct(grp, xs, b"".join(three.shares))
        with pytest.raises(capi.EngineError, match="duplicate positions"):
            engine.group_reconstruct(grp, [1, 2, 1], b"".join(three.shares))
        if zero_neg:                                                        # the zero-share check reads the host's signs
            assert one(engine, grp, zero_neg) == refusal(grp.elem_bytes)
            for c in b.sign_cases(5) if key == "rfc1024" else []:           # (the reference's pow: cheap at 1024 bits only)
                if c.expect[0] == "ref":
                    assert one(engine, grp, c)[1] == b.expected(c), c.id


# ---- (5) many secrets --------------------------------------------------------------------------------------------------
def test_thirteen_lists_in_one_pass_of_launches(engine):
    grp, b = kit(engine, "b40")
    cases = MC.segment_cases(b)
    assert len(cases) == 13
    want = [(0, b.expected(c), b.mask(b.expected(c))) for c in cases]
    for order in (cases, cases[::-1]):
        w = want if order is cases else want[::-1]
        (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, grp, order))
        assert host == w and dev == w, [c.id for c, g, x in zip(order, dev, w) if g != x]
        assert dh == (0, 13, 0) and dd == (13, 0, 0)
        assert sh == sd == (1, 13, 0)                                       # the passes do not depend on the mode
    with mode(engine, 2):
        many(engine, grp, cases)
        assert engine.lib.mpvss_last_kernel_ms(engine.ctx, 4) > 0           # the coefficient launches are kind 4
        assert engine.lib.mpvss_last_kernel_launches(engine.ctx, 4) == 4    # terms, tables, powers, finish: one chunk


@pytest.mark.parametrize("key", ["rfc1024", "rfc2048", "rfc3072"])
def test_segment_lists_at_the_other_widths(engine, key):
    grp, b = kit(engine, key)
    cases = [c for c in MC.segment_cases(b) if len(c.positions) in (1, 3, 16, 17, 33)]
    want = [(0, b.expected(c), b.mask(b.expected(c))) for c in cases]
    (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, grp, cases))
    assert host == want and dev == want
    assert dh == (0, 5, 0) and dd == (5, 0, 0) and sh == sd == (1, 5, 0)


def test_equal_lists_are_computed_once(engine):
    grp, b = kit(engine, "b40")
    cases = MC.sharing_cases(b)
    want = [(0, b.expected(c), b.mask(b.expected(c))) for c in cases]
    (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, grp, cases))
    assert host == want and dev == want
    assert dh == (0, 3, 0) and dd == (3, 0, 0)                              # ten secrets over three lists
    assert sh == sd == (1, 10, 0)


def test_refused_lists_between_good_ones(engine):
    grp, b = kit(engine, "b40")
    pairs = MC.refused_between_good(b)
    cases = [c for c, _ in pairs]
    want = [refusal(256) if r else (0, b.expected(c), b.mask(b.expected(c))) for c, r in pairs]
    (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, grp, cases))
    assert host == want and dev == want
    # the lists that have exponents: those of the good secrets and of the secret refused for its zero share
    lists = {tuple(c.positions) for c, r in pairs if not r or c.id.endswith("zero-neg")}
    assert dh == (0, len(lists), 0) and dd == (len(lists), 0, 0)
    assert sh == sd == (1, sum(not r for _, r in pairs), 0)
    bad = [c for c, r in pairs if r and not c.id.endswith("zero-neg")]
    (host, dh, _), (dev, dd, _) = both_modes(engine, lambda: many(engine, grp, bad))
    assert host == dev == [refusal(256)] * len(bad) and dh == dd == (0, 0, 0)   # refused lists are in none of the counts


def test_fallback_lists_between_good_ones_at_q23(engine):
    grp, b = kit(engine, "q23")
    memo = {}
    pairs = MC.tiny_refused_between_good(b, lambda c: b.reference(c, memo))
    cases = [c for c, _ in pairs]
    want = [refusal(256) if r else (0, b.reference(c, memo), b.mask(b.reference(c, memo))) for c, r in pairs]
    (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, grp, cases))
    assert host == want and dev == want, [c.id for c, g, x in zip(cases, dev, want) if g != x]
    good = {tuple(c.positions) for c, r in pairs if not r}
    fell = {xs for xs in good if LC.raw_denominator_vanishes(xs, 11)}
    assert dh == (0, len(good), 0)
    assert dd == (len(good) - len(fell), len(fell), len(fell))              # the refused lists were tried too and count nowhere
    assert sh == sd
    # a list that falls back to a value between lists that stay on the device
    mixed = [[1, 2, 3], LC.Q23_VALUE, [3, 4], LC.Q23_REFUSED, LC.Q23_ON_DEVICE]
    secrets = []
    for xs in mixed:
        shares, _ = b.dealt(xs, 2, 9900 + len(secrets))
        secrets.append(K.Case(f"M-{len(secrets)}", xs, shares, ("oracle", None)))
    (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, grp, secrets))
    assert host == dev and [h[0] for h in host] == [0, 0, 0, -1, 0]
    assert [h[1] for h in host if h[0] == 0] == [b.reference(c, memo) for c in secrets if c.positions != LC.Q23_REFUSED]
    assert dh == (0, 4, 0) and dd == (3, 1, 1) and sh == sd


@pytest.mark.parametrize("key", ["b40", "rfc2048"])
def test_many_secrets_with_shares_in_hbm(engine, key):
    import torch
    grp, b = kit(engine, key)
    eb = grp.elem_bytes
    cases = [c for c in MC.segment_cases(b) if len(c.positions) in (1, 3, 16, 17, 33)] + MC.small_cases(b, 3)
    with mode(engine, 0):
        host = many(engine, grp, cases)
    assert [h[0] for h in host] == [0] * len(cases)
    data = b"".join(b"".join(c.shares) for c in cases)
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    secrets, at = [], 0
    for c in cases:
        secrets.append(dict(positions=list(c.positions), shares_ptr=buf.data_ptr() + at, m=len(c.positions)))
        at += len(c.positions) * eb
    (h, dh, sh), (d, dd, sd) = both_modes(engine, lambda: engine.group_reconstruct_many_device(grp, secrets))
    torch.cuda.synchronize()
    assert h == host and d == host and sh == sd == (1, len(cases), 0)
    assert dh == (0, len(cases), 0) and dd == (len(cases), 0, 0)
    with mode(engine, 2):
        assert engine.group_reconstruct_many_device(grp, secrets[:1]) == host[:1]                    # a run of one: the one-secret path
        assert engine.group_reconstruct_device(grp, cases[3].positions, secrets[3]["shares_ptr"], secrets[3]["m"]) == host[3][1:]
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == data, "the share buffers in HBM changed"


# ---- (6) pass boundaries, in a fresh child -----------------------------------------------------------------------------
def child(key, path):
    from mpvss_rs_amd import Engine, ModpGroup
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(MC.CHUNK)
    with open(path) as fh:
        secrets = [dict(positions=s["positions"], shares=bytes.fromhex(s["shares"])) for s in json.load(fh)]
    eng = Engine(0)
    assert eng.set_rt_lagrange(2) == 1
    grp = ModpGroup(K.modulus(key), elem_bytes=K.GROUPS[key][1])
    got = eng.group_reconstruct_many(grp, secrets)
    launches = eng.lib.mpvss_last_kernel_launches(eng.ctx, 4)
    print("RESULT " + json.dumps(dict(got=[[s, gs.hex(), mask.hex()] for s, gs, mask in got], stats=eng.group_reconstruct_many_stats(),
                                      lagrange=eng.group_lagrange_stats(), launches=launches)))
    eng.close()


def test_pass_boundaries_in_a_fresh_process(engine, tmp_path):
    """one child after another, each under its own timeout, stopping at the first that fails.  The exponents of three passes are
    gathered from the call's one buffer, which two tiles at a time filled (MPVSS_MAX_CHUNK = 32 slots); the secret of 33 shares
    between them is a SINGLE secret and computes its own, the trailing run of one takes its list's from the buffer."""
    for key in ("b40", "rfc1024"):
        grp, b = kit(engine, key)
        cases = MC.chunk_cases(b)
        want = [(0, b.expected(c), b.mask(b.expected(c))) for c in cases]
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
        # distinct lists of at most 32 positions: 16 (twice), 3, 5, 20, 7, 17 -- six in the one pass of launches -- and the single of 33
        assert res["lagrange"] == {"device": 7, "host": 0, "fallback": 0}
        # tiles of the six lists: 1 + 1 + 1 + 2 + 1 + 2 = 8, two per chunk: four chunks of four launches among the last pass's times
        assert res["launches"] == 16


# ---- (7) 257 workgroups, seventeen staging trips -----------------------------------------------------------------------
def test_four_thousand_and_ninety_seven_positions(engine):
    grp = group("b40")
    xs, want = LC.big_expected()
    with mode(engine, 2):
        got, d = lag_delta(engine, lambda: engine.group_lagrange_exponents(grp, xs))
    assert d == (1, 0, 0)
    assert got == want, differing(got, want, 256)


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    child(sys.argv[2], sys.argv[3])
