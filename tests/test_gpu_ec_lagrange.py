"""k_ec_lagrange: the Lagrange coefficients of the curve groups on the device (mpvss_ctx_set_ec_lagrange, mpvss_ec_lagrange_scalars,
mpvss_ec_lagrange_stats), against Python integers (tests/ec_lagrange_cases.py) and against the host path of the same engine, byte
for byte.  Both curves.

(1) the kernel on its own under mode 2 over every case: the reference, mode 0, and what the stats say; (2) refusals under mode 2;
(3) ec_reconstruct under mode 2 against mode 0; (4) ec_reconstruct_many under mode 2 against mode 0 and the builder's closed form:
thirteen lists in ONE launch, shared lists counted once, refused lists between good ones, shares in HBM; (5) pass boundaries in a
fresh child process with MPVSS_MAX_CHUNK=32 -- this file is its own child: `python test_gpu_ec_lagrange.py child <curve>
<secrets.json>`; (6) m = 4097 through the kernel on its own.  Every test leaves the engine in the mode it found.

Measured on an MI355X: 18 tests in 5.8 s.  Seconds: four_thousand_and_ninety_seven_positions 1.27 / 1.21 (secp256k1 /
ristretto255: nearly all of it the Python reference), pass_boundaries (two children) 1.17, refused_lists_between_good_ones
0.08 / 0.37, scalars_on_the_device_equal_the_reference_and_the_host 0.23 / 0.22, one_secret_under_both_modes 0.11 / 0.08,
thirteen_lists_in_one_launch 0.11 / 0.04; every other test below 0.1."""
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

import ec_lagrange_cases as LC
import ec_reconstruct_many_cases as MC
import reconstruct_cases as K

pytestmark = pytest.mark.gpu
GID = {"secp256k1": 1, "ristretto255": 2}
_KITS = {}
MANY_STATS = ("passes", "grouped_secrets", "single_secrets")


@contextlib.contextmanager
def mode(engine, m):
    before = engine.set_ec_lagrange(m)
    try:
        yield
    finally:
        assert engine.set_ec_lagrange(before) == m


def builder(engine, name):
    """a builder whose shares come from the engine's fixed-base call"""
    if name not in _KITS:
        G = K.O.GROUPS[name]()

        def power(exps):
            out = engine.ec_batch_exp_generator(GID[name], b"".join(G.scalar_to_fixed(e) for e in exps))
            return [out[k:k + G.elem_len] for k in range(0, len(out), G.elem_len)]

        _KITS[name] = K.Builder(name, power)
    return _KITS[name]


def lag_delta(engine, fn):
    s0 = engine.ec_lagrange_stats()
    out = fn()
    s1 = engine.ec_lagrange_stats()
    return out, (s1["device"] - s0["device"], s1["host"] - s0["host"])


def refusal(name):
    return (-1, bytes(33 if name == "secp256k1" else 32), bytes(32))


def many(engine, name, cases, **kw):
    return engine.ec_reconstruct_many(GID[name], [MC.as_secret(c) for c in cases], **kw)


# ---- (1) the kernel on its own -----------------------------------------------------------------------------------------
def test_the_default_mode_is_automatic(engine):
    assert engine.set_ec_lagrange(1) == 1
    from mpvss_rs_amd import capi
    with pytest.raises(capi.EngineError):
        engine.set_ec_lagrange(3)
    with pytest.raises(capi.EngineError):
        engine.set_ec_lagrange(-1)
    assert engine.set_ec_lagrange(1) == 1


@pytest.mark.parametrize("name", LC.CURVES)
def test_scalars_on_the_device_equal_the_reference_and_the_host(engine, name):
    for cid, xs in LC.cases():
        want = LC.expected_of(name, cid, xs)
        with mode(engine, 2):
            got, d = lag_delta(engine, lambda: engine.ec_lagrange_scalars(GID[name], xs))
        assert d == (1, 0), cid
        assert got == want, (name, cid, [k for k in range(len(xs)) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]][:8])
        with mode(engine, 0):
            host, d = lag_delta(engine, lambda: engine.ec_lagrange_scalars(GID[name], xs))
        assert d == (0, 1) and host == want, (name, cid)


# ---- (2) refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.CURVES)
def test_refusals_on_the_device_path(engine, name):
    import ctypes as C
    long_list = list(range(1, 601))
    bad = {"empty": [],
           "position-0": [3, 0, 5],
           "negative": [3, -7, 5],
           "duplicate-ends": [4, 2, 9, 4],
           "duplicate-middle": [1, 6, 6, 2],
           "duplicate-in-two-tiles": long_list[:100] + [long_list[400]] + long_list[101:]}       # indices 100 and 400: LDS tiles 0 and 1
    assert bad["duplicate-in-two-tiles"][100] == bad["duplicate-in-two-tiles"][400] and 100 // LC.STAGE != 400 // LC.STAGE
    with mode(engine, 2):
        for what, xs in bad.items():
            pos = (C.c_int64 * max(len(xs), 1))(*xs)
            out = (C.c_uint8 * (32 * max(len(xs), 1)))(*([0xA5] * (32 * max(len(xs), 1))))

            def call():
                return engine.lib.mpvss_ec_lagrange_scalars(engine.ctx, GID[name], C.cast(pos, C.c_void_p), len(xs), C.cast(out, C.c_void_p))

            rc, d = lag_delta(engine, call)
            assert rc == -1 and d == (0, 0), what
            assert bytes(out) == b"\xa5" * len(out), what
        out = (C.c_uint8 * 32)()
        pos = (C.c_int64 * 1)(1)
        assert engine.lib.mpvss_ec_lagrange_scalars(engine.ctx, GID[name], None, 1, C.cast(out, C.c_void_p)) == -1
        assert engine.lib.mpvss_ec_lagrange_scalars(engine.ctx, GID[name], C.cast(pos, C.c_void_p), 1, None) == -1
        assert engine.lib.mpvss_ec_lagrange_scalars(engine.ctx, 7, C.cast(pos, C.c_void_p), 1, C.cast(out, C.c_void_p)) == -4    # MPVSS_E_UNSUPPORTED
        # and the engine goes on
        assert engine.ec_lagrange_scalars(GID[name], [3, 1, 2]) == LC.expected(name, [3, 1, 2])


# ---- (3) one secret ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.CURVES)
def test_one_secret_under_both_modes(engine, name):
    b = builder(engine, name)
    from mpvss_rs_amd import capi
    for m in LC.SIZES:
        case = b.shape_case(m)
        shares = b"".join(case.shares)
        with mode(engine, 0):
            host, dh = lag_delta(engine, lambda: engine.ec_reconstruct(GID[name], case.positions, shares))
        with mode(engine, 2):
            dev, dd = lag_delta(engine, lambda: engine.ec_reconstruct(GID[name], case.positions, shares))
        assert dh == (0, 1) and dd == (1, 0), m
        assert dev == host and host[0] == b.expected(case) and host[1] == b.mask(host[0]), (name, m)
    three = b.shape_case(3)
    with mode(engine, 2):
        for xs in ([1, 2, 1], [1, 0, 2]):
            with pytest.raises(capi.EngineError, match="rc=-1"):
                engine.ec_reconstruct(GID[name], xs, b"".join(three.shares))
        assert "duplicate positions" in _error_of(engine, name, [1, 2, 1], three)


def _error_of(engine, name, xs, case):
    from mpvss_rs_amd import capi
    try:
        engine.ec_reconstruct(GID[name], xs, b"".join(case.shares))
    except capi.EngineError as e:
        return str(e)
    return ""


# ---- (4) many secrets --------------------------------------------------------------------------------------------------
def both_modes(engine, fn):
    """(result, Lagrange stats delta, reconstruct_many stats delta) of fn under mode 0 and under mode 2"""
    out = []
    for m in (0, 2):
        s0 = engine.ec_reconstruct_many_stats()
        with mode(engine, m):
            got, d = lag_delta(engine, fn)
        s1 = engine.ec_reconstruct_many_stats()
        out.append((got, d, tuple(s1[k] - s0[k] for k in MANY_STATS)))
    return out


@pytest.mark.parametrize("name", LC.CURVES)
def test_thirteen_lists_in_one_launch(engine, name):
    b = builder(engine, name)
    cases = MC.segment_cases(b)
    want = [(0, b.expected(c), b.mask(b.expected(c))) for c in cases]
    for order in (cases, cases[::-1]):
        w = want if order is cases else want[::-1]
        (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, name, order))
        assert host == w and dev == w, [c.id for c, g, x in zip(order, dev, w) if g != x]
        assert dh == (0, 13) and dd == (13, 0)
        assert sh == sd == (1, 13, 0)                                           # the passes do not depend on the mode


@pytest.mark.parametrize("name", LC.CURVES)
def test_equal_lists_are_computed_once(engine, name):
    b = builder(engine, name)
    cases = MC.sharing_cases(b)
    want = [(0, b.expected(c), b.mask(b.expected(c))) for c in cases]
    (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, name, cases))
    assert host == want and dev == want
    assert dh == (0, 3) and dd == (3, 0)                                        # ten secrets over three lists
    assert sh == sd == (1, 10, 0)


@pytest.mark.parametrize("name", LC.CURVES)
def test_refused_lists_between_good_ones(engine, name):
    b = builder(engine, name)
    pairs = MC.refused_between_good(b)
    cases = [c for c, _ in pairs]
    want = [refusal(name) if r else (0, b.expected(c), b.mask(b.expected(c))) for c, r in pairs]
    (host, dh, sh), (dev, dd, sd) = both_modes(engine, lambda: many(engine, name, cases))
    assert host == want and dev == want
    # the lists that have coefficients: those of the good secrets and of the secret with a rejected encoding
    lists = {tuple(c.positions) for c, r in pairs if not r or c.id == "R-encoding"}
    assert dh == (0, len(lists)) and dd == (len(lists), 0)
    assert sh == sd == (1, sum(not r for _, r in pairs), 0)
    bad = [c for c, r in pairs if r and c.id != "R-encoding"]
    (host, dh, _), (dev, dd, _) = both_modes(engine, lambda: many(engine, name, bad))
    assert host == dev == [refusal(name)] * len(bad) and dh == dd == (0, 0)     # refused lists are in neither count


@pytest.mark.parametrize("name", LC.CURVES)
def test_many_secrets_with_shares_in_hbm(engine, name):
    import torch
    b = builder(engine, name)
    cases = MC.segment_cases(b) + [c for c, _ in MC.refused_between_good(b) if c.shares is not None and len(c.positions) > 0]
    with mode(engine, 0):
        host = many(engine, name, cases)
    assert sum(h == refusal(name) for h in host) == 3
    off = 1 if name == "secp256k1" else 0
    datas = [bytes(off) + b"".join(c.shares) for c in cases]
    bufs = [torch.frombuffer(bytearray(d), dtype=torch.uint8).to(torch.device("cuda", 0)) for d in datas]
    torch.cuda.synchronize()
    secrets = [dict(positions=list(c.positions), shares_ptr=buf.data_ptr() + off, m=len(c.positions)) for c, buf in zip(cases, bufs)]
    (h, dh, sh), (d, dd, sd) = both_modes(engine, lambda: engine.ec_reconstruct_many_device(GID[name], secrets))
    torch.cuda.synchronize()
    assert h == host and d == host and sh == sd
    assert dh[0] == 0 and dd[1] == 0 and dd[0] == dh[1] > 13
    with mode(engine, 2):
        assert engine.ec_reconstruct_many_device(GID[name], secrets[:1]) == host[:1]                 # a run of one: the one-secret path
        assert engine.ec_reconstruct_device(GID[name], cases[12].positions, secrets[12]["shares_ptr"], secrets[12]["m"]) == host[12][1:]
    torch.cuda.synchronize()
    for buf, data in zip(bufs, datas):
        assert buf.cpu().numpy().tobytes() == data, "a share buffer in HBM changed"


# ---- (5) pass boundaries, in a fresh child -----------------------------------------------------------------------------
def child(name, path):
    from mpvss_rs_amd import Engine
    assert os.environ.get("MPVSS_MAX_CHUNK") == str(MC.CHUNK)
    with open(path) as fh:
        secrets = [dict(positions=s["positions"], shares=bytes.fromhex(s["shares"])) for s in json.load(fh)]
    eng = Engine(0)
    assert eng.set_ec_lagrange(2) == 1
    got = eng.ec_reconstruct_many(GID[name], secrets)
    print("RESULT " + json.dumps(dict(got=[[s, gs.hex(), mask.hex()] for s, gs, mask in got], stats=eng.ec_reconstruct_many_stats(),
                                      lagrange=eng.ec_lagrange_stats())))
    eng.close()


def test_pass_boundaries_in_a_fresh_process(engine, tmp_path):
    """one child after another, each under its own timeout, stopping at the first that fails.  The coefficients of three passes are
    gathered from the call's one buffer; the secret of 33 shares between them is a SINGLE secret and computes its own, the trailing
    run of one takes its list's from the buffer."""
    for name in LC.CURVES:
        b = builder(engine, name)
        cases = MC.chunk_cases(b)
        want = [(0, b.expected(c), b.mask(b.expected(c))) for c in cases]
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
        # distinct lists of at most 32 positions: 16 (twice), 3, 5, 20, 7, 17 -- six in the one launch -- and the single of 33
        assert res["lagrange"] == {"device": 7, "host": 0}


# ---- (6) sixty-five workgroups, seventeen staging trips ----------------------------------------------------------------
@pytest.mark.parametrize("name", LC.CURVES)
def test_four_thousand_and_ninety_seven_positions(engine, name):
    xs = LC.shape_positions(LC.BIG_M)
    want = LC.expected_of(name, f"shuffled-{LC.BIG_M}", xs)
    with mode(engine, 2):
        got, d = lag_delta(engine, lambda: engine.ec_lagrange_scalars(GID[name], xs))
    assert d == (1, 0)
    assert got == want, [k for k in range(len(xs)) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]][:8]


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    child(sys.argv[2], sys.argv[3])
