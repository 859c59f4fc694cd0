"""`reconstruct` of the three fixed groups (mpvss_modp_reconstruct, mpvss_ec_reconstruct) at its shape and operand edges, on one
engine: the one-workgroup sum of the curves across its wave, workgroup and stride-loop edges and in place over the stale points of
larger calls; the pairwise fold of MODP at every parity pattern and across the row / quad switch of the exponentiations; positions
at both ends of int64 in three orders; signs of unsorted positions; the identity, equal, opposite, non-residue, unreduced and zero
shares; shares in HBM; the mask and the refusals.  tests/test_gpu_reconstruct.py holds a dealt box of n = 9 and one MODP run at
m = 300; the cases and their reference are in tests/reconstruct_cases.py, held to the oracle by tests/test_reconstruct_cases.py.
Every comparison is of bytes.

Measured on an MI355X: 43 tests in 23 s.  test_shapes_around_4096 (three calls at 4097, 4096, 4097 and one at 257) takes 12.9 s for
MODP -- the host's quadratic Lagrange loop at 32 limbs, about 4 s a call -- and 2.1 / 2.3 s for the curves; every other test is below
one second."""
import pytest

import reconstruct_cases as K
from mpvss_rs_amd import capi

pytestmark = pytest.mark.gpu
GID = {"modp2048": 0, "secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}
_KITS = {}


def kit(engine, name):
    """(builder whose shares come from the engine's fixed-base calls, memo of the reference's factors) of a group"""
    if name not in _KITS:
        G = K.O.GROUPS[name]()
        if name == "modp2048":
            def power(exps):
                out = engine.batch_exp_fixed_base((2).to_bytes(256, "big"), b"".join(e.to_bytes(256, "big") for e in exps))
                return [out[k:k + 256] for k in range(0, len(out), 256)]
        else:
            def power(exps):
                out = engine.ec_batch_exp_generator(GID[name], b"".join(G.scalar_to_fixed(e) for e in exps))
                return [out[k:k + G.elem_len] for k in range(0, len(out), G.elem_len)]
        _KITS[name] = (K.Builder(name, power), {})
    return _KITS[name]


def run(engine, name, positions, shares, space="host", want_mask=True):
    data = b"".join(shares)
    if space == "host":
        if GID[name] == 0:
            return engine.reconstruct(positions, data, want_mask=want_mask)
        return engine.ec_reconstruct(GID[name], positions, data, want_mask=want_mask)
    import torch
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    if GID[name] == 0:
        res = engine.reconstruct_device(positions, buf.data_ptr(), len(positions), want_mask=want_mask)
    else:
        res = engine.ec_reconstruct_device(GID[name], positions, buf.data_ptr(), len(positions), want_mask=want_mask)
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == data, "the share buffer in HBM changed"
    return res


def check(engine, name, case, want=None, space="host"):
    """one case on the engine: G^s is the expected encoding and the mask is G.secret_mask of the returned element; a refusal is an
    EngineError.  want: the expectation where the caller has computed it already"""
    b, memo = kit(engine, name)
    if want is None:
        want = b.expected(case, memo)
    if want is None:
        with pytest.raises(capi.EngineError):
            run(engine, name, case.positions, case.shares, space)
        return None
    gs, mask = run(engine, name, case.positions, case.shares, space)
    assert gs == want, (case.id, space)
    assert mask == b.mask(gs), (case.id, space)
    return gs


def small_call_is_right(engine, name):
    """the m = 3 call after a refusal"""
    check(engine, name, kit(engine, name)[0].shape_case(3))


# ---- A: shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.NAMES)
def test_shapes_descending_then_ascending(engine, name):
    """every size after a larger one and after a smaller one, on one context: a kernel that reads past m meets the points of the
    larger call"""
    b, _ = kit(engine, name)
    cases = [b.shape_case(m) for m in K.SHAPE_M[name]]
    want = [b.expected(c) for c in cases]
    for c, w in list(zip(cases, want))[::-1] + list(zip(cases, want)):
        check(engine, name, c, w)


@pytest.mark.parametrize("name", K.NAMES)
def test_shapes_around_4096(engine, name):
    """the sizing rule of the curves' validity flags and the row / quad switch of MODP's exponentiations; the host's quadratic
    Lagrange loop is most of the time"""
    b, _ = kit(engine, name)
    cases = [b.shape_case(m) for m in K.SHAPE_M_BIG]
    want = [b.expected(c) for c in cases]
    for k in (1, 0, 1):
        check(engine, name, cases[k], want[k])
    check(engine, name, b.shape_case(257))


# ---- B: positions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", K.POSITION_M)
@pytest.mark.parametrize("name", K.NAMES)
def test_positions_to_both_ends_of_int64_in_three_orders(engine, name, m):
    b, memo = kit(engine, name)
    cases = b.position_cases(m)
    want = b.expected(cases["asc"])
    got = {order: check(engine, name, c, want) for order, c in cases.items()}
    assert got["asc"] == got["desc"] == got["shuffled"]
    if m == 17:
        asc = cases["asc"]
        assert b.G.element_to_fixed(K.ref_reconstruct(b.G, asc.positions, b.elements(asc), memo)) == got["asc"]


# ---- C: signs and degenerate shares ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", K.SIGN_M)
@pytest.mark.parametrize("name", K.NAMES)
def test_signs_and_degenerate_shares(engine, name, m):
    b, _ = kit(engine, name)
    kinds = set()
    for case in b.sign_cases(m):
        kinds.add(case.expect[0])
        if check(engine, name, case) is None:
            check(engine, name, b.sign_cases(m)[0])               # the very next call on the same context is right
            small_call_is_right(engine, name)
    assert kinds == ({"ref", "refuse"} if name == "modp2048" else {"ref"})


@pytest.mark.parametrize("lane", K.LANES_257)
@pytest.mark.parametrize("name", K.CURVES)
def test_identity_on_one_lane_of_257(engine, name, lane):
    check(engine, name, kit(engine, name)[0].lane_case_257(lane))


# ---- D: device space ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", K.DEVICE_M)
@pytest.mark.parametrize("name", K.NAMES)
def test_shares_in_hbm(engine, name, m):
    case = kit(engine, name)[0].shape_case(m)
    host = check(engine, name, case)
    assert check(engine, name, case, host, space="device") == host


# ---- E: mask and arguments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.NAMES)
def test_without_the_mask(engine, name):
    b, _ = kit(engine, name)
    for case in (b.shape_case(3), b.shape_case(65 if name != "modp2048" else 33), b.sign_cases(5)[0]):
        gs = check(engine, name, case)
        for space in ("host", "device"):
            assert run(engine, name, case.positions, case.shares, space, want_mask=False) == (gs, None)


@pytest.mark.parametrize("name", K.NAMES)
def test_refusals_leave_the_context_usable(engine, name):
    b, _ = kit(engine, name)
    big = b.shape_case(257)
    dup = list(big.positions)
    dup[-1] = dup[0]                                              # the two ends of the list
    three = b.shape_case(3)
    bad = [(dup, big.shares)]
    for x in (0, -1):
        for lane in range(3):
            xs = list(three.positions)
            xs[lane] = x
            bad.append((xs, three.shares))
    bad.append(([], []))
    for xs, shares in bad:
        with pytest.raises(capi.EngineError):
            run(engine, name, xs, shares)
        small_call_is_right(engine, name)
    with pytest.raises(capi.EngineError):
        run(engine, name, dup, big.shares, space="device")
    small_call_is_right(engine, name)
