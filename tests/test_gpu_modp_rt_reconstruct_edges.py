"""`reconstruct` of the run-time MODP groups (mpvss_modp_group_reconstruct) at its shape, modulus and operand edges, on one engine
and eight handles from q = 23 to RFC 3526 group 15: the pairwise fold of rt_product_tree (to_mont, mul of the two halves, the copy
of the odd element) at every parity pattern, after larger and smaller calls and after calls of another limb width over the same
workspace; positions past q' = (q-1)/2 and congruent mod q', where the coefficient in lowest terms decides; every small position
set at q = 23 and q = 47 against the oracle itself; signs of unsorted positions with equal, unit, swapped, non-residue, unreduced
and zero shares; shares in HBM; the mask's reduction mod q; the refusals.  The cases and their reference are in
tests/modp_rt_reconstruct_cases.py, held to the oracle by tests/test_modp_rt_reconstruct_cases.py.  Every comparison is of bytes:
G^s at the handle's element width, and the mask against secret_mask of the returned element.

Measured on an MI355X: 46 tests in 20.4 s.  Seconds: the module's shapes fixture 2.6; shapes_descending_then_ascending 0.03 / 0.34 /
1.02 / 2.65 (40, 1024, 2048, 3072 bits); widths_interleaved 2.38; shape_4097 0.45; positions in three orders 0.99 and 0.31 at 3072
bits (m = 17 with the reference, m = 65), 0.32 and 0.11 at 2048, below 0.1 elsewhere; every_small_set 0.20 (q = 23, 1 470 sets) and
0.43 (q = 47, all 2 951 sets: no cut needed); signs_and_degenerate_shares 2.59 / 1.47 at 3072 bits (m = 17 / 5), 0.84 / 0.48 at 2048,
0.14 / 0.08 at 1024, below 0.03 at 64 and 256; shares_in_hbm 0.64 / 0.30 / 0.04 at 3072 bits (m = 257 / 65 / 1), 0.28 / 0.11 / 0.01 at
2048, 0.01 at 40; refusals 0.73 / 0.24 at 3072 / 2048 bits; every other test below 0.01.  Most of each figure is Python's pow in
the reference, not the engine.  One case of family B2 cannot exist: {q', 2q', 3} at the 64-bit prime, where 2q' = q - 1 is no int64."""
import pytest

import modp_rt_reconstruct_cases as K
import mpvss_oracle as O
from mpvss_rs_amd import ModpGroup, capi

pytestmark = pytest.mark.gpu
_KITS = {}


def kit(engine, key):
    """(handle, builder whose shares come from the handle's fixed-base call, memo of the reference's factors) of a group"""
    if key not in _KITS:
        q, eb = K.modulus(key), K.GROUPS[key][1]
        grp = ModpGroup(q, elem_bytes=eb)
        assert grp.limbs_per_lane == K.GROUPS[key][2] and grp.elem_bytes == eb, key

        def power(base, exps):
            out = engine.group_batch_exp_fixed_base(grp, base.to_bytes(eb, "big"), b"".join(e.to_bytes(eb, "big") for e in exps))
            return [out[k:k + eb] for k in range(0, len(out), eb)]

        _KITS[key] = (grp, K.RtBuilder(key, power), {})
    return _KITS[key]


def run(engine, key, positions, shares, space="host", want_mask=True):
    grp = kit(engine, key)[0]
    data = b"".join(shares)
    if space == "host":
        return engine.group_reconstruct(grp, positions, data, want_mask=want_mask)
    import torch
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    res = engine.group_reconstruct_device(grp, positions, buf.data_ptr(), len(positions), want_mask=want_mask)
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == data, "the share buffer in HBM changed"
    return res


def refused(engine, key, positions, shares, space="host"):
    with pytest.raises(capi.EngineError, match="rc=-1"):
        run(engine, key, positions, shares, space)


def check(engine, key, case, want=None, space="host"):
    """one case on the engine: G^s is the expected encoding and the mask is G.secret_mask of the returned element; a refusal is
    MPVSS_E_INVALID.  want: the expectation where the caller has computed it already"""
    _, b, memo = kit(engine, key)
    if want is None:
        want = b.expected(case, memo)
    if want is None:
        refused(engine, key, case.positions, case.shares, space)
        return None
    gs, mask = run(engine, key, case.positions, case.shares, space)
    assert gs == want, (key, case.id, space)
    assert mask == b.mask(gs), (key, case.id, space)
    return gs


def small_call_is_right(engine, key):
    """the m = 3 call after a refusal"""
    check(engine, key, kit(engine, key)[1].shape_case(3))


@pytest.fixture(scope="module")
def shapes(engine):
    """{(key, m): (case, expected bytes)} of family A at the four widths, made once"""
    out = {}
    for key in K.WIDTHS:
        b = kit(engine, key)[1]
        for m in K.SHAPE_M:
            c = b.shape_case(m)
            out[key, m] = (c, b.expected(c))
    return out


# ---- A: shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", K.WIDTHS)
def test_shapes_descending_then_ascending(engine, shapes, key):
    """every size after a larger one and after a smaller one on one context and one handle"""
    for m in K.SHAPE_M[::-1] + K.SHAPE_M:
        check(engine, key, *shapes[key, m])


def test_shapes_with_the_widths_interleaved(engine, shapes):
    """rt_tab1 and rt_out[0] hold the numbers of the call before at another stride"""
    for key, m in K.interleaved_order():
        check(engine, key, *shapes[key, m])


def test_shape_4097_at_40_bits(engine, shapes):
    """the ragged last workgroup; the host's quadratic Lagrange loop is one limb wide here"""
    check(engine, "b40", kit(engine, "b40")[1].shape_case(K.SHAPE_M_BIG))
    check(engine, "b40", *shapes["b40", 257])


# ---- B: positions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", K.POSITION_M)
@pytest.mark.parametrize("key", K.POSITION_KEYS)
def test_positions_to_both_ends_of_int64_in_three_orders(engine, key, m):
    _, b, memo = kit(engine, key)
    cases = b.position_cases(m)
    want = b.expected(cases["asc"])
    got = {order: check(engine, key, c, want) for order, c in cases.items()}
    assert got["asc"] == got["desc"] == got["shuffled"]
    if m == 17:
        assert b.reference(cases["asc"], memo) == got["asc"]


@pytest.mark.parametrize("key", K.SMALL_Q)
def test_positions_at_and_past_the_subgroup_order(engine, key):
    """the fraction in lowest terms decides between a value and a refusal (participant.rs:546-553)"""
    b = kit(engine, key)[1]
    for cases in b.small_q_cases():
        got = {check(engine, key, c) for c in cases}
        assert len(got) == 1
        if got == {None}:
            small_call_is_right(engine, key)


# ---- C: tiny moduli against the oracle itself --------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(K.TINY))
def test_every_small_set_at_a_tiny_modulus(engine, key):
    """every position set once through the engine: the oracle's mask where it has one, a refusal exactly where it returns None"""
    _, b, memo = kit(engine, key)
    value = none = gcd_sets = 0
    wrong = []                                                                       # every set that disagrees, not the first
    for c in b.tiny_cases():
        sbs, box = K.synthetic_box(b.G, c)
        want = O.reconstruct(b.G, sbs, box)                                          # U = 0: the mask itself
        try:
            got = run(engine, key, c.positions, c.shares)
        except capi.EngineError as e:
            assert "rc=-1" in str(e), (key, c.id)
            got = None
        if want is None:
            none += 1
            if got is not None:
                wrong.append((c.id, "a value where the oracle returns None"))
            continue
        value += 1
        gcd_sets += K.raw_denominator_vanishes(c.positions, b.sub)
        if got is None:
            wrong.append((c.id, "refused"))
        elif got != (b.reference(c, memo), want.to_bytes(32, "big")):
            wrong.append((c.id, "another value"))
    assert not wrong, (key, len(wrong), wrong)
    assert (value + none, value, none, gcd_sets) == K.TINY_COUNTS[key]
    small_call_is_right(engine, key)


# ---- D: signs and degenerate shares ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", K.SIGN_M)
@pytest.mark.parametrize("key", K.SIGN_KEYS)
def test_signs_and_degenerate_shares(engine, key, m):
    b = kit(engine, key)[1]
    kinds = set()
    for case in b.sign_cases(m):
        kinds.add(case.expect[0])
        if check(engine, key, case) is None:
            check(engine, key, b.sign_cases(m)[0])                # the very next call on the same context is right
            small_call_is_right(engine, key)
    assert kinds == {"ref", "refuse"}


# ---- E: device space, mask, refusals -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", K.DEVICE_M)
@pytest.mark.parametrize("key", K.DEVICE_KEYS)
def test_shares_in_hbm_and_without_the_mask(engine, key, m):
    case = kit(engine, key)[1].shape_case(m)
    host = check(engine, key, case)
    assert check(engine, key, case, host, space="device") == host
    for space in ("host", "device"):
        assert run(engine, key, case.positions, case.shares, space, want_mask=False) == (host, None)


@pytest.mark.parametrize("key", K.MASK_KEYS)
def test_mask_is_reduced_mod_q(engine, key):
    """int(SHA-256) mod q: never below q at 40 and 64 bits, on both sides of q at 256 bits"""
    b = kit(engine, key)[1]
    sides = {b.hash_below_q(check(engine, key, c)) for c in b.mask_cases()}
    assert sides == ({True, False} if key == "b256" else {False})


@pytest.mark.parametrize("key", K.DEVICE_KEYS)
def test_refusals_leave_the_context_usable(engine, key):
    b = kit(engine, key)[1]
    bad = b.refused_arguments()
    for xs, shares in bad:
        refused(engine, key, xs, shares)
        small_call_is_right(engine, key)
    refused(engine, key, *bad[0], space="device")
    small_call_is_right(engine, key)


def test_even_subgroup_order_is_refused(engine):
    """the documented limit of the call: (q-1)/2 must be odd"""
    grp = ModpGroup(K.Q_1_MOD_4)
    with pytest.raises(capi.EngineError, match="rc=-1"):
        engine.group_reconstruct(grp, [1, 2], (3).to_bytes(256, "big") + (5).to_bytes(256, "big"))
    small_call_is_right(engine, "b40")
