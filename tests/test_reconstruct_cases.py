"""The builders and the reference of tests/reconstruct_cases.py against the oracle, so that tests/test_gpu_reconstruct_edges.py
cannot pass against a wrong expectation.  No GPU: the shares that the GPU module takes from the engine's fixed-base calls come
from the oracle here."""
import functools

import pytest

import mpvss_oracle as O
import reconstruct_cases as K

SECRET = 0x48656C6C6F204D50565353


@functools.lru_cache(maxsize=None)
def builder(name):
    return K.Builder(name)


def efix(G, e):
    return G.element_to_fixed(e)


@pytest.mark.parametrize("name", K.NAMES)
def test_reference_equals_oracle_on_a_dealt_box(name):
    G, pks, box, sbs = K.dealt_instance(name, 9, 4, 31, SECRET)
    pos_of = [box["positions"][G.element_to_bytes(p)] for p in pks]
    for subset in ([0, 1, 2, 3], [8, 6, 3, 1], [2, 4, 5, 7, 8]):
        chosen = [sbs[i] for i in subset]
        got = K.ref_reconstruct(G, [pos_of[i] for i in subset], [sb["share"] for sb in chosen])
        assert G.secret_mask(got) ^ box["U"] == O.reconstruct(G, chosen, box) == SECRET


def small_cases(name):
    b = builder(name)
    cases = [b.shape_case(m) for m in K.SHAPE_M[name] if m <= 9]
    if name != "modp2048":
        # (the oracle's MODP coefficient walks 1..max(positions), util.rs:47-64: positions near 2^63 are out of its reach; the
        # polynomial identity below holds them for MODP)
        cases.append(b.position_cases(17)["asc"])
    for m in K.SIGN_M:
        cases += b.sign_cases(m)
    return cases


@pytest.mark.parametrize("name", K.NAMES)
def test_reference_equals_oracle_on_synthetic_boxes(name):
    b = builder(name)
    G, memo = b.G, {}
    seen = set()
    for case in small_cases(name):
        sbs, box = K.synthetic_box(G, case)
        want = O.reconstruct(G, sbs, box)                                    # U = 0: the mask itself
        got = K.ref_reconstruct(G, case.positions, b.elements(case), memo)
        kind, v = case.expect
        seen.add(kind)
        if kind == "refuse":
            assert want is None and got is K.REFUSED, case.id
            continue
        assert got is not K.REFUSED and want == G.secret_mask(got), case.id
        assert efix(G, got) == b.expected(case, memo), case.id                # the identity or the builder's claim
        assert int.from_bytes(b.mask(efix(G, got)), "big") == want, case.id
        if case.id.endswith("swapped") and not case.id.endswith("unreduced-swapped"):
            m = len(case.positions)
            right = K.ref_reconstruct(G, case.positions, [G.element_from_fixed(s) for s in b.dealt(case.positions, 4, 5000 + m)[0]], memo)
            assert efix(G, got) != efix(G, right), case.id                    # a wrong value
    assert seen == ({"identity", "ref", "refuse"} if name == "modp2048" else {"identity", "ref"})


@pytest.mark.parametrize("name", K.NAMES)
def test_zero_shares_sit_on_the_lanes_their_cases_name(name):
    """MODP: a share of 0 or q on a positive lane gives G^s = 0, whose mask is that of the single byte 0x00"""
    if name != "modp2048":
        assert not any(c.expect[0] == "refuse" for m in K.SIGN_M for c in builder(name).sign_cases(m))
        return
    b = builder(name)
    assert b.mask(bytes(256)) == O.sha256(b"\x00")
    for m in K.SIGN_M:
        neg = K.lane_signs(b.sign_positions(m))
        for c in b.sign_cases(m):
            zero = [k for k, s in enumerate(c.shares) if int.from_bytes(s, "big") % b.G.q == 0]
            if c.expect[0] == "refuse":
                assert len(zero) == 1 and neg[zero[0]], c.id
            else:
                assert all(not neg[k] for k in zero), c.id
                assert (c.expect[1] == bytes(256)) == bool(zero), c.id


@pytest.mark.parametrize("name", K.NAMES)
def test_polynomial_identity_by_the_reference_alone(name):
    """G^P(0) = prod (G^P(x_i))^lambda_i at positions up to 2^63 - 1, for m >= t shares"""
    b = builder(name)
    G = b.G
    for m, t in zip([1, 2, 9, 17, 33], [1, 2, 4, 17, 5]):
        xs = K.orders(K.large_positions(m))["shuffled"]
        assert set(K.SPECIAL[:m]) <= set(xs) and max(xs) == 2 ** 63 - 1
        shares, s = b.dealt(xs, t, 7000 + m)
        got = K.ref_reconstruct(G, xs, [G.element_from_fixed(e) for e in shares])
        assert efix(G, got) == efix(G, G.exp(G.generator(), s)), (m, t)


def test_coefficients_of_every_gpu_position_list_sum_to_one():
    done = set()
    for name in K.NAMES:
        for xs in K.gpu_position_lists(name):
            key = tuple(sorted(xs))                                          # (the sum does not depend on the order)
            if key in done:
                continue
            done.add(key)
            assert sum(K.exact_lagrange(key)) == 1, (name, len(xs))
    assert {len(k) for k in done} >= set(K.SHAPE_M_BIG + K.POSITION_M + K.SIGN_M + K.DEVICE_M)


def test_sign_pattern_is_what_the_builder_claims():
    b = builder("secp256k1")
    lists = [b.sign_positions(m) for m in K.SIGN_M] + [b.shape_positions(257)]
    for m in K.POSITION_M:
        lists += list(K.orders(K.large_positions(m)).values())
    for xs in lists:
        assert K.lane_signs(xs) == [lam < 0 for lam in K.exact_lagrange(xs)]
    for m in K.SIGN_M:
        xs = b.sign_positions(m)
        assert xs != sorted(xs) and xs != sorted(xs, reverse=True)            # the sign count of unsorted positions
        lam = K.exact_lagrange(xs)
        pos_l, neg_l = b.sign_lanes(xs)
        assert len(pos_l) == 2 and len(neg_l) == 2
        assert all(lam[k] > 0 for k in pos_l) and all(lam[k] < 0 for k in neg_l)
    # m = 257: the five lanes of the identity see both signs
    neg = K.lane_signs(b.shape_positions(257))
    assert {neg[k] for k in K.LANES_257} == {True, False}
    with pytest.raises(ValueError):
        K.exact_lagrange([1, 2, 2, 3])
