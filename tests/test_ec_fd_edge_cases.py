"""The case builder of tests/ec_fd_edge_child.py, checked with the oracle alone (no GPU): the cases that
tests/test_gpu_ec_fd_edges.py sends through the forward-difference kernels must BE the degenerate ones they are named after -- a
builder that drifted into ordinary polynomials would leave that module green and empty."""
import pytest

import ec_fd_edge_child as K
import mpvss_oracle as O

T, N = K.DEFAULT


def by_id(curve):
    return {c.id: c for c in K.build_cases(curve)}


_CM = {}


def commitments(curve, case):
    """C_j = a_j G by the oracle, once per case"""
    key = (curve, case.id)
    if key not in _CM:
        G = O.GROUPS[curve]()
        _CM[key] = [G.generate_public_key(a) if a else G.identity() for a in case.coeffs]
    return _CM[key]


def enc_x(curve, case, index):
    G = O.GROUPS[curve]()
    return G.element_to_bytes(O.commitment_eval(G, commitments(curve, case), case.positions[index]))


def identity(curve):
    G = O.GROUPS[curve]()
    return G.element_to_bytes(G.identity())


@pytest.mark.parametrize("curve", K.CURVES)
def test_the_set_of_cases(curve):
    cases = K.build_cases(curve)
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)) == 32
    shapes = {(c.t, c.n) for c in cases}
    assert shapes == {(16, 4096), (17, 4099), (33, 4099), (256, 4096), (15, 4096), (16, 4095), (257, 4112)}
    assert [c.family for c in cases if (c.t, c.n) == (256, 4096)] == ["roots-a"]          # one family at the largest t
    assert all(len(c.coeffs) == c.t and len(c.positions) == c.n and len(c.spots()) <= 24 for c in cases)
    assert set(K.BOX_CASES + K.MANY) <= set(ids)
    assert K.CONFIGS == {"horner": {"MPVSS_EC_FD": "0"},
                         "quad": {"MPVSS_EC_FD": "1", "MPVSS_EC_FD_QUAD": "2", "MPVSS_EC_FD_L1": "0"},
                         "quad-l1": {"MPVSS_EC_FD": "1", "MPVSS_EC_FD_QUAD": "2", "MPVSS_EC_FD_L1": "2"},
                         "chain-l1": {"MPVSS_EC_FD": "1", "MPVSS_EC_FD_QUAD": "0", "MPVSS_EC_FD_L1": "2"}}


@pytest.mark.parametrize("curve", K.CURVES)
def test_each_family_is_what_it_claims(curve):
    G = O.GROUPS[curve]()
    order = G.group_order_int()
    ident = identity(curve)
    c = by_id(curve)
    assert all(0 < a < order for a in c["f1-control"].coeffs)
    a = c["f2-zero-a7"].coeffs
    assert a[7] == 0 and all(x for j, x in enumerate(a) if j != 7)
    assert G.element_to_bytes(commitments(curve, c["f2-zero-a7"])[7]) == ident
    a = c["f3-top1"].coeffs
    assert a[-1] == 0 and all(a[:-1])
    a = c["f3-linear"].coeffs
    assert a[0] and a[1] and a[2:] == [0] * (T - 2)
    a = c["f3-constant"].coeffs
    assert a[0] and a[1:] == [0] * (T - 1)
    assert enc_x(curve, c["f3-constant"], 1234) == G.element_to_bytes(commitments(curve, c["f3-constant"])[0])
    assert c["f4-all-zero"].coeffs == [0] * T and enc_x(curve, c["f4-all-zero"], 77) == ident
    a = c["f7-alternating"].coeffs
    assert a[0] and all((a[j] + a[j + 1]) % order == 0 for j in range(T - 1))
    cm = commitments(curve, c["f7-alternating"])
    assert all(G.element_to_bytes(G.mul(cm[j], cm[j + 1])) == ident for j in range(T - 1))
    assert G.element_to_bytes(cm[0]) != ident
    a = c["f8-equal"].coeffs
    assert a[0] and a == [a[0]] * T
    for tt in (17, 33):
        assert c[f"t{tt}-linear"].coeffs[2:] == [0] * (tt - 2) and all(c[f"t{tt}-control"].coeffs)


@pytest.mark.parametrize("curve", K.CURVES)
def test_the_roots_of_family_5_are_the_identity_and_lie_where_they_are_meant_to(curve):
    ident = identity(curve)
    c = by_id(curve)
    for cid, variant in (("f5-roots-a", "a"), ("f5-roots-b", "b")):
        case = c[cid]
        roots = K.root_indices(N, T, variant)
        assert case.named == roots and len(set(roots)) == 4
        assert case.coeffs[-1] != 0 and len(case.coeffs) == T                   # degree t - 1: R has degree t - 5
        for i in roots:
            assert enc_x(curve, case, i) == ident, (cid, i)
        for i in (1, roots[2] + 1, roots[3] - 1):                               # and their neighbours are not
            assert enc_x(curve, case, i) != ident, (cid, i)
    # where the mirror of ec_fd_geometry puts them, at every shape the family runs at
    for t, n in ((16, 4096), (17, 4099), (33, 4099), (256, 4096)):
        S, chain_len, w0 = K.fd_geometry(n, t)
        assert S >= 4 and S * chain_len >= n > S * (chain_len - 1) and 0 < w0 and w0 + t < chain_len
        for variant in "ab":
            first, last, seed, stepped = K.root_indices(n, t, variant)
            assert (first, last) == (0, n - 1) and 0 < stepped < n - 1
            assert w0 <= seed // S < w0 + t                                     # a seed of its chain
            w1 = (S * t - t) // 2                                               # the two-level seeding's Horner seeds: w1 .. w1 + t - 1
            assert (w1 <= seed - S * w0 < w1 + t) == (variant == "b")
            j = stepped // S
            assert (j >= w0 + t) if variant == "a" else (j < w0)                # forward / backward of the seeds
    assert K.fd_geometry(4096, 16) == (64, 64, 24) and K.fd_geometry(4096, 256) == (4, 1024, 384)
    assert K.fd_geometry(65536, 256) == (16, 4096, 1920) and K.fd_geometry(4099, 33) == (31, 133, 50)


@pytest.mark.parametrize("curve", K.CURVES)
def test_linear_family_has_second_differences_equal_to_the_identity(curve):
    G = O.GROUPS[curve]()
    case = by_id(curve)["f3-linear"]
    cm = commitments(curve, case)
    x = [O.commitment_eval(G, cm, case.positions[i]) for i in (100, 101, 102)]
    d1 = G.mul(x[1], G.element_inverse(x[0]))
    d2 = G.mul(x[2], G.element_inverse(x[1]))
    assert G.element_to_bytes(d1) == G.element_to_bytes(d2) == G.element_to_bytes(cm[1])      # first differences: C_1
    assert G.element_to_bytes(G.mul(d2, G.element_inverse(d1))) == identity(curve)            # second differences: the identity


@pytest.mark.parametrize("curve", K.CURVES)
def test_family_6_is_the_identity_at_position_0(curve):
    case = by_id(curve)["f6-a0-zero-p0"]
    assert case.p0 == 0 and case.positions[0] == 0 and case.coeffs[0] == 0 and all(case.coeffs[1:]) and case.path == "fd"
    assert enc_x(curve, case, 0) == identity(curve) and enc_x(curve, case, 1) != identity(curve)


def admitted(positions):
    """positions_consecutive (mpvss_capi.cpp) on int64 values: consecutive from a start in [0, 2^61)"""
    return 0 <= positions[0] < (1 << 61) and all(p == positions[0] + i for i, p in enumerate(positions))


def test_expected_paths_follow_from_the_rules():
    """the expected-path column of the first positions and of the shape-rule edges"""
    table = {"0": "fd", "1": "fd", "2^32-n/2": "fd", "2^61-1": "fd", "2^61": "horner", "-5": "horner"}
    first = {"0": 0, "1": 1, "2^32-n/2": 2**32 - N // 2, "2^61-1": 2**61 - 1, "2^61": 2**61, "-5": -5}
    c = by_id("secp256k1")
    seen = set()
    for case in c.values():
        assert all(-2**63 <= p < 2**63 for p in (case.positions[0], case.positions[-1]))       # they enter as int64
        rule = 16 <= case.t <= 256 and case.n >= 16 * case.t and case.n >= 4096 and admitted(case.positions)
        assert case.path == ("fd" if rule else "horner"), case.id
        if case.id.startswith("p0="):
            label, space = case.id[3:].rsplit("-", 1)
            assert case.p0 == first[label] and case.path == table[label] and space in ("host", "device") and case.family == "control"
            assert (case.t, case.n) == (T, N) and case.coeffs == c["f1-control"].coeffs
            seen.add((label, space))
        elif case.id.startswith("shape-"):
            assert case.path == "horner" and not K.fd_shape(case.t, case.n)
        else:
            assert case.path == "fd", case.id
    assert seen | {("1", "host")} == {(l, s) for l in table for s in ("host", "device")}
    assert (c["f1-control"].p0, c["f1-control"].space) == (1, "host")
    cross = c["p0=2^32-n/2-host"]
    assert cross.positions[N // 2 - 1] == 2**32 - 1 and cross.positions[N // 2] == 2**32          # the run crosses 2^32
    neg = c["p0=-5-host"]
    assert neg.positions[4] == -1 and neg.positions[5] == 0 and K.scalar_of_position(-1) == 2**64 - 1
    assert [(case.t, case.n) for case in c.values() if case.id.startswith("shape-")] == [(15, 4096), (16, 4095), (257, 4112)]
    assert K.fd_shape(16, 4096) and K.fd_shape(256, 4096) and not K.fd_shape(256, 4095) and not K.fd_shape(17, 4095)
