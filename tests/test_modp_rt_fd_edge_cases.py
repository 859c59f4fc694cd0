"""The cases of tests/modp_rt_fd_edge_child.py against the integer model of tests/test_modp_rt_fd_model.py, without a GPU: the
builder claims "fd" only for what the host gate admits, its mirror of the chain geometry is the model's, the planted roots are
roots and sit where the placement says, every case small enough goes through the model of the kernel (table, both directions,
stepping) at all positions, the model's mutants are caught by families B and C -- and not by the all-ones polynomial of family
A, which is why A alone would not do -- and the positions at which the child evaluates Python integers cover what the issue of
the sampling condition demands."""
import pytest

import modp_rt_fd_edge_child as K
import test_modp_rt_fd_model as M
from test_modp_rt_fd_model import admissible, chain_bounds, fd_eval, reference


def x_cases(width):
    return [c for c in K.build_cases(width) if c.kind == "x"]


def small(c):
    return c.mod.bits <= K.ALL_BITS and c.n * c.t <= K.ALL_NT


@pytest.mark.parametrize("width", K.WIDTHS)
def test_every_width_has_the_cases_it_is_owed(width):
    cases = K.build_cases(width)
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    lpl = int(width)
    tmax = K.FD_MAX_T[lpl]
    big = [m for m in K.moduli(width) if not m.tiny]
    assert all(m.lpl == lpl and H_width(m) == lpl for m in K.moduli(width))
    # the largest workgroup on every modulus of the width, and one past it
    for m in big:
        c = next(c for c in cases if c.id == f"C-tmax-{m.name}")
        assert (c.t, c.n, c.chains, c.path) == (tmax, 4 * tmax + 3, 3, "fd")
    over = next(c for c in cases if c.id == "C-tmax+1")
    assert over.t == tmax + 1 and over.path == "horner" and over.n >= over.t
    # family A: every kind at t = 5 and t = 33 on every modulus with room for it, the non-unit on the composite ones
    kinds = {"mid-one", "top-one", "constant", "linear", "all-one", "all-minus-one", "mid-minus-one", "all-equal", "alternating",
             "plus-kq", "top-value"}
    for m in big:
        for t in (5, 33):
            have = {c.id.rsplit("-p1-", 1)[1]: c for c in cases if c.id.startswith(f"A-{m.name}-t{t}-p1-")}
            assert set(have) == kinds | ({"non-unit"} if not m.safe else set())
            assert all((c.n, c.chains) == (4 * t + 3, 3) for c in have.values())
            assert all(c.path == "fd" for k, c in have.items() if k not in ("non-unit", "top-value"))
            if not m.safe:
                c = have["non-unit"]
                assert c.path == "horner" and 1 < K.math.gcd(c.given[1], m.q) < m.q
            c = have["plus-kq"]
            assert c.given[1] % m.q == c.C[1] and c.given[1] <= m.top < c.given[1] + m.q
            assert have["top-value"].given[1] == m.top
            assert have["top-value"].path == ("fd" if K.math.gcd(m.top % m.q, m.q) == 1 else "horner")
    if width in ("18", "27"):       # q = 2^k - 1 is the largest EB-byte value itself: that commitment is 0 mod q
        assert next(c for c in cases if c.id.endswith("t33-p1-top-value") and "ones" in c.id).path == "horner"
    # family B on the safe primes, C's shapes, D's first positions
    for m in big:
        if m.safe and m.name != "p64":
            assert {f"B-{m.name}-t{t}-place{p}" for t in (9, 37) for p in (1, 2)} <= set(ids)
    want_t = {"5": K.SHAPE_T, "9": (16, 17, 128, 129, 241, 256), "18": (16, 17, 128, 129, 241, 256), "27": (16, 17, 127, 128)}[width]
    assert {c.t for c in cases if c.family == "C" and c.path == "fd" and (c.n, c.chains) == (4 * c.t + 3, 3)} == set(want_t)
    t = 17
    for name, shape in (("no-steps", (t, 3 * t, 3)), ("one-direction", (t, 3 * t + 1, 3)), ("ragged", (t, 3 * t + 2, 3)),
                        ("2t-1", (t, 2 * t - 1, 1)), ("long-chain", (3, 4099, 1)), ("64-chains", (2, 4099, 64)),
                        ("clamped", (t, 4099, 1000))):
        c = next(c for c in cases if c.id == f"C-{name}")
        assert (c.t, c.n, c.chains) == shape and c.path == "fd"
    d = [c for c in cases if c.family == "D" and c.mod in big and (c.t, c.n) == (5, 40) and c.mod.bits > 64]
    assert {(c.p0, c.space) for c in d} == {(p, s) for p in (0, 1, 2 ** 32 - 20, 2 ** 62, 2 ** 63 - 40) for s in ("host", "device")}
    if width == "5":
        assert {c.id for c in cases if c.family == "D" and c.mod.name in ("q23", "p40")} == {
            f"D-{m}-{k}" for m in ("q23", "p40") for k in ("ends-q-2", "ends-q-1", "p0=-5-host", "p0=-5-device")}
        assert {c.space for c in cases if c.id.startswith("D-p64-p0=2^63-n")} == {"host", "device"}
    assert bool([c for c in cases if c.family == "E"]) == (width in ("18", "27"))
    assert bool([c for c in cases if c.family == "F"]) == (width in ("5", "18"))


def H_width(m):
    """limbs per lane the library picks for this modulus (modp_rt_helpers.width_for_bits; 27 for a wide handle)"""
    return 27 if m.eb != 256 else K.H.width_for_bits(m.bits)


def test_the_moduli_sit_on_the_limb_count_boundaries():
    bits = {w: [m.bits for m in K.moduli(w)] for w in K.WIDTHS}
    assert bits == {"5": [3, 5, 40, 64, 256, 578], "9": [579, 1024, 1042], "18": [1043, 2048, 2048], "27": [2049, 3072, 3072]}
    for w, name, k in (("18", "ones2048", 2048), ("27", "ones3072", 3072)):
        q = K.modulus(w, name).q
        assert q % 4 == 3 and 0 < 2 ** k - q and all((2 ** k - c) % 4 != 3 for c in range(1, 2 ** k - q))
    assert all(m.factor and m.q % m.factor == 0 for w in K.WIDTHS for m in K.moduli(w) if not m.safe)
    assert all(K.H.miller_rabin(m.q, rounds=4) and K.H.miller_rabin((m.q - 1) // 2, rounds=4)
               for w in K.WIDTHS for m in K.moduli(w) if m.safe and m.bits <= 1024)


@pytest.mark.parametrize("width", K.WIDTHS)
def test_the_expected_path_is_the_host_gates(width):
    tmax = K.FD_MAX_T[int(width)]
    for c in K.build_cases(width):
        given = c.given if c.kind == "x" else [4] * c.t          # (a box's commitments are powers of 4 mod a prime: units)
        ok = admissible(c.q, given, c.positions, K.FD_MAX_T[c.mod.lpl], 0, 2)
        # (a negative first position is refused by the entry point before the gate: the gate would say Horner)
        assert ("fd" if ok else "invalid" if c.p0 < 0 else "horner") == c.path, c.id
        assert not admissible(c.q, given, c.positions, tmax, 0, 0)


def test_chain_geometry_mirror_and_the_seed_rule():
    for n, t, chains in ((39, 9, 3), (151, 37, 3), (51, 17, 3), (52, 17, 3), (53, 17, 3), (33, 17, 1), (4099, 3, 1), (4099, 2, 64),
                         (4099, 17, 1000), (1027, 256, 3), (40, 5, 0), (64, 7, 0), (64, 64, 0), (21, 21, 3), (65536, 256, 0)):
        g = K.fd_geometry(n, t, chains)
        S = len(g)
        assert S == K.fd_chains(n, t, chains) and 1 <= S <= n // t
        for c, (first, length, seed0) in enumerate(g):
            assert (first, length) == chain_bounds(n, S, c) == K.fd_chain(n, S, c)
            assert length >= t and seed0 == first + (length - t) // 2 and first <= seed0 and seed0 + t <= first + length
    assert K.fd_chains(4099, 17, 1000) == 4099 // 17 and K.fd_chains(65536, 256, 0) == 32 and K.fd_chains(40, 5, 0) == 2
    # the shapes family C names: no steps at all, one direction without steps, ragged chains with len - t odd in some and even in others
    assert all(l == 17 for _, l, _ in K.fd_geometry(51, 17, 3))
    assert sorted(l - 17 for _, l, _ in K.fd_geometry(52, 17, 3)) == [0, 0, 1]
    assert sorted((l - 17) % 2 for _, l, _ in K.fd_geometry(4099, 17, 1000)) != [0] * 241
    assert {l - 2 for _, l, _ in K.fd_geometry(4099, 2, 64)} == {62, 63}
    assert K.fd_geometry(4099, 3, 1) == [(0, 4099, 2048)]


def family_b():
    return [c for w in K.WIDTHS for c in K.build_cases(w) if c.family == "B"]


@pytest.mark.parametrize("case", family_b(), ids=lambda c: c.id)
def test_planted_roots_are_roots_and_sit_where_the_placement_says(case):
    c = case
    g = K.fd_geometry(c.n, c.t, c.chains)
    assert len(g) == 3 and len(set(c.roots)) == 4
    first, length, seed0 = g[1]
    if c.id.endswith("place1"):
        assert c.roots == [first, first + length - 1, seed0, seed0 + c.t - 1]
        assert first < seed0 and seed0 + c.t - 1 < first + length - 1          # the chain's edges are reached by stepping
    else:
        assert c.roots == [seed0 - 1, seed0 + c.t, g[2][0], g[0][2] + c.t]
        assert first < seed0 - 1 and seed0 + c.t < first + length - 1 and g[0][2] + c.t < g[0][0] + g[0][1]
    near = sorted({i + d for i in c.roots for d in (-1, 1)} - set(c.roots))[:2]
    vals = reference(c.C, c.q, [c.p0 + i for i in c.roots + near])
    assert vals[:4] == [1] * 4
    assert all(v != 1 for v in vals[4:])
    assert set(c.roots) <= set(c.at)
    assert c.C[-1] != 1 and c.path == "fd"                                     # degree t - 1 exactly


@pytest.mark.parametrize("width", K.WIDTHS)
def test_small_cases_through_the_model_of_the_kernel_at_all_positions(width):
    """fd_eval, both forms of its table, against Python integers at all positions.  The integers are the child's ref_x (Horner's
    rule in the exponent) and the model's reference (prod_j C_j^(i^j) with pow); the latter costs a second per case at t = 33
    above 256 bits (exponents of 230 bits), so there it is taken at the positions the sampling rule names and ref_x, which it
    equals everywhere else, at all of them."""
    ran = 0
    for c in x_cases(width):
        if not small(c):
            continue
        assert c.at == list(range(c.n)), c.id
        if c.path != "fd":
            continue
        want = [K.ref_x(c.C, c.q, p) for p in c.positions]
        S = K.fd_chains(c.n, c.t, c.chains)
        assert fd_eval(c.C, c.q, c.p0, c.n, S)[0] == want, c.id
        assert fd_eval(c.C, c.q, c.p0, c.n, S, in_place=True)[0] == want, c.id
        idx = K.sample_indices(c.n, c.t, c.chains) if c.t > 17 and c.mod.bits > 256 else range(c.n)
        assert reference(c.C, c.q, [c.positions[i] for i in idx]) == [want[i] for i in idx], c.id
        ran += 1
    assert ran > (100 if width == "5" else 20 if width == "9" else -1)


def test_ref_x_is_the_reference_where_positions_are_reduced_or_a_commitment_is_no_unit():
    q = 23
    C = [5, 7, 11, 2, 3]
    for i in (0, 1, 21, 22, 23, 100, -5, -1):
        ip = (i % 2 ** 64) % (q - 1)
        want = 1
        for j, c in enumerate(C):
            want = want * pow(c, ip ** j % (q - 1), q) % q
        assert K.ref_x(C, q, i) == want
        assert K.ref_x(C[:2] + [0] + C[3:], q, i) == (0 if ip else 5)
    q = 1015 * 1019
    assert K.ref_x([2, 5, 3], q, 7) == 2 * 5 ** 7 * 3 ** 49 % q               # i^j < q - 1: nothing is reduced


def wrong_order_table(G0, H0, q):
    """a mutant of table_in_place: a level overwrites G and H quad by quad, so quad k reads its neighbour's NEW numbers -- the
    kernel without the barrier between forming a level and storing it"""
    t = len(G0)
    G, H = list(G0), list(H0)
    for l in range(1, t):
        for k in range(l, t):
            G[k], H[k] = G[k] * H[k - 1] % q, H[k] * G[k - 1] % q
    return G


def mutants(c):
    """which of the model's mutants this case tells from the kernel's rule"""
    S = K.fd_chains(c.n, c.t, c.chains)
    want = [K.ref_x(c.C, c.q, p) for p in c.positions]
    run = lambda **kw: fd_eval(c.C, c.q, c.p0, c.n, S, **kw)[0]
    assert run() == want
    caught = set()
    for name, kw in (("swap_at=1", dict(swap_at=1)), ("swap_at=t-1", dict(swap_at=c.t - 1)), ("wrong_parity", dict(wrong_parity=True)),
                     ("stale=False", dict(stale=False))):
        if run(**kw) != want:
            caught.add(name)
    keep = M.table_in_place
    M.table_in_place = wrong_order_table
    try:
        if run(in_place=True) != want:
            caught.add("wrong order in place")
    finally:
        M.table_in_place = keep
    return caught


ALL_MUTANTS = {"swap_at=1", "swap_at=t-1", "wrong_parity", "stale=False", "wrong order in place"}


def test_mutants_are_caught_by_families_b_and_c_and_not_by_the_all_ones_polynomial():
    cases = [c for c in x_cases("5") if small(c) and c.path == "fd"]
    by = {}
    for c in cases:
        if c.family == "B" or (c.family == "C" and 3 <= c.t <= 17):
            for m in mutants(c):
                by.setdefault(m, []).append(c.id)
    assert set(by) == ALL_MUTANTS
    assert all(any(i.startswith("B-") for i in ids) and any(i.startswith("C-") for i in ids) for ids in by.values())
    # family A: where every commitment is one, every number of every table is one and no mutant shows.  A constant X (only C_0 is
    # not one) makes every level above 0 one: it tells nothing about the roles of E and F in a table step or about the stepping,
    # and shows only the two mistakes that reach level 0 -- the backward state from the other diagonal, which holds X^-1 there
    # instead of X, and a level 1 that reads an already overwritten neighbour
    for c in cases:
        if c.family == "A" and c.t >= 3 and c.mod.name == "p256":
            if c.id.endswith("all-one"):
                assert mutants(c) == set(), c.id
            if c.id.endswith("constant"):
                assert mutants(c) == {"wrong_parity", "wrong order in place"}, c.id
    assert sum(c.family == "A" and c.id.endswith(("all-one", "constant")) and c.mod.name == "p256" for c in cases) == 4


@pytest.mark.parametrize("width", K.WIDTHS)
def test_the_sampling_condition_holds(width):
    sampled = 0
    for c in K.build_cases(width):
        assert c.at == sorted(set(c.at)) and all(0 <= i < c.n for i in c.at), c.id
        if small(c):
            assert c.at == list(range(c.n)), c.id
            continue
        sampled += 1
        need = set(c.roots)
        if c.n >= c.t:
            S = K.fd_chains(c.n, c.t, c.chains)
            for k in range(S):
                first, length = chain_bounds(c.n, S, k)
                seed0 = first + (length - c.t) // 2
                need |= {first, first + length - 1, seed0, seed0 + c.t - 1}
                need |= {i for i in (seed0 - 1, seed0 + c.t) if 0 <= i < c.n}
        assert need <= set(c.at), c.id
    assert sampled or width == "5"


def test_the_chunks_child_expects_what_the_chunk_loop_gives():
    """group_verify_distribution cuts n into chunks of MPVSS_MAX_CHUNK; a chunk takes forward differences when t <= min(n, chunk)
    (rt_fd_prepare) and cnt >= t (rt_commit_eval_dev).  group_commit_eval is one pass under the same rt_fd_prepare."""
    for (n, t), paths in zip(K.CHUNK_CASES, K.CHUNK_PATHS):
        ready = 2 <= t <= min(n, K.CHUNK)
        chunks = [min(K.CHUNK, n - off) for off in range(0, n, K.CHUNK)]
        fd = sum(ready and cnt >= t for cnt in chunks)
        assert paths["verify"] == f"fd={fd},horner={len(chunks) - fd}"
        assert paths["commit_eval"] == ("fd=1,horner=0" if ready and n >= t else "fd=0,horner=1")
    assert K.CHUNK_CASES == ((133, 7), (128, 64), (130, 65))
    assert [p["verify"] for p in K.CHUNK_PATHS] == ["fd=2,horner=1", "fd=2,horner=0", "fd=0,horner=3"]
    assert set(K.expected("chunks")) == {f"chunks-n{n}-t{t}-{w}" for n, t in K.CHUNK_CASES for w in ("commit_eval", "verify")}
