"""Child process of tests/test_gpu_ec_fd_edges.py: the switches that choose how the curve groups compute X_i for consecutive
positions (MPVSS_EC_FD, MPVSS_EC_FD_QUAD, MPVSS_EC_FD_L1) are read once per process, so one child runs every case of ONE
configuration, both curves, and prints one line per case:

    case <curve> <case id> <sha256 of the X bytes> fd=<blocks counted>,<fall-backs counted>

    python ec_fd_edge_child.py horner | quad | quad-l1 | chain-l1

The cases are polynomials whose X_i = P(i) G meets the identity -- the value the group law treats specially -- in the difference
tables (fd_table_body, fd_quad_table_body), in the stepping recurrence (fd_step_body, fd_quad_step_body, the two-level seeding chain)
and in Secp::encode_batch; first positions at the edges of the admissibility rule 0 <= p0 < 2^61 (positions_consecutive,
k_modp_fd_check_positions); shapes at the edges of ec_fd_shape.  The dealer's coefficients a_j are known here, so every X_i of every
case is compared with P(i mod 2^64) mod order (Python integers) times G through the fixed-base comb (mpvss_ec_batch_exp_generator,
another kernel, pinned to the oracle by tests/test_gpu_ec.py), byte for byte; the `horner` and `quad` children also compare up to
24 positions per case with O.commitment_eval in the reference's order (participant.rs:423-434, `position as u64`
participant.rs:1419 / 1862).

What the counter proves: mpvss_modp_fd_stats counts verifiers' blocks only.  Where the quad-lane pipelines run (`quad`, `quad-l1`) a
box has a gate, a pipeline that gives up leaves every X to the gated Horner launch, and for a case that exists only as
mpvss_ec_commit_eval (all-zero, roots-b, a0-zero, the first positions, t = 17, 33 and 256) no counter tells which of the two wrote
the bytes: their hashes in those two children are no proof of the forward-difference path -- the whole boxes and ec_verify_many
calls, whose counter is asserted, are.  The `chain-l1` child has no gate for host positions: there forward differences computed them.

build_cases() needs neither torch nor a GPU: tests/test_ec_fd_edge_cases.py checks with the oracle alone that the cases are the
degenerate ones they claim to be."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mpvss_oracle as O  # noqa: E402

# (torch and the engine are imported by main only: the spawned oracle workers re-import this module)

CONFIGS = {
    "horner": {"MPVSS_EC_FD": "0"},
    "quad": {"MPVSS_EC_FD": "1", "MPVSS_EC_FD_QUAD": "2", "MPVSS_EC_FD_L1": "0"},
    "quad-l1": {"MPVSS_EC_FD": "1", "MPVSS_EC_FD_QUAD": "2", "MPVSS_EC_FD_L1": "2"},
    "chain-l1": {"MPVSS_EC_FD": "1", "MPVSS_EC_FD_QUAD": "0", "MPVSS_EC_FD_L1": "2"},
}
CURVES = ("secp256k1", "ristretto255")
P0_LIMIT = 1 << 61                 # positions_consecutive / k_modp_fd_check_positions admit 0 <= p0 < 2^61
DEFAULT = (16, 4096)               # the smallest shape ec_fd_shape admits
BOX_CASES = ("f2-zero-a7", "f3-linear", "f5-roots-a", "f7-alternating")      # also dealt and verified as whole boxes
MANY = ("f1-control", "f5-roots-a", "f3-linear", "f1-control")               # the four boxes of one ec_verify_many call


def fd_geometry(n, t):
    """mirror of ec_fd_geometry (mpvss_rs_amd/csrc/capi_ec.inc): S strided chains -- member j of chain c is run index c + S j --
    of chain_len members, the t seeds of a chain are its members w0 .. w0 + t - 1.  It only steers where family 5 puts its roots."""
    S = max(1, min(max(4096 // t, 4), n // (4 * t)))
    chain_len = -(-n // S)
    return S, chain_len, (chain_len - t) // 2


def fd_shape(t, n):
    """ec_fd_shape (capi_ec.inc) without its MPVSS_EC_FD switch"""
    return 16 <= t <= 256 and n >= 16 * t and n >= 4096


def expected_path(t, n, p0):
    """'fd' when the rule sends a run of n consecutive positions from p0 through forward differences, else 'horner'"""
    return "fd" if fd_shape(t, n) and 0 <= p0 < P0_LIMIT else "horner"


def root_indices(n, t, variant):
    """run indices at which family 5 makes X the identity: the run's first and last member, one seed, one member reached by stepping.
    variant a: a seed in the first quarter of the seed window (the two-level seeding reaches it by its stride-1 chain), a member reached by
    stepping FORWARD; variant b: one of the t seeds the two-level seeding evaluates by Horner's rule, a member reached by stepping
    BACKWARD.  (The first member is the last backward step of chain 0, the last member the last forward step of its chain.)"""
    S, chain_len, w0 = fd_geometry(n, t)
    if variant == "a":
        seed = S // 2 + S * (w0 + t // 4)
        stepped = min(5, S - 1) + S * (w0 + t + (chain_len - w0 - t) // 2)
    else:
        seed = S * w0 + (S * t - t) // 2 + 3
        stepped = max(S - 2, 0) + S * (w0 // 2)
    return [0, n - 1, seed, stepped]


def poly_mul(a, b, order):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % order
    return out


def poly_eval(coeffs, x, order):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % order
    return acc


def scalar_of_position(p):
    return p & 0xFFFFFFFFFFFFFFFF      # Scalar::from(position as u64)


class Case:
    def __init__(self, cid, family, t, n, p0, coeffs, named=(), space="host"):
        self.id, self.family, self.t, self.n, self.p0, self.coeffs, self.space = cid, family, t, n, p0, coeffs, space
        self.named = list(named)       # run indices the family is about (oracle spot checks)
        self.path = expected_path(t, n, p0)
        self.positions = list(range(p0, p0 + n))

    def spots(self):
        """at most 24 run indices for the oracle"""
        t, n = self.t, self.n
        s = []
        for i in [0, 1, t, n // 2 - 1, n // 2, n - 2, n - 1] + self.named:
            if 0 <= i < n and i not in s:
                s.append(i)
        assert len(s) <= 24
        return s


def family_coeffs(family, t, n, p0, order, rng):
    """the t coefficients a_0 .. a_{t-1} of a family and the run indices it is about"""
    rnd = lambda: rng.randrange(1, order)
    a = [rnd() for _ in range(t)]
    if family == "control":
        return a, []
    if family == "zero-a7":
        a[7] = 0
        return a, []
    if family == "top1":
        a[t - 1] = 0
        return a, []
    if family == "linear":
        return a[:2] + [0] * (t - 2), []
    if family == "constant":
        return a[:1] + [0] * (t - 1), []
    if family == "all-zero":
        return [0] * t, []
    if family in ("roots-a", "roots-b"):
        idx = root_indices(n, t, family[-1])
        p = [rnd() for _ in range(t - 4)]                  # R of degree t - 5, leading coefficient not zero
        for i in idx:
            p = poly_mul(p, [(-scalar_of_position(p0 + i)) % order, 1], order)
        assert len(p) == t
        return p, idx
    if family == "a0-zero":
        a[0] = 0
        return a, [0]
    if family == "alternating":
        return [a[0] if j % 2 == 0 else order - a[0] for j in range(t)], []
    if family == "equal":
        return [a[0]] * t, []
    raise KeyError(family)


def build_cases(curve):
    """every case of one curve, the same in every configuration"""
    order = O.GROUPS[curve]().group_order_int()
    cases = []

    def add(cid, family, t, n, p0, space="host", named=()):
        rng = random.Random(f"{curve}/{family}/{t}/{n}")      # (one polynomial per family and shape, whatever the first position)
        coeffs, idx = family_coeffs(family, t, n, p0, order, rng)
        cases.append(Case(cid, family, t, n, p0, coeffs, list(idx) + list(named), space))

    t, n = DEFAULT
    add("f1-control", "control", t, n, 1)
    add("f2-zero-a7", "zero-a7", t, n, 1)
    add("f3-top1", "top1", t, n, 1)
    add("f3-linear", "linear", t, n, 1)
    add("f3-constant", "constant", t, n, 1)
    add("f4-all-zero", "all-zero", t, n, 1)
    add("f5-roots-a", "roots-a", t, n, 1)
    add("f5-roots-b", "roots-b", t, n, 1)
    add("f6-a0-zero-p0", "a0-zero", t, n, 0)
    add("f7-alternating", "alternating", t, n, 1)
    add("f8-equal", "equal", t, n, 1)
    for tt in (17, 33):                # ragged chains, ONE level in the top stage of the 16-level quad pipeline
        for fam in ("control", "roots-a", "linear"):
            add(f"t{tt}-{fam}", fam, tt, 4099, 1)
    add("t256-roots-a", "roots-a", 256, 4096, 1)            # the largest t at the smallest n: S = 4 chains of 1024 members
    # first positions, family 1, host and device-resident positions ("f1-control" is p0 = 1 with host positions)
    for label, p0, named in (("0", 0, [0]), ("1", 1, []), ("2^32-n/2", (1 << 32) - n // 2, []), ("2^61-1", P0_LIMIT - 1, []),
                             ("2^61", P0_LIMIT, []), ("-5", -5, [4, 5, 6])):
        for space in ("host", "device"):
            if (label, space) != ("1", "host"):
                add(f"p0={label}-{space}", "control", t, n, p0, space, named)
    # the edges of ec_fd_shape: Horner's rule by the shape alone
    for tt, nn in ((15, 4096), (16, 4095), (257, 4112)):
        add(f"shape-{tt}x{nn}", "control", tt, nn, 1)
    assert len({c.id for c in cases}) == len(cases)
    return cases


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------
def run(config):
    import ctypes as C

    import torch

    from helpers import ec_reference_x, parallel_map
    from mpvss_rs_amd import Engine, capi

    for k, v in CONFIGS[config].items():
        assert os.environ.get(k) == v, f"{k} must be {v} for the {config} child"
    with_oracle = config in ("horner", "quad")
    quad = CONFIGS[config].get("MPVSS_EC_FD_QUAD") == "2"      # then every X path by forward differences has a gate, and is counted
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    oracle_items, oracle_want = [], []

    for curve in CURVES:
        G = O.GROUPS[curve]()
        gid = capi.GROUP_SECP256K1 if curve == "secp256k1" else capi.GROUP_RISTRETTO255
        order, L = G.group_order_int(), G.elem_len
        ident = G.element_to_bytes(G.identity())
        sc = lambda vals: b"".join(G.scalar_to_bytes(v) for v in vals)
        cases = build_cases(curve)
        done = {}

        def commit_eval(case, cm):
            if case.space == "host":
                return eng.ec_commit_eval(gid, cm, case.positions)
            # device-resident positions: nobody on the host looks at them, k_modp_fd_check_positions decides
            d_cm = torch.frombuffer(bytearray(cm), dtype=torch.uint8).to(dev)
            d_pos = torch.tensor(case.positions, dtype=torch.int64, device=dev)
            d_out = torch.zeros(case.n * L, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()          # torch's copies run on torch's stream, the engine's kernels on the engine's
            rc = eng.lib.mpvss_ec_commit_eval(eng.ctx, gid, capi.MPVSS_DEVICE, C.c_void_p(d_cm.data_ptr()), case.t,
                                              C.c_void_p(d_pos.data_ptr()), case.n, C.c_void_p(d_out.data_ptr()))
            eng._check(rc, "ec_commit_eval(device)")
            eng.lib.mpvss_ctx_synchronize(eng.ctx)
            return bytes(d_out.cpu().numpy().tobytes())

        for case in cases:
            t, n = case.t, case.n
            cm = eng.ec_batch_exp_generator(gid, sc(case.coeffs))
            for j, a in enumerate(case.coeffs):             # a zero coefficient is the identity's encoding
                if a == 0:
                    assert cm[j * L:(j + 1) * L] == ident, (curve, case.id, j)
            values = [poly_eval(case.coeffs, scalar_of_position(p), order) for p in case.positions]
            want = eng.ec_batch_exp_generator(gid, sc(values))
            for i in case.named:
                if case.family.startswith("roots") or case.family in ("a0-zero", "all-zero"):
                    assert values[i] == 0 and want[i * L:(i + 1) * L] == ident, (curve, case.id, i)
            before = eng.fd_stats()
            if case.family == "all-zero":
                assert want == ident * n
            got = commit_eval(case, cm)
            after = eng.fd_stats()
            assert after == before, "mpvss_ec_commit_eval is no verifier's block: it counts nothing"
            if got != want:
                bad = [i for i in range(n) if got[i * L:(i + 1) * L] != want[i * L:(i + 1) * L]]
                S, chain_len, w0 = fd_geometry(n, t)
                raise AssertionError(f"{config} {curve} {case.id} (t = {t}, n = {n}, p0 = {case.p0}, {case.space} positions): "
                                     f"{len(bad)} of {n} X differ from P(i) G, first at run indices {bad[:12]} "
                                     f"(S = {S}, chain_len = {chain_len}, w0 = {w0})")
            if with_oracle and t != 256:        # (256, 4096): Python integers and the comb cover it
                for i in case.spots():
                    oracle_items.append((curve, cm, case.positions[i]))
                    oracle_want.append(((curve, case.id, i), got[i * L:(i + 1) * L]))
            done[case.id] = (case, cm, got)
            print("case", curve, case.id, hashlib.sha256(got).hexdigest(), "fd=0,0", flush=True)

        # ---- whole boxes of shape (16, 4096): ec_deal with the family's coefficients, then the verifier with a dump
        t, n = DEFAULT
        rng = random.Random(f"{curve}/boxes")
        pk = eng.ec_batch_exp_generator(gid, sc([rng.randrange(1, order) for _ in range(n)]))
        wit = sc([rng.randrange(1, order) for _ in range(n)])
        boxes, single = {}, {}
        for cid in sorted(set(BOX_CASES) | set(MANY)):
            case, cm, x = done[cid]
            assert (case.t, case.n, case.space, case.path) == (t, n, "host", "fd")
            box = eng.ec_deal(gid, sc(case.coeffs), case.positions, pk, wit)
            assert box["X"] == x, f"{curve} {cid}: the dealer's X (P(i) G through the comb)"
            before = eng.fd_stats()
            res = eng.ec_verify_distribution(gid, cm, case.positions, pk, box["Y"], box["responses"], box["challenge"], dump=True)
            after = eng.fd_stats()
            delta = (after[0] - before[0], after[1] - before[1])
            assert res["verdict"] is True, f"{config} {curve} {cid}: the verifier rejects the dealer's own box"
            assert res["digest"] == box["digest"], f"{config} {curve} {cid}: transcript digest"
            assert res["X"] == x, f"{config} {curve} {cid}: the verifier's X differ from mpvss_ec_commit_eval's"
            assert res["a1"] == box["a1"] and res["a2"] == box["a2"], f"{config} {curve} {cid}: a1 / a2"
            # the counter is the only evidence that the pipelines computed these bytes and did not leave them to the gated Horner launch
            assert delta == ((1, 0) if quad else (0, 0)), f"{config} {curve} {cid}: fd_stats moved by {delta}"
            boxes[cid] = dict(commitments=cm, positions=case.positions, pubkeys=pk, shares=box["Y"], responses=box["responses"],
                              challenge=box["challenge"])
            single[cid] = (res["verdict"], res["digest"])
            print("case", curve, "box-" + cid, hashlib.sha256(res["X"] + res["a1"] + res["a2"] + res["digest"]).hexdigest(),
                  f"fd={delta[0]},{delta[1]}", flush=True)

        # ---- four boxes in one ec_verify_many call: their X paths by the same launches, the box as the second grid dimension
        if config in ("quad", "chain-l1"):
            lsb = 31 if curve == "secp256k1" else 0          # (the low byte of a response: the scalar stays canonical)
            r = boxes["f5-roots-a"]["responses"]
            k = 5 * 32 + lsb
            bad = dict(boxes["f5-roots-a"], responses=r[:k] + bytes([r[k] ^ 1]) + r[k + 1:])
            res = eng.ec_verify_distribution(gid, bad["commitments"], bad["positions"], bad["pubkeys"], bad["shares"], bad["responses"],
                                             bad["challenge"])
            assert res["verdict"] is False
            single["tampered"] = (res["verdict"], res["digest"])
            for what, seq, ids in (("many", [boxes[c] for c in MANY], list(MANY)),
                                   ("many-tampered", [boxes[MANY[0]], bad, boxes[MANY[2]], boxes[MANY[3]]],
                                    [MANY[0], "tampered", MANY[2], MANY[3]])):
                before = eng.fd_stats()
                out = eng.ec_verify_many(gid, seq, depth=4)
                after = eng.fd_stats()
                delta = (after[0] - before[0], after[1] - before[1])
                assert out == [single[c] for c in ids], f"{config} {curve} {what}: not what one box at a time gives"
                assert delta == ((4, 0) if quad else (0, 0)), f"{config} {curve} {what}: fd_stats moved by {delta}"
                print("case", curve, what, hashlib.sha256(b"".join(bytes([v]) + d for v, d in out)).hexdigest(),
                      f"fd={delta[0]},{delta[1]}", flush=True)

    eng.close()
    if with_oracle:       # the reference's own order of operations, on freshly spawned oracle-only workers
        outs = parallel_map(ec_reference_x, oracle_items)
        for (tag, got), want in zip(oracle_want, outs):
            assert got == want, f"{config} {tag}: not what O.commitment_eval gives"
        print("oracle positions", len(outs), flush=True)
    print(f"ec fd edges {config} ok", flush=True)


if __name__ == "__main__":
    import torch  # noqa: F401  (torch's HIP runtime first, as tests/conftest.py)
    run(sys.argv[1])
