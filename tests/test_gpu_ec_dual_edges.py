"""The curve groups' windowed double-scalar kernel (dual_win_body / dual_win_glv_body) on the GPU at its scalar, base and
lane edges: every configuration (comb, one table, comb + table, two tables) and every table source (encodings per share
or shared, internal points, a table kept from an earlier call), byte for byte against the plain-C reference
(oracle/ec_ref.c, plain double-and-add).  The cases and what they claim: tests/ec_dual_cases.py, held to it by
tests/test_ec_dual_cases.py."""
import hashlib
import random

import pytest

import ec_dual_cases as D
import mpvss_oracle as O
from mpvss_rs_amd import capi

pytestmark = pytest.mark.gpu
GID = {"secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}


@pytest.fixture(scope="module", params=D.NAMES)
def cs(request):
    return D.cases(request.param)


def split(b, n):
    return [b[i:i + n] for i in range(0, len(b), n)]


def compare(cs, what, config, tags, got, want):
    """byte for byte; a mismatch names the row, its class or bases and the configuration"""
    got = split(got, len(want[0])) if want else []
    assert len(got) == len(want), "%s %s: %d results for %d rows" % (cs.name, config, len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    for i in bad[:8]:
        print("%s %s: %s of row %d (%s): got %s, expected %s" % (cs.name, config, what, i, tags[i], got[i].hex(), want[i].hex()))
    assert not bad, "%s %s: %s differs in %d of %d rows, first row %d (%s)" % (cs.name, config, what, len(bad), len(want), bad[0],
                                                                                 tags[bad[0]])


def dleq(engine, cs, rows, path, c_per_share, config):
    g1 = cs.gen if path == "G" else cs.p0
    c = D.scalars(cs, rows, "c") if c_per_share else cs.scalar(rows[0].c)
    assert c_per_share or len({row.c for row in rows}) == 1
    a1, a2 = engine.ec_dleq_commitments(GID[cs.name], g1, D.cat(rows, "h1"), D.cat(rows, "g2"), D.cat(rows, "h2"),
                                        D.scalars(cs, rows, "r"), c, c_per_share)
    want = [cs.expected(row, path) for row in rows]
    tags = [row.tag for row in rows]
    config = "%s, g1 = %s, %s challenge" % (config, "G (comb + table)" if path == "G" else "a point (table + table)",
                                            "per-share" if c_per_share else "shared")
    compare(cs, "a1", config, tags, a1, [w[0] for w in want])
    compare(cs, "a2", config, tags, a2, [w[1] for w in want])


@pytest.mark.parametrize("path", ["G", "P"])
def test_dleq_commitments_grids_with_per_share_challenges(engine, cs, path):
    """digit grid, class grid (secp256k1) and base grid, one call per grid"""
    for gname, rows in cs.grids():
        if rows:
            dleq(engine, cs, rows, path, True, gname)


@pytest.mark.parametrize("path", ["G", "P"])
def test_dleq_commitments_base_grid_with_a_shared_challenge(engine, cs, path):
    """the base grid once per distinct challenge it holds (k2_stride = 0)"""
    distinct = sorted({row.c for row in cs.base_grid})
    assert len(distinct) == 4
    for c in distinct:
        rows = [row for row in cs.base_grid if row.c == c]
        dleq(engine, cs, rows, path, False, "base grid with c = %#x" % c)


@pytest.mark.parametrize("path", ["G", "P"])
@pytest.mark.parametrize("c_per_share", [True, False])
def test_dleq_commitments_at_the_lane_and_workgroup_edges(engine, cs, path, c_per_share):
    for n in D.SHAPES:
        dleq(engine, cs, cs.lane_rows(n, shared=not c_per_share), path, c_per_share, "lane pool, n = %d" % n)


def test_one_scalar_configurations_at_the_lane_and_workgroup_edges(engine, cs):
    """k * P from a per-share table and k * G from the comb alone, bases and scalars from the pool"""
    gid = GID[cs.name]
    for n in D.SHAPES:
        rows = cs.lane_rows(n)
        tags = [row.tag for row in rows]
        out = engine.ec_batch_exp(gid, D.cat(rows, "g1"), D.scalars(cs, rows, "r"))
        compare(cs, "k * P", "ec_batch_exp (table), n = %d" % n, tags, out, [cs.mul(row.g1, row.r) for row in rows])
        out = engine.ec_batch_exp_generator(gid, D.scalars(cs, rows, "r"))
        compare(cs, "k * G", "ec_batch_exp_generator (comb), n = %d" % n, tags, out, [cs.mul(cs.gen, row.r) for row in rows])


def extract_expected(cs, rows):
    """rows (tag, pk, Y, xinv, w) -> S = xinv Y, a1 = w G, a2 = w S and the challenge over the oracle's framing"""
    G = cs.G
    e = G.element_from_fixed
    S, cb = [], []
    for _, pk, Y, xinv, w in rows:
        s = cs.mul(Y, xinv)
        a1, a2 = cs.mul(cs.gen, w), cs.mul(s, w)
        digest = hashlib.sha256(O.append_transcript(G, e(pk), e(Y), e(a1), e(a2))).digest()
        S.append(s)
        cb.append(cs.scalar(G.hash_to_scalar(digest)))
    return S, cb


def run_extract(engine, cs, rows, config):
    gid = GID[cs.name]
    S, c = engine.ec_extract_shares(gid, b"".join(r[1] for r in rows), b"".join(r[2] for r in rows),
                                    b"".join(cs.scalar(r[3]) for r in rows), b"".join(cs.scalar(r[4]) for r in rows))
    want_S, want_c = extract_expected(cs, rows)
    tags = [r[0] for r in rows]
    compare(cs, "S", config, tags, S, want_S)
    compare(cs, "challenge", config, tags, c, want_c)
    return S, c


def test_extract_shares_at_the_lane_and_workgroup_edges(engine, cs):
    """a2 = w * S from a table built from internal points (the third call), pool rows as (pk, Y, xinv, w)"""
    for n in D.EXTRACT_SHAPES:
        rows = [(row.tag, row.h1, row.g2, row.r, row.c) for row in cs.lane_rows(n)]
        run_extract(engine, cs, rows, "ec_extract_shares, lane pool, n = %d" % n)


def test_extract_shares_edge_rows_and_their_proofs(engine, cs):
    """Y = I, 1/x = 0, 1, n - 1, w = 0, 1, n - 1, Y = G, -G and (secp256k1) top-digit classes of w and 1/x; the honest rows
    (pk = x G, the scalar 1/x) are closed into proofs that ec_verify_shares accepts, and refuses after one flipped bit
    of r, as the oracle does"""
    G, gid, n = cs.G, GID[cs.name], cs.order
    rng = random.Random(0xE7 + gid)
    rnd = lambda: rng.randrange(2, n)
    inv = lambda x: pow(x, -1, n)
    honest = []                                                   # (tag, x, Y, w)
    honest.append(("Y = I", rnd(), cs.ident, rnd()))
    honest.append(("1/x = 1", 1, cs.point(), rnd()))
    honest.append(("1/x = n - 1", n - 1, cs.point(), rnd()))
    for w in (0, 1, n - 1):
        honest.append(("w = %s" % {0: "0", 1: "1"}.get(w, "n - 1"), rnd(), cs.point(), w))
    honest.append(("Y = G", rnd(), cs.gen, rnd()))
    honest.append(("Y = -G", rnd(), cs.neg(cs.gen), rnd()))
    top = [(cl, k) for cl, k in cs.classes if cl[2] or cl[3]]
    assert cs.name != "secp256k1" or len(top) >= 3
    for (ca, ka), (cb, kb) in zip(top[:3], top[1:4] if len(top) > 3 else top[:3]):
        honest.append(("w of class %r, 1/x of class %r" % (ca, cb), inv(kb), cs.point(), ka))
    rows = [(tag, cs.mul(cs.gen, x), Y, inv(x), w) for tag, x, Y, w in honest]
    rows.insert(1, ("1/x = 0 with Y != I", cs.point(), cs.point(), 0, rnd()))
    S, c = run_extract(engine, cs, rows, "ec_extract_shares, edge rows")
    assert split(S, cs.L)[0] == cs.ident and split(S, cs.L)[1] == cs.ident
    keep = [i for i in range(len(rows)) if i != 1]
    pk, Sb, Y = (b"".join(col[i] for i in keep) for col in ([r[1] for r in rows], split(S, cs.L), [r[2] for r in rows]))
    cb = [split(c, 32)[i] for i in keep]
    ci = [G.scalar_from_fixed(x) for x in cb]
    r = [O.dleq_response(G, w, x, cc) % n for (_, x, _, w), cc in zip(honest, ci)]
    good = b"".join(cs.scalar(x) for x in r)
    assert list(engine.ec_verify_shares(gid, pk, Sb, Y, b"".join(cb), good)) == [1] * len(keep)
    flipped = [x ^ 1 if (x ^ 1) < n else x ^ 2 for x in r]
    assert list(engine.ec_verify_shares(gid, pk, Sb, Y, b"".join(cb), b"".join(cs.scalar(x) for x in flipped))) == [0] * len(keep)
    e = G.element_from_fixed
    for k, i in enumerate(keep):
        args = (G, G.generator(), e(rows[i][1]), e(split(S, cs.L)[i]), e(rows[i][2]), ci[k])
        assert O.dleq_verify(*args, r[k]) is True, rows[i][0]
        assert O.dleq_verify(*args, flipped[k]) is False, rows[i][0]


def test_distribute_reuses_the_table_of_y(engine, cs):
    """t = 1 (X_i = C_0 at any position): Y = p * y builds the table, a2 = w * y reuses it; p = 0, p = n - 1, w = 0, y = I,
    y = G one by one (n = 1) and at the head of n = 257 rows of the pool"""
    G, gid, n = cs.G, GID[cs.name], cs.order
    e = G.element_from_fixed
    cm = cs.pool[7].g2
    pr = cs.pool[:5]
    edges = [("p = 0", pr[0].h1, 0, pr[0].c), ("p = n - 1", pr[1].h1, n - 1, pr[1].c), ("w = 0", pr[2].h1, pr[2].r, 0),
             ("y = I", cs.ident, pr[3].r, pr[3].c), ("y = G", cs.gen, pr[4].r, pr[4].c)]
    pool = [(row.tag, row.h1, row.r, row.c) for row in cs.lane_rows(257)]
    calls = [[row] for row in edges] + [[pool[1]], edges + pool[len(edges):]]
    for rows in calls:
        m = len(rows)
        positions = list(range(1, m + 1))
        positions[0], positions[-1] = (1 << 40) + 3, 0
        config = "ec_distribute, t = 1, n = %d" % m
        d = engine.ec_distribute(gid, cm, positions, b"".join(r[1] for r in rows), b"".join(cs.scalar(r[2]) for r in rows),
                                 b"".join(cs.scalar(r[3]) for r in rows))
        tags = [r[0] for r in rows]
        want = [(cm, cs.mul(y, p), cs.mul(cs.gen, w), cs.mul(y, w)) for _, y, p, w in rows]
        for k, what in enumerate(("X", "Y", "a1", "a2")):
            compare(cs, what, config, tags, d[what], [x[k] for x in want])
        h = hashlib.sha256()
        for x in want:
            h.update(O.append_transcript(G, *(e(v) for v in x)))
        assert d["digest"] == h.digest(), config
