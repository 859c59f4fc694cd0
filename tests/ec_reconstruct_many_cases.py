"""The secrets that tests/test_gpu_ec_reconstruct_many.py gives to mpvss_ec_reconstruct_many, built over Builder of
tests/reconstruct_cases.py (seeded polynomials, shares as multiples of the generator).  The GPU module compares every result with
the one-secret call on the same engine and with the builder's closed form; tests/test_ec_reconstruct_many_cases.py holds the same
cases to the oracle's ref_reconstruct, so that the GPU expectations do not rest on the engine alone.

Sizes are the boundaries of k_*_sum_segments, one wave per secret: a lone factor, the starts of its tree at 2 and 4 lanes, a wave
short of one lane, exactly full, one factor into the second trip of the stride loop, the same at two trips, and four trips with
one factor over (257)."""
import encoding_vectors as EV
from reconstruct_cases import CURVES, LANES_257, Case  # noqa: F401

SEGMENT_M = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
# 9 and 513 cross the eight-points-per-lane and the 512-per-block edges of k_secp_encode_batch; 513 workgroups are more than the
# chip has compute units
SECRET_COUNTS = [1, 2, 9, 65, 513]
# under MPVSS_MAX_CHUNK = 32: [16, 16] is a pass cut exactly on 32, [3, 5] a pass that the single secret of 33 ends, [20, 7] a pass
# that 17 more shares would overfill, and [17] a trailing pass of one, which takes the one-secret path
CHUNK = 32
CHUNK_M = [16, 16, 3, 5, 33, 20, 7, 17]
CHUNK_STATS = {"passes": 3, "grouped_secrets": 6, "single_secrets": 2}


def segment_cases(b):
    """family A's shape cases at the sum's boundaries, ascending: neighbours differ in size"""
    return [b.shape_case(m) for m in SEGMENT_M]


def small_cases(b, count):
    """`count` secrets of m = 3 from seeded polynomials over twelve different position lists"""
    out = []
    for k in range(count):
        xs = [10, 1 + k % 4, 6 + k % 3]
        shares, s = b.dealt(xs, 3, 7000 + k)
        out.append(Case(f"W-{k}", xs, shares, ("identity", s)))
    return out


def sharing_cases(b):
    """eight secrets over one position list, then the first of them with positions and shares permuted alike -- another list with
    the same result -- and one over another list of the same length"""
    xs = [5, 2, 9, 4]
    out = []
    for k in range(8):
        shares, s = b.dealt(xs, 3, 7500 + k)
        out.append(Case(f"S-same-{k}", xs, shares, ("identity", s)))
    perm = [2, 0, 3, 1]
    out.append(Case("S-permuted", [xs[i] for i in perm], [out[0].shares[i] for i in perm], out[0].expect))
    ys = [5, 2, 9, 7]
    shares, s = b.dealt(ys, 3, 7600)
    out.append(Case("S-other", ys, shares, ("identity", s)))
    return out


def rejected_encoding(name):
    """one encoding that the curve's decoder rejects (the first of tests/encoding_vectors.py's rejecting vectors)"""
    return EV.rejecting(name)[0][1]


def refused_between_good(b):
    """[(case, refused)]: good secrets of m = 3 with the refusals of the one-secret call between them.  A refused case may have
    shares None (a null pointer).  The last refusal has a rejected encoding as the middle share of a secret."""
    good = small_cases(b, 7)
    three = b.shape_case(3)
    bad_enc = rejected_encoding(b.name)
    assert len(bad_enc) == len(three.shares[1])
    bad = [Case("R-empty", [], [], ("refuse", None)),
           Case("R-null-shares", three.positions, None, ("refuse", None)),
           Case("R-position-0", [three.positions[0], 0, three.positions[2]], three.shares, ("refuse", None)),
           Case("R-duplicate", [three.positions[0], three.positions[1], three.positions[0]], three.shares, ("refuse", None)),
           Case("R-encoding", three.positions, [three.shares[0], bad_enc, three.shares[2]], ("refuse", None))]
    out = [(good[0], False)]
    for k, c in enumerate(bad):
        out += [(c, True), (good[k + 1], False)]
    out.append((good[6], False))
    return out


def sign_and_degenerate_cases(b):
    """family C at m = 5 and m = 17: the identity, equal and opposite shares on lanes of either sign"""
    return b.sign_cases(5) + b.sign_cases(17)


def lane_cases(b):
    """m = 257 with the identity on the first and last lane of the wave, and on the first lanes of later trips"""
    return [b.lane_case_257(lane) for lane in LANES_257]


def identity_lane_expected(b, m, lane):
    """the closed form of shape_case(m) with the identity in place of share `lane`: the other factors add up to
    (P(0) - lambda_lane P(x_lane)) G -- one exponentiation, no fold"""
    from reconstruct_cases import T_SHAPE, exact_lagrange
    xs = b.shape_positions(m)
    coeffs = b.poly(min(T_SHAPE, m), 2000 + m)
    lam = exact_lagrange(xs)[lane]
    lam = lam.numerator * pow(lam.denominator, -1, b.ring) % b.ring
    e = (coeffs[0] - lam * b.values(coeffs, [xs[lane]])[0]) % b.ring
    return b.G.element_to_fixed(b.G.exp(b.G.generator(), e))


def chunk_cases(b):
    return [b.shape_case(m) for m in CHUNK_M]


def as_secret(case):
    """a case as ec_reconstruct_many takes it"""
    return dict(positions=list(case.positions), shares=None if case.shares is None else b"".join(case.shares))
