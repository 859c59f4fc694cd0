"""The secrets that tests/test_gpu_modp_rt_reconstruct_many.py gives to mpvss_modp_group_reconstruct_many, built over RtBuilder of
tests/modp_rt_reconstruct_cases.py (seeded polynomials, shares as powers of g = 4).  The GPU module compares every result with the
one-secret call on the same engine; tests/test_modp_rt_reconstruct_many_host.py holds the same cases to the oracle's
ref_reconstruct at 40 bits, so that the GPU expectations do not rest on the engine alone.

Sizes are the boundaries of k_rt_product_segments' fold over 16 quads: a lone factor, a partly filled wave, exactly one trip, one
factor into the second trip, the same at two trips, and five trips with one factor over (65); at 40 bits 16 and 17 trips too."""
from modp_rt_reconstruct_cases import Case

SEGMENT_M = [1, 2, 3, 15, 16, 17, 31, 32, 33, 65]
SEGMENT_M_B40 = [255, 256, 257]
WORKGROUP_COUNTS = [1, 2, 17, 64]
# under MPVSS_MAX_CHUNK = 32: [16, 16] is a pass cut exactly on 32, [3, 5] a pass that the single secret of 33 ends, [20, 7] a pass
# that 17 more shares would overfill, and [17] a trailing pass of one, which takes the one-secret path
CHUNK = 32
CHUNK_M = [16, 16, 3, 5, 33, 20, 7, 17]
CHUNK_STATS = {"passes": 3, "grouped_secrets": 6, "single_secrets": 2}


def segment_sizes(key):
    return SEGMENT_M + (SEGMENT_M_B40 if key == "b40" else [])


def segment_cases(b):
    """family A's shape cases at the fold's boundaries, ascending"""
    return [b.shape_case(m) for m in segment_sizes(b.name)]


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


def refused_between_good(b):
    """[(case, refused)]: good secrets of m = 3 with the refusals of the one-secret call between them.  A refused case may have
    shares None (a null pointer)."""
    good = small_cases(b, 7)
    three = b.shape_case(3)
    zero_neg = [c for c in b.sign_cases(5) if c.id.endswith("zero-neg")]
    assert len(zero_neg) == 1 and zero_neg[0].expect == ("refuse", None)
    bad = [Case("R-empty", [], [], ("refuse", None)),
           Case("R-null-shares", three.positions, None, ("refuse", None)),
           Case("R-position-0", [three.positions[0], 0, three.positions[2]], three.shares, ("refuse", None)),
           Case("R-duplicate", [three.positions[0], three.positions[1], three.positions[0]], three.shares, ("refuse", None)),
           zero_neg[0]]
    out = [(good[0], False)]
    for k, c in enumerate(bad):
        out += [(c, True), (good[k + 1], False)]
    out.append((good[6], False))
    return out


def tiny_refused_between_good(b, reference):
    """q = 23: [(case, refused)] of family C -- three sets the reference gives a value for, then alternately one whose reduced
    denominator has no inverse mod 11 and one more with a value.  reference(case) is the encoding or None."""
    value, none = [], []
    for c in b.tiny_cases():
        if len(c.positions) < 2:
            continue
        (none if reference(c) is None else value).append(c)
        if len(value) >= 6 and len(none) >= 3:
            break
    assert len(value) >= 6 and len(none) >= 3
    out = [(c, False) for c in value[:3]]
    for k in range(3):
        out += [(none[k], True), (value[3 + k], False)]
    return out


def chunk_cases(b):
    return [b.shape_case(m) for m in CHUNK_M]


def as_secret(case):
    """a case as group_reconstruct_many takes it"""
    return dict(positions=list(case.positions), shares=None if case.shares is None else b"".join(case.shares))
