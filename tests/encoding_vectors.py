"""Classified encodings of curve points for the decoder tests (CPU shim, GPU kernels, the oracle itself).

Every vector is `(label, bytes, expected)`; `expected` is None (the encoding must be rejected) or the oracle's point.
The vectors are built here by seeded searches, not copied from anywhere, and each one carries the exact set of decode
checks it fails, computed by the straight-line re-statement of the decode steps below (Python integers only, no oracle
code), so a vector's class is a fact about the vector.  A rejecting class holds vectors that fail exactly ONE check and
pass all the others -- a decoder that drops that check accepts them -- with the exceptions below; a class whose
name ends in `+other` or names two checks holds vectors that fail more than one, each with its exact set asserted:

  * ristretto255 has only 19 non-canonical values below 2^255 (p ... p + 18).  All 19 are present.  Three of them
    (p + 0, p + 4, p + 6) fail the canonical check alone under RFC 9496's reading (sign of the REDUCED value); the
    class `noncanonical` holds them.  A decoder that tests the sign on the RAW low bit (mpvss_rs_amd/csrc/ec_curves.h
    does: p is odd, so p + even is odd) rejects those three by its sign test as well; what only its canonical check
    rejects is p + s0 with s0 odd and -s0 a valid encoding (raw value even, reduced value negative).  These are the
    class `noncanonical+negative_s`; the remaining values of the 19 are `noncanonical+other`.
  * an encoding with bit 255 set is, read as a 256-bit integer, >= 2^255 > p: whether it "also" fails the canonical
    check depends on whether a decoder masks the bit first.  The re-statement masks it (as the RFC's printed vectors
    assume), so `bit255` vectors fail the bit test alone here.

  * `negative_s+other` (s = 1, p - 2, small odd s) and secp256k1 `noncanonical_x+other` (x = p: no point has x = 0) are the
    issue's named edge values that fail a second check too; they still go through every decoder.

The ristretto255 check names carry the RFC 9496 section 4.3.1 step they belong to.
"""
import random

import mpvss_oracle as O

# ---- ristretto255 -------------------------------------------------------------------------------------------------------------
P25519 = 2**255 - 19
_D = (-121665 * pow(121666, P25519 - 2, P25519)) % P25519
_SQRT_M1 = pow(2, (P25519 - 1) // 4, P25519)
assert _SQRT_M1 * _SQRT_M1 % P25519 == P25519 - 1

# RFC 9496 appendix A.1: multiples 0 ... 15 of the generator (tests/test_oracle_reference_kats.py pins the oracle to them)
RFC9496_GENERATOR_MULTIPLES = [
    "0000000000000000000000000000000000000000000000000000000000000000",
    "e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76",
    "6a493210f7499cd17fecb510ae0cea23a110e8d5b901f8acadd3095c73a3b919",
    "94741f5d5d52755ece4f23f044ee27d5d1ea1e2bd196b462166b16152a9d0259",
    "da80862773358b466ffadfe0b3293ab3d9fd53c5ea6c955358f568322daf6a57",
    "e882b131016b52c1d3337080187cf768423efccbb517bb495ab812c4160ff44e",
    "f64746d3c92b13050ed8d80236a7f0007c3b3f962f5ba793d19a601ebb1df403",
    "44f53520926ec81fbd5a387845beb7df85a96a24ece18738bdcfa6a7822a176d",
    "903293d8f2287ebe10e2374dc1a53e0bc887e592699f02d077d5263cdd55601c",
    "02622ace8f7303a31cafc63f8fc48fdc16e1c8c8d234b2f0d6685282a9076031",
    "20706fd788b2720a1ed2a5dad4952b01f413bcf0e7564de8cdc816689e2db95f",
    "bce83f8ba5dd2fa572864c24ba1810f9522bc6004afe95877ac73241cafdab42",
    "e4549ee16b9aa03099ca208c67adafcafa4c3f3e4e5303de6026e3ca8ff84460",
    "aa52e000df2e16f55fb1032fc33bc42742dad6bd5a8fc0be0167436c5948501f",
    "46376b80f409b29dc2b5f6f0c52591990896e5716f41477cd30085ab7f10301e",
    "e0c418f7c8d9c4cdd7395b93ea124f3ad99021bb681dfc3302a9d99a2e53e64e",
]

R_BIT255 = "step1:bit255"
R_CANON = "step1:noncanonical"
R_NEG_S = "step2:negative_s"
R_NONSQ = "step7:nonsquare"
R_NEG_XY = "step12:negative_xy"
R_Y_ZERO = "step12:y_zero"


def ristretto_checks(b):
    """(set of failed checks, which branch of SQRT_RATIO_M1 matched) for a 32-byte string: every step of RFC 9496 4.3.1
    evaluated, none short-circuited, on the value reduced mod p (bit 255 masked off first)."""
    assert len(b) == 32
    p = P25519
    raw = int.from_bytes(b, "little")
    failed = set()
    if raw >> 255:
        failed.add(R_BIT255)
    s = raw & ((1 << 255) - 1)
    if s >= p:
        failed.add(R_CANON)
    s %= p
    if s & 1:
        failed.add(R_NEG_S)
    ss = s * s % p
    u1 = (1 - ss) % p
    u2 = (1 + ss) % p
    u2_sqr = u2 * u2 % p
    v = (-(_D * u1 * u1) - u2_sqr) % p
    w = v * u2_sqr % p
    # SQRT_RATIO_M1(1, w), RFC 9496 4.2
    r = pow(w, 3, p) * pow(pow(w, 7, p), (p - 5) // 8, p) % p
    check = w * r * r % p
    branch = {1: "correct", p - 1: "flipped", (-_SQRT_M1) % p: "flipped_i"}.get(check, "none")
    if branch in ("flipped", "flipped_i"):
        r = r * _SQRT_M1 % p
    if r & 1:
        r = p - r
    if branch not in ("correct", "flipped"):
        failed.add(R_NONSQ)
    den_x = r * u2 % p
    den_y = r * den_x * v % p
    x = 2 * s * den_x % p
    if x & 1:
        x = p - x
    y = u1 * den_y % p
    t = x * y % p
    if t & 1:
        failed.add(R_NEG_XY)
    if y == 0:
        failed.add(R_Y_ZERO)
    return failed, branch


def _le(v):
    return v.to_bytes(32, "little")


def ristretto255_vectors(min_per_class=32, draws=4096):
    """{class: [(label, bytes, expected)]}.  Raises when a class comes up short."""
    G = O.Ristretto255Group()
    p = P25519
    rng = random.Random(0x9496)
    out = {k: [] for k in ("noncanonical", "noncanonical+negative_s", "noncanonical+other", "bit255", "negative_s", "negative_s+other",
                           "nonsquare", "negative_xy", "y_zero", "valid")}

    def reject(cls, label, b, want_failed):
        failed, branch = ristretto_checks(b)
        assert failed == set(want_failed), (cls, label, b.hex(), sorted(failed))
        assert G.bytes_to_element(b) is None, (cls, label, b.hex())
        out[cls].append((label, b, None))
        return branch

    def accept(label, b):
        failed, _ = ristretto_checks(b)
        assert not failed, (label, b.hex(), sorted(failed))
        pt = G.bytes_to_element(b)
        assert pt is not None and G.element_to_bytes(pt) == b, (label, b.hex())
        out["valid"].append((label, b, pt))

    # valid: identity, the RFC's multiples of the generator, random multiples
    for k, h in enumerate(RFC9496_GENERATOR_MULTIPLES):
        accept(f"valid:{k}*B", bytes.fromhex(h))
    for i in range(min_per_class):
        k = rng.randrange(1, G.l)
        accept(f"valid:random{i}", G.element_to_bytes(G.exp(G.generator(), k)))
    small_valid = [s0 for s0 in range(0, 64, 2) if not ristretto_checks(_le(s0))[0]]
    assert small_valid[:8] == [0, 4, 6, 20, 22, 30, 42, 46], small_valid
    for s0 in small_valid[1:]:
        accept(f"valid:s={s0}", _le(s0))
    valid_s = [int.from_bytes(b, "little") for _, b, _ in out["valid"] if any(b)]

    # step 1, canonical: all 19 values p ... p + 18 (bit 255 clear), each with the exact set it fails
    for s0 in range(19):
        b = _le(p + s0)
        failed, _ = ristretto_checks(b)
        assert R_CANON in failed and R_BIT255 not in failed
        cls = {frozenset([R_CANON]): "noncanonical", frozenset([R_CANON, R_NEG_S]): "noncanonical+negative_s"}.get(
            frozenset(failed), "noncanonical+other")
        reject(cls, f"{cls}:p+{s0}", b, failed)
    assert [l for l, _, _ in out["noncanonical"]] == ["noncanonical:p+0", "noncanonical:p+4", "noncanonical:p+6"]
    # step 1, bit 255: valid encodings with the top bit set (alias the valid point when the bit is masked, not checked)
    for s in [0] + valid_s[:min_per_class]:
        reject("bit255", f"bit255:{s:x}", _le(s | (1 << 255)), [R_BIT255])
    # step 2: odd canonical s.  1 fails y_zero too, so the lone-check vectors are the negations of valid encodings
    for s in valid_s[:min_per_class + 8]:
        reject("negative_s", f"negative_s:p-{s:x}", _le(p - s), [R_NEG_S])
    # odd canonical s that fail a later step as well (1: y = 0; p - 2 and most small odd values: not a square or x y negative)
    for s in [1, p - 2] + list(range(3, 40, 2)):
        failed, _ = ristretto_checks(_le(s))
        assert R_NEG_S in failed and R_CANON not in failed
        if len(failed) > 1:
            reject("negative_s+other", f"negative_s+other:{s:x}", _le(s), failed)
    assert {"negative_s+other:1", f"negative_s+other:{p - 2:x}"} <= {l for l, _, _ in out["negative_s+other"]}
    # steps 7 and 12: seeded draws of even canonical s
    n_i = n_none = 0
    for it in range(draws):
        s = rng.randrange(p) & ~1
        b = _le(s)
        failed, branch = ristretto_checks(b)
        if failed == {R_NONSQ}:
            if branch == "flipped_i" and n_i < min_per_class:
                n_i += 1
                reject("nonsquare", f"nonsquare:flipped_i:{it}", b, [R_NONSQ])
            elif branch == "none" and n_none < min_per_class:
                n_none += 1
                reject("nonsquare", f"nonsquare:no_flag:{it}", b, [R_NONSQ])
        elif failed == {R_NEG_XY} and len(out["negative_xy"]) < 2 * min_per_class:
            reject("negative_xy", f"negative_xy:{it}", b, [R_NEG_XY])
    assert n_i >= min_per_class // 2 and n_none >= min_per_class // 2, (n_i, n_none)
    # step 12, y = 0: u1 = 1 - s^2 = 0 <=> s = +-1; s = 1 is negative as well, s = p - 1 (even) is the only lone-check vector
    reject("y_zero", "y_zero:p-1", _le(p - 1), [R_Y_ZERO])
    assert ristretto_checks(_le(1))[0] == {R_NEG_S, R_Y_ZERO}

    need = {"noncanonical": 3, "noncanonical+negative_s": 2, "noncanonical+other": 14, "negative_s+other": 8, "bit255": min_per_class, "negative_s": min_per_class,
            "nonsquare": min_per_class, "negative_xy": min_per_class, "y_zero": 1, "valid": min_per_class}
    for cls, n in need.items():
        if len(out[cls]) < n:
            raise RuntimeError(f"ristretto255 class {cls}: {len(out[cls])} vectors, {n} wanted")
    assert sum(len(out[c]) for c in out if c.startswith("noncanonical")) == 19
    return out


# ---- secp256k1 ----------------------------------------------------------------------------------------------------------------
PSECP = 2**256 - 2**32 - 977
S_PREFIX = "prefix"
S_CANON = "noncanonical_x"
S_CURVE = "not_on_curve"


def secp_checks(b):
    """set of failed SEC1 compressed-point checks for a 33-byte string that is not all zero (secp256k1.rs:138-152)"""
    assert len(b) == 33 and any(b)
    p = PSECP
    failed = set()
    if b[0] not in (2, 3):
        failed.add(S_PREFIX)
    x = int.from_bytes(b[1:], "big")
    if x >= p:
        failed.add(S_CANON)
    y2 = (pow(x % p, 3, p) + 7) % p
    if pow(y2, (p - 1) // 2, p) != 1:         # y2 = 0 would need x^3 = -7; -7 is no cube mod p (checked below)
        failed.add(S_CURVE)
    return failed


def _sec1(prefix, x):
    return bytes([prefix]) + x.to_bytes(32, "big")


def secp256k1_vectors(min_per_class=32, draws=4096):
    G = O.Secp256k1Group()
    p = PSECP
    rng = random.Random(0x5EC1)
    out = {k: [] for k in ("prefix", "noncanonical_x", "noncanonical_x+other", "not_on_curve", "valid")}
    assert pow(7, (p - 1) // 2, p) == p - 1, "7 is a non-residue: no point has x = 0"
    assert pow(p - 7, (p - 1) // 3, p) != 1, "-7 is no cube: no point has y = 0"

    def on_curve(x):
        return pow((pow(x, 3, p) + 7) % p, (p - 1) // 2, p) == 1

    def reject(cls, label, b, want_failed):
        failed = secp_checks(b)
        assert failed == set(want_failed), (cls, label, b.hex(), sorted(failed))
        assert G.bytes_to_element(b) is None, (cls, label, b.hex())
        out[cls].append((label, b, None))

    def accept(label, b):
        if any(b):
            assert not secp_checks(b), (label, b.hex())
        ok, pt = G.decode_element(b)
        assert ok and G.element_to_bytes(pt) == b, (label, b.hex())
        out["valid"].append((label, b, pt))

    accept("valid:identity", bytes(33))
    accept("valid:G", G.element_to_bytes(G.generator()))
    xs = []
    for _ in range(draws):
        x = rng.randrange(p)
        if on_curve(x):
            xs.append(x)
            if len(xs) == min_per_class:
                break
    small = [x for x in range(1, 14) if on_curve(x)]
    assert small == [1, 2, 3, 4, 6, 8, 12, 13], small
    near_p = next(p - k for k in range(1, 64) if on_curve(p - k))
    for x in xs + [small[0], near_p]:
        accept(f"valid:02:{x:x}", _sec1(2, x))
        accept(f"valid:03:{x:x}", _sec1(3, x))

    for pre in (0x00, 0x01, 0x04, 0x05, 0x06, 0x07, 0x82, 0x83, 0xfe, 0xff):
        for x in (xs[0], small[0]):
            reject("prefix", f"prefix:{pre:02x}:{x:x}", _sec1(pre, x), [S_PREFIX])
    for pre in (2, 3):
        reject("not_on_curve", f"not_on_curve:{pre:02x}:x=0", _sec1(pre, 0), [S_CURVE])
    for x0 in small:
        for pre in (2, 3):
            reject("noncanonical_x", f"noncanonical_x:{pre:02x}:p+{x0}", _sec1(pre, p + x0), [S_CANON])
    for x in (p, 2**256 - 1):
        b = _sec1(2, x)
        failed = secp_checks(b)
        assert S_CANON in failed
        reject("noncanonical_x" if failed == {S_CANON} else "noncanonical_x+other", f"noncanonical_x:02:{x:x}", b, failed)
    edge = next(p - k for k in range(1, 64) if not on_curve(p - k))
    assert edge in (p - 1, p - 2)
    off = [edge]
    for _ in range(draws):
        x = rng.randrange(p)
        if not on_curve(x):
            off.append(x)
            if len(off) == min_per_class + 1:
                break
    for i, x in enumerate(off):
        reject("not_on_curve", f"not_on_curve:{2 + (i & 1):02x}:{x:x}", _sec1(2 + (i & 1), x), [S_CURVE])

    need = {"prefix": 16, "noncanonical_x": 16, "noncanonical_x+other": 1, "not_on_curve": min_per_class, "valid": 2 * min_per_class + 4}
    for cls, n in need.items():
        if len(out[cls]) < n:
            raise RuntimeError(f"secp256k1 class {cls}: {len(out[cls])} vectors, {n} wanted")
    return out


_CACHE = {}


def vectors(name):
    """{class: [(label, bytes, expected)]} for "secp256k1" or "ristretto255" (built once per process)"""
    if name not in _CACHE:
        _CACHE[name] = {"secp256k1": secp256k1_vectors, "ristretto255": ristretto255_vectors}[name]()
    return _CACHE[name]


def rejecting(name):
    """every vector that must be rejected, all classes, as [(label, bytes)]"""
    return [(l, b) for cls, vs in vectors(name).items() if cls != "valid" for l, b, _ in vs]


def valid(name):
    return list(vectors(name)["valid"])


def representatives(name):
    """one rejecting vector per class: [(class, bytes)]"""
    return [(cls, vs[0][1]) for cls, vs in vectors(name).items() if cls != "valid" and vs]
