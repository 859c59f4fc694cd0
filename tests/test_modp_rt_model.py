"""CPU checks of the run-time MODP group: an integer model of bn::mont_mul (mpvss_rs_amd/csrc/bn_quad.h, the widths of bn_quad_rt.h) at each
instantiated width with a run-time n0inv -- same step order, same lazy carries, same two-pass normalisation -- that proves
the column bound for worst-case almost-normalised limbs; the long product that brings a 2048-bit input into a narrower width;
and the host side of the C ABI (group creation, width choice, hash_to_scalar against the oracle)."""
import hashlib
import random

import pytest

import mpvss_oracle as O
import modp_rt_helpers as H
from mpvss_rs_amd import capi

W = 29
M = (1 << W) - 1
LIMB_BOUND = M + 512
WIDTHS = (5, 9, 18)


def limbs(v, n):
    return [(v >> (W * j)) & M for j in range(n)]


def val(l):
    return sum(x << (W * j) for j, x in enumerate(l))


def in_rows(lpl):
    return lpl * ((72 + lpl - 1) // lpl)


def mont_model(a, b, N, lpl, rows, stats, square=False, bound_only=False):
    """bn::mont_mul<N0INV_RUNTIME, square, rows / lpl> as integers: a has L = 4 lpl limbs, b has `rows` limbs; returns the L result limbs
    (bound_only: operands far above 2N as integers, only the accumulator bound is checked)"""
    L = 4 * lpl
    NL = limbs(N, L)
    n0inv = (-pow(N, -1, 1 << W)) % (1 << W)
    T = [0] * L
    for i in range(rows):
        bi = b[i]
        rr = i % lpl
        for j in range(L):
            k = j % lpl
            if not square:
                T[j] += a[j] * bi
            elif k >= rr:
                T[j] += a[j] * (2 * bi if k > rr else bi)
        m = ((T[0] & 0xFFFFFFFF) * n0inv) & M        # (u32)T[rr] * n0inv, masked: the run-time multiply of the kernel
        for j in range(L):
            T[j] += m * NL[j]
        assert T[0] & M == 0
        stats["maxacc"] = max(stats["maxacc"], max(T))
        for q in range(4):
            j = q * lpl
            T[j + 1] += T[j] >> W
            T[j] &= M
        assert max(T) < (1 << 64)
        T = T[1:] + [0]
    if bound_only:
        return None
    out, couts = [0] * L, [0] * 4
    for q in range(4):
        c = 0
        for k in range(lpl):
            v = T[q * lpl + k] + c
            assert v < (1 << 64)
            out[q * lpl + k] = v & M
            c = v >> W
        couts[q] = c
    assert couts[3] == 0
    for q in range(1, 4):
        v = out[q * lpl] + couts[q - 1]
        out[q * lpl] = v & M
        out[q * lpl + 1] += v >> W
    return out


def moduli_for(lpl, rng):
    cap = 29 * 4 * lpl - 2
    qs = [H.random_odd_modulus(cap, rng), (1 << cap) - 1, (1 << (cap - 1)) + 1, H.random_odd_modulus(cap - 100, rng)]
    if lpl == 18:
        qs.append(int(O.MODP_Q_HEX, 16))
    return qs


@pytest.mark.parametrize("lpl", WIDTHS)
def test_product_and_squaring_match_montgomery_with_runtime_n0inv(lpl):
    rng = random.Random(lpl)
    L = 4 * lpl
    R = 1 << (W * L)
    stats = {"maxacc": 0}
    n0invs = set()
    for N in moduli_for(lpl, rng):
        assert 4 * N < R
        n0invs.add((-pow(N, -1, 1 << W)) % (1 << W))
        rinv = pow(R, -1, N)
        cases = [(2 * N - 1, 2 * N - 1), (0, 2 * N - 1), (1, N)] + [(rng.randrange(2 * N), rng.randrange(2 * N)) for _ in range(6)]
        for a, b in cases:
            for sq in (False, True):
                bb = a if sq else b
                r = mont_model(limbs(a, L), limbs(bb, L), N, lpl, L, stats, square=sq)
                v = val(r)
                assert v < 2 * N and v % N == a * bb * rinv % N
                assert max(r) <= LIMB_BOUND
    assert len(n0invs - {1}) >= 2, "the run-time n0inv must be exercised with values other than 1"
    assert stats["maxacc"] < (1 << 64)


@pytest.mark.parametrize("lpl", WIDTHS)
def test_worst_case_limbs_do_not_overflow(lpl):
    """every limb at the almost-normalised bound (far above 2N as an integer): the 64-bit columns must still hold -- at most
    2 lpl products between two carries of a column"""
    rng = random.Random(100 + lpl)
    L = 4 * lpl
    for N in moduli_for(lpl, rng)[:2]:
        stats = {"maxacc": 0}
        mont_model([LIMB_BOUND] * L, [LIMB_BOUND] * L, N, lpl, L, stats, bound_only=True)
        mont_model([LIMB_BOUND] * L, [LIMB_BOUND] * L, N, lpl, L, stats, square=True, bound_only=True)
        mont_model([LIMB_BOUND] * L, [M] * in_rows(lpl), N, lpl, in_rows(lpl), stats, bound_only=True)
        assert stats["maxacc"].bit_length() <= 64
        assert stats["maxacc"] < 2 * lpl * LIMB_BOUND * LIMB_BOUND + (1 << 40)


@pytest.mark.parametrize("lpl", WIDTHS)
def test_long_product_brings_any_2048_bit_input_into_the_width(lpl):
    """to_mont_in: kin = 2^(29 (IN_ROWS + L)) mod N times the input's IN_ROWS limbs gives in R mod N below 2N, for inputs up
    to 2^2048 - 1 (far above N for the narrow widths)"""
    rng = random.Random(200 + lpl)
    L, rows = 4 * lpl, in_rows(lpl)
    assert rows % lpl == 0 and rows >= 72
    R = 1 << (W * L)
    stats = {"maxacc": 0}
    for N in moduli_for(lpl, rng)[:3]:
        kin = pow(2, W * (rows + L), N)
        for x in (0, 1, N, N + 1, (1 << 2048) - 1, rng.randrange(1 << 2048)):
            r = mont_model(limbs(kin, L), limbs(x, rows), N, lpl, rows, stats)
            v = val(r)
            assert v < 2 * N and v % N == x * R % N
    assert stats["maxacc"] < (1 << 64)


def test_width_choice_and_bad_moduli():
    for bits, lpl in ((3, 5), (64, 5), (578, 5), (579, 9), (1042, 9), (1043, 18), (2048, 18)):
        q = (1 << (bits - 1)) | 1 if bits > 3 else 5
        g = capi.ModpGroup(q)
        assert g.bits == q.bit_length() and g.limbs_per_lane == lpl == H.width_for_bits(q.bit_length())
        g.close()
    for bad in (0, 1, 2, 3, 4, 6, 1 << 100, (1 << 2048) + 1, 1 << 2048):
        with pytest.raises(capi.EngineError):
            capi.ModpGroup(bad)
    # leading zero bytes are allowed
    lib = capi.load_library()
    import ctypes as C
    h = C.c_void_p()
    q = bytes(8) + (23).to_bytes(1, "big")
    assert lib.mpvss_modp_group_create(q, len(q), C.byref(h)) == 0
    assert lib.mpvss_modp_group_bits(h) == 5
    lib.mpvss_modp_group_destroy(h)


@pytest.mark.parametrize("bits", [64, 2048])
def test_hash_to_scalar_against_the_oracle(bits):
    q = H.small_safe_primes()[64] if bits == 64 else H.rfc_prime(2048)
    g = H.RtOracleGroup(q)
    grp = capi.ModpGroup(q)
    for data in (b"", b"abc", bytes(range(200)), b"\xff" * 64):
        want = g.hash_to_scalar(data)
        assert int.from_bytes(grp.hash_to_scalar(data), "big") == want
    if bits == 64:      # a real reduction: most digests exceed (q-1)/2
        assert any(int.from_bytes(hashlib.sha256(d).digest(), "big") >= g.g for d in (b"", b"abc"))


def test_moduli_of_the_tests():
    """the RFC formula (Machin's pi) gives safe primes, and the 2048-bit one is the oracle's group 14; the stored small safe
    primes are safe primes of their sizes"""
    for k in (768, 1024, 1536, 2048):
        q = H.rfc_prime(k)
        assert q.bit_length() == k and H.miller_rabin(q, 8) and H.miller_rabin((q - 1) // 2, 8)
    assert H.rfc_prime(2048) == int(O.MODP_Q_HEX, 16)
    for bits, q in H.small_safe_primes().items():
        assert q.bit_length() == bits and H.miller_rabin(q) and H.miller_rabin((q - 1) // 2)
