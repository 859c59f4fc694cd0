"""Moduli and oracle groups for the run-time MODP group tests (tests/test_modp_rt_*.py, tests/test_gpu_modp_rt.py).

The RFC 2409 / 3526 safe primes are computed here, not stored: q = 2^k - 2^(k-64) - 1 + 2^64 (floor(2^(k-130) pi) + c), pi from
Machin's formula in integers.  The small safe primes come from tools/gen_modp_rt_safe_primes.py (tests/golden/modp_rt/safe_primes.json)."""
import json
import os
import random

import mpvss_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))

RFC_C = {768: 149686, 1024: 129093, 1536: 741804, 2048: 124476}


def _arctan_inv(x, one):
    """one * arctan(1/x), integer series"""
    total, term, k, sign = 0, one // x, 1, 1
    x2 = x * x
    while term:
        total += sign * (term // k)
        term //= x2
        k += 2
        sign = -sign
    return total


def pi_scaled(bits):
    """floor(pi * 2^bits) (Machin: pi = 16 atan(1/5) - 4 atan(1/239)), with guard bits"""
    guard = 64
    one = 1 << (bits + guard)
    return (16 * _arctan_inv(5, one) - 4 * _arctan_inv(239, one)) >> guard


def rfc_prime(k):
    return 2 ** k - 2 ** (k - 64) - 1 + 2 ** 64 * (pi_scaled(k - 130) + RFC_C[k])


def miller_rabin(n, rounds=24, seed=1):
    if n < 4:
        return n in (2, 3)
    if n % 2 == 0:
        return False
    rng = random.Random(seed)
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for _ in range(rounds):
        a = rng.randrange(2, n - 1)
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def small_safe_primes():
    with open(os.path.join(HERE, "golden", "modp_rt", "safe_primes.json")) as fh:
        return {int(k): int(v, 16) for k, v in json.load(fh).items()}


def width_for_bits(bits):
    """limbs per lane the library picks: the smallest of 5, 9, 18 with bits <= 29 * 4 * lpl - 2"""
    for lpl in (5, 9, 18):
        if bits <= 29 * 4 * lpl - 2:
            return lpl
    return None


def random_odd_modulus(bits, rng):
    return rng.getrandbits(bits - 1) | (1 << (bits - 1)) | 1


class RtOracleGroup(O.ModpGroup):
    """The oracle's ModpGroup with the constants of ModpGroup::init (src/groups/modp.rs:72-84): q, g = (q-1)/2, G = 2,
    g_gen = 4 mod q, q - 1.  Every method of the oracle then runs over this modulus (oracle/ itself is unchanged)."""

    def __init__(self, q):
        super().__init__()
        self.q = q
        self.g = (q - 1) // 2
        self.G = 2
        self.g_gen = pow(2, 2, q)
        self.q_minus_1 = q - 1
        self.name = "modp2048"     # the oracle's MODP code paths (scalar reductions of distribute_secret)


def keygen(g, rng):
    import math
    while True:
        k = rng.randrange(1, g.q)
        if math.gcd(k, g.q - 1) == 1:
            return k


def make_instance(q, n, t, seed):
    """a box of distribute_secret over the group of q, with the oracle's own dealer"""
    g = RtOracleGroup(q)
    rng = random.Random(seed)
    privs = [keygen(g, rng) for _ in range(n)]
    pks = [g.generate_public_key(k) for k in privs]
    # distinct keys: the box maps shares by the key's bytes (small groups can repeat a key)
    seen, P, K = set(), [], []
    for k, pk in zip(privs, pks):
        if pk not in seen:
            seen.add(pk)
            P.append(pk)
            K.append(k)
    coeffs = [rng.randrange(g.q - 1) for _ in range(t)]
    ws = [keygen(g, rng) for _ in range(len(P))]
    box = O.distribute_secret(g, 0x1234, P, min(t, len(P)), coeffs[:min(t, len(P))], ws)
    return g, K, P, box
