"""Moduli, byte packing and the oracle's protocol runs for the tests of a 512-byte run-time MODP group (moduli of 3073 .. 4096
bits): tests/test_modp_rt_4096_*.py and tests/test_gpu_modp_rt_4096.py.  RFC 3526 group 16 is computed like the narrower RFC
primes of modp_rt_helpers: 2^4096 - 2^4032 - 1 + 2^64 (floor(2^3966 pi) + 240904)."""
import functools
import random

import modp_rt_helpers as H

EB = 512                     # element / scalar bytes of the handle
LPL = 36                     # limbs per lane it runs at
TOP = (1 << 4096) - 1
SECRET = 0x1234
TAMPER_ROW = 2


@functools.lru_cache(maxsize=None)
def group16():
    return 2 ** 4096 - 2 ** 4032 - 1 + 2 ** 64 * (H.pi_scaled(3966) + 240904)


@functools.lru_cache(maxsize=None)
def odd_3073():
    """a fixed random odd modulus of 3073 bits: the narrowest a 512-byte handle takes (not a prime)"""
    return H.random_odd_modulus(3073, random.Random(3073))


def be(v, eb=EB):
    return v.to_bytes(eb, "big")


def cat(values, eb=EB):
    return b"".join(v.to_bytes(eb, "big") for v in values)


def split(buf, eb=EB):
    return [int.from_bytes(buf[i:i + eb], "big") for i in range(0, len(buf), eb)]


def picks(n, t):
    """the share subsets the oracle reconstructs from: all n, exactly t spread ones, the first t, the last t"""
    return [list(range(n)), sorted({round(i * (n - 1) / (t - 1)) for i in range(t)}), list(range(t)), list(range(n - t, n))]


@functools.lru_cache(maxsize=None)
def protocol_run(n, t):
    """mpvss_oracle over H.RtOracleGroup(group16()) through the whole protocol, once per process and left unchanged: keys, the
    dealer's box with its X, a1, a2 and digest, every participant's extracted share with its proof, the secret reconstructed
    from picks(n, t) and, for n <= 5, the verdict on the box with the last byte of share TAMPER_ROW flipped.  The run takes some
    450 exponentiations at (33, 4), 0.2 s each with Python's pow: like modp_rt_many_helpers.case() for its large groups, the
    oracle's ModpGroup.exp goes over libcrypto's BN_mod_exp where libcrypto is at hand (a few seconds for both shapes)."""
    import mpvss_oracle as O
    import modp_rt_many_helpers as M
    g = H.RtOracleGroup(group16())
    rng = random.Random(4096 * n + t)
    privs = [H.keygen(g, rng) for _ in range(n)]
    coeffs = [rng.randrange(1, g.q - 1) for _ in range(t)]
    ws, w2 = [H.keygen(g, rng) for _ in range(n)], [H.keygen(g, rng) for _ in range(n)]
    with M.libcrypto_pow(M.LARGE[-1]):                 # (the name only says "a large group")
        pks = [g.generate_public_key(k) for k in privs]
        assert len(set(pks)) == n
        box = O.distribute_secret(g, SECRET, pks, t, coeffs, ws)
        keys = [g.element_to_bytes(p) for p in pks]
        assert [box["positions"][k] for k in keys] == list(range(1, n + 1))
        sbs = [O.extract_secret_share(g, box, k, w) for k, w in zip(privs, w2)]
        reconstructed = [(pick, O.reconstruct(g, [sbs[i] for i in pick], box)) for pick in picks(n, t)]
        tampered_valid = None
        if n <= 5:
            bad_shares = dict(box["shares"])
            bad_shares[keys[TAMPER_ROW]] ^= 1
            tampered_valid = bool(O.verify_distribution_shares(g, dict(box, shares=bad_shares)))
    return dict(privs=privs, coeffs=coeffs, ws=ws, w2=w2, pks=pks, commitments=box["commitments"], Y=[box["shares"][k] for k in keys],
                X=box["_X"], a1=box["_a1"], a2=box["_a2"], digest=box["_digest"], challenge=box["challenge"],
                responses=[box["responses"][k] for k in keys], U=box["U"], share=[sb["share"] for sb in sbs],
                share_challenge=[sb["challenge"] for sb in sbs], share_response=[sb["response"] for sb in sbs],
                reconstructed=reconstructed, tampered_valid=tampered_valid)
