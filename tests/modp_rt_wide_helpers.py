"""Moduli and byte packing for the tests of a wide run-time MODP group (384-byte elements, moduli of 2049 .. 3072 bits):
tests/test_modp_rt_wide_*.py and tests/test_gpu_modp_rt_wide.py.  RFC 3526 group 15 is computed like the narrower RFC
primes of modp_rt_helpers: 2^3072 - 2^3008 - 1 + 2^64 (floor(2^2942 pi) + 1690314)."""
import functools
import random

import modp_rt_helpers as H

EB = 384                     # element / scalar bytes of a wide handle
LPL = 27                     # limbs per lane it runs at
TOP = (1 << 3072) - 1


@functools.lru_cache(maxsize=None)
def group15():
    return 2 ** 3072 - 2 ** 3008 - 1 + 2 ** 64 * (H.pi_scaled(2942) + 1690314)


@functools.lru_cache(maxsize=None)
def odd_2049():
    """a fixed random odd modulus of 2049 bits: the narrowest a wide handle takes (not a prime)"""
    return H.random_odd_modulus(2049, random.Random(2049))


def be(v, eb=EB):
    return v.to_bytes(eb, "big")


def cat(values, eb=EB):
    return b"".join(v.to_bytes(eb, "big") for v in values)


def split(buf, eb=EB):
    return [int.from_bytes(buf[i:i + eb], "big") for i in range(0, len(buf), eb)]
