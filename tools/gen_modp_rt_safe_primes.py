"""Safe primes q = 2p + 1 of 40, 64, 128, 256 and 512 bits for the run-time MODP group tests (tests/golden/modp_rt/safe_primes.json).

A seeded search (random.Random(2026)): odd candidates p with the top bit set, small-prime sieve on p and 2p + 1, then Miller-Rabin
(40 rounds) on both.  The 40-bit prime leaves room for int64 positions that are multiples of q - 1.  Re-running gives the same file."""
import json
import os
import random
import sys

SMALL = [p for p in range(3, 2000) if all(p % d for d in range(2, int(p ** 0.5) + 1))]


def is_probable_prime(n, rng, rounds=40):
    if n < 2:
        return False
    for p in SMALL:
        if n % p == 0:
            return n == p
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


def safe_prime(bits, rng):
    while True:
        p = rng.getrandbits(bits - 1) | (1 << (bits - 2)) | 1
        q = 2 * p + 1
        if any(p % s == 0 and p != s or q % s == 0 for s in SMALL):
            continue
        if is_probable_prime(p, rng) and is_probable_prime(q, rng):
            return q


def main():
    rng = random.Random(2026)
    out = {str(b): hex(safe_prime(b, rng)) for b in (40, 64, 128, 256, 512)}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "modp_rt", "safe_primes.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    sys.exit(main())
