"""Rates of the run-time MODP group entry points (include/mpvss_hip.h, mpvss_modp_group_*) on one GPU.

  batch_exp   n = 65536 bases and exponents as long as the modulus, at 512, 1024, 1536 and 2048 bits, beside the group-14
              entry point mpvss_modp_batch_exp on the same shape (random 2048-bit exponents)
  verify      mpvss_modp_group_verify_distribution at (n, t) = (4096, 64) and (65536, 256) for 1024, 1536 and 2048 bits:
              share verifications per second (random box contents: the same work as a valid box, the verdict is 0)

Host buffers in and out (the calls' own staging included), best of `--reps` after one warm-up call.  One JSON line per
measurement.  Usage: python tools/modp_rt_rate.py [--quick] [--reps 3]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import modp_rt_helpers as H  # noqa: E402
from mpvss_rs_amd import Engine, ModpGroup  # noqa: E402


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def kernel_ms(eng):
    """GPU time of the last call's kernels (hipEvents around each launch, summed over the kinds of mpvss_last_kernel_ms)"""
    return round(sum(max(0.0, eng.kernel_ms(k)) for k in range(4)), 3)


def rand_bytes(rng, n, bits):
    return b"".join(rng.getrandbits(bits).to_bytes(256, "big") for _ in range(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="smaller shapes (a check of the tool, not a measurement)")
    a = ap.parse_args()
    eng = Engine(0)
    rng = random.Random(1)
    n = 4096 if a.quick else 65536
    moduli = {512: H.small_safe_primes()[512], 1024: H.rfc_prime(1024), 1536: H.rfc_prime(1536), 2048: H.rfc_prime(2048)}
    rates = {}
    for bits, q in moduli.items():
        grp = ModpGroup(q)
        B, E = rand_bytes(rng, n, 2048), rand_bytes(rng, n, bits)
        s = best(lambda: eng.group_batch_exp(grp, B, E), a.reps)
        kms = kernel_ms(eng)
        rates[bits] = n / (kms / 1e3)
        print(json.dumps({"what": "group_batch_exp", "bits": bits, "limbs_per_lane": grp.limbs_per_lane, "n": n,
                          "s": round(s, 4), "exps_per_s": round(n / s), "kernel_ms": kms,
                          "kernel_exps_per_s": round(rates[bits])}), flush=True)
    B, E = rand_bytes(rng, n, 2048), rand_bytes(rng, n, 2048)
    s = best(lambda: eng.batch_exp(B, E), a.reps)
    kms = kernel_ms(eng)
    print(json.dumps({"what": "group14_batch_exp", "bits": 2048, "n": n, "s": round(s, 4), "exps_per_s": round(n / s),
                      "kernel_ms": kms, "kernel_exps_per_s": round(n / (kms / 1e3)),
                      "kernel_runtime_2048_over_group14": round(rates[2048] / (n / (kms / 1e3)), 3),
                      "kernel_runtime_1024_over_2048": round(rates[1024] / rates[2048], 2),
                      "kernel_runtime_512_over_2048": round(rates[512] / rates[2048], 2)}), flush=True)
    shapes = [(4096, 64), (8192, 64)] if a.quick else [(4096, 64), (65536, 256)]
    for bits in (1024, 1536, 2048):
        grp = ModpGroup(moduli[bits])
        for nn, t in shapes:
            cm = rand_bytes(rng, t, bits)
            pos = list(range(1, nn + 1))
            y, Y, r = rand_bytes(rng, nn, bits), rand_bytes(rng, nn, bits), rand_bytes(rng, nn, bits)
            c = rng.getrandbits(min(bits - 2, 256)).to_bytes(256, "big")
            s = best(lambda: eng.group_verify_distribution(grp, cm, pos, y, Y, r, c), a.reps)
            print(json.dumps({"what": "group_verify_distribution", "bits": bits, "n": nn, "t": t, "s": round(s, 4),
                              "share_verifications_per_s": round(nn / s), "kernel_ms": kernel_ms(eng)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
