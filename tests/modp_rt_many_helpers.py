"""Boxes for the tests of mpvss_modp_group_verify_many (tests/test_gpu_modp_rt_verify_many.py).

Every box comes from modp_rt_helpers.make_instance -- the oracle's own dealer over RtOracleGroup -- and its validity from the
oracle's verify_distribution_shares.  At 2048 and 3072 bits one modular power costs Python 30 and 105 ms, the boxes of one test
a minute: for those groups `libcrypto_pow` puts libcrypto's BN_mod_exp (the loader of oracle/openssl_ref.py) in the place of
Python's pow inside the oracle's ModpGroup.exp while the boxes are dealt and judged -- the oracle's protocol code runs
unchanged, and tests/test_modp_rt_many_boxes_host.py holds the two powers equal.  Without libcrypto the tests are as right and
slower."""
import contextlib
import ctypes as C
import functools

import mpvss_oracle as O
import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import openssl_ref

GROUPS = {                                # name -> (q, element bytes, limbs per lane)
    "40": (lambda: H.small_safe_primes()[40], 256, 5),
    "256": (lambda: H.small_safe_primes()[256], 256, 5),
    "1024": (lambda: H.rfc_prime(1024), 256, 9),
    "2048": (lambda: H.rfc_prime(2048), 256, 18),
    "3072": (WH.group15, WH.EB, 27),
}
LARGE = ("2048", "3072")
# tile edges 15 / 16 / 17 / 33, t = 1, adjacent tiles with different t, one shape twice
SHAPES = [(1, 1), (5, 3), (15, 2), (16, 4), (17, 17), (33, 2), (5, 3)]
# one flipped byte per box of a run of five boxes of (5, 3): (array, row) -- the lowest byte of that element
TAMPERS = [("shares", 2), ("responses", 4), ("commitments", 1), ("pubkeys", 0), ("challenge", 0)]
TAMPER_SHAPE = (5, 3)


def cat(vals, eb):
    return b"".join(v.to_bytes(eb, "big") for v in vals)


def split(b, eb):
    return [int.from_bytes(b[i:i + eb], "big") for i in range(0, len(b), eb)]


def flip(buf, row, eb):
    b = bytearray(buf)
    b[row * eb + eb - 1] ^= 1
    return bytes(b)


def bn_mod_exp(base, e, q):
    """base^e mod q (q odd) by libcrypto"""
    lib = openssl_ref._load()
    ctx = lib.BN_CTX_new()
    raw = [v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big") for v in (base, e, q)]
    bns = [lib.BN_bin2bn(b, len(b), None) for b in raw]
    out = lib.BN_new()
    try:
        assert lib.BN_mod_exp_mont(out, bns[0], bns[1], bns[2], ctx, None) == 1
        size = len(raw[2])
        buf = (C.c_uint8 * size)()
        assert lib.BN_bn2binpad(out, buf, size) == size
        return int.from_bytes(bytes(buf), "big")
    finally:
        for b in bns + [out]:
            lib.BN_free(b)
        lib.BN_CTX_free(ctx)


@contextlib.contextmanager
def libcrypto_pow(name):
    """for a LARGE group and with libcrypto at hand: the oracle's ModpGroup.exp over BN_mod_exp inside the block"""
    if name not in LARGE or not openssl_ref.available():
        yield
        return
    plain = O.ModpGroup.exp

    def exp(self, base, scalar):
        if scalar < 0 or self.q % 2 == 0:
            return plain(self, base, scalar)
        return bn_mod_exp(base, scalar, self.q)

    O.ModpGroup.exp = exp
    try:
        yield
    finally:
        O.ModpGroup.exp = plain


def flat_box(g, pks, box, eb):
    """the arrays the C ABI takes, in the order of the box's public keys"""
    keys = [g.element_to_bytes(p) for p in pks]
    return dict(commitments=cat(box["commitments"], eb), positions=[box["positions"][k] for k in keys], pubkeys=cat(pks, eb),
                shares=cat([box["shares"][k] for k in keys], eb), responses=cat([box["responses"][k] for k in keys], eb),
                challenge=cat([box["challenge"]], eb))


def oracle_verdict(q, eb, flat):
    """the oracle's verify_distribution_shares on the arrays of a flat box (tampered or not)"""
    g = H.RtOracleGroup(q)
    pks = split(flat["pubkeys"], eb)
    keys = [g.element_to_bytes(p) for p in pks]
    box = dict(publickeys=pks, commitments=split(flat["commitments"], eb), challenge=split(flat["challenge"], eb)[0],
               positions=dict(zip(keys, flat["positions"])), shares=dict(zip(keys, split(flat["shares"], eb))),
               responses=dict(zip(keys, split(flat["responses"], eb))))
    return bool(O.verify_distribution_shares(g, box))


def dealt_box(name, n, t, seed):
    q, eb = GROUPS[name][0](), GROUPS[name][1]
    g, _, pks, box = H.make_instance(q, n, t, seed)
    assert len(pks) == n, "make_instance dropped a repeated key: take another seed"
    return flat_box(g, pks, box, eb)


def tampered(flat, eb, kind):
    arr, row = kind
    return dict(flat, **{arr: flip(flat[arr], row, eb)})


@functools.lru_cache(maxsize=None)
def case(name):
    """{"mixed": [flat boxes of SHAPES], "run": [five flat boxes of TAMPER_SHAPE], "mixed_valid", "run_valid", "tampered_valid"}:
    everything the oracle has to say about the boxes of the tests, for one group; computed once per process, left unchanged"""
    q, eb = GROUPS[name][0](), GROUPS[name][1]
    with libcrypto_pow(name):
        mixed = [dealt_box(name, n, t, 100 + k) for k, (n, t) in enumerate(SHAPES)]
        run = [dealt_box(name, *TAMPER_SHAPE, 200 + k) for k in range(len(TAMPERS))]
        return dict(mixed=mixed, run=run, mixed_valid=[oracle_verdict(q, eb, b) for b in mixed],
                    run_valid=[oracle_verdict(q, eb, b) for b in run],
                    tampered_valid=[oracle_verdict(q, eb, tampered(b, eb, kind)) for b, kind in zip(run, TAMPERS)])
