"""Integer model of k_rt_twin_exp / k_rt_twin_combine (mpvss_rs_amd/csrc/modp_rt_kernels.hip): two powers of one base, right to
left over 4-bit windows into 15 buckets per exponent with the squarings shared, then the running-product combine.  The model
runs in Montgomery form at each width's R = 2^(29 L) and counts every Montgomery operation a wave issues; the count for
full-width exponents at 2048 bits is the figure DESIGN section 13 quotes.  No GPU, no library."""
import os
import random
import re

import pytest

import modp_rt_helpers as H

WINDOW = 4
BUCKETS = (1 << WINDOW) - 1
WIDTHS = {5: 20, 9: 36, 18: 72}          # limbs per lane -> L


class Mont:
    def __init__(self, q, L):
        self.q, self.R = q, 1 << (29 * L)
        assert self.R > 4 * q
        self.Rinv = pow(self.R, -1, q)
        self.ops = {"entry": 0, "square": 0, "bucket": 0, "combine": 0, "exit": 0}

    def mul(self, a, b, kind):
        self.ops[kind] += 1
        return a * b * self.Rinv % self.q


def twin_model(q, L, base, e1, e2):
    """(base^e1 mod q, base^e2 mod q, operation counts) the way the kernels compute them"""
    m = Mont(q, L)
    one_m = m.R % q
    # to_mont_in: one long product takes any 256-byte value into Montgomery form (reduced mod q on the way)
    m.ops["entry"] += 1
    p = base * m.R % q
    K = [[one_m] * BUCKETS for _ in range(2)]
    nb = max(e1.bit_length(), e2.bit_length())
    nw = (nb + WINDOW - 1) // WINDOW
    for w in range(nw):
        for k, e in enumerate((e1, e2)):
            d = (e >> (WINDOW * w)) & BUCKETS
            if d:                                     # (a wave skips the product only when the digit is 0 in all 16 numbers)
                K[k][d - 1] = m.mul(K[k][d - 1], p, "bucket")
        if w + 1 < nw:
            for _ in range(WINDOW):
                p = m.mul(p, p, "square")
    out = []
    for k in range(2):
        s = t = K[k][BUCKETS - 1]
        for j in range(BUCKETS - 2, -1, -1):
            s = m.mul(s, K[k][j], "combine")
            t = m.mul(t, s, "combine")
        out.append(m.mul(t, 1, "exit"))
    return out[0], out[1], m.ops


def _edge_pairs(bits):
    full = (1 << bits) - 1
    return [(0, 0), (1, 1), (0, full), (full, 0), (full, full), (1, full), (0, 1), (1 << (bits - 1), 3)]


@pytest.mark.parametrize("lpl", sorted(WIDTHS))
def test_model_equals_pow(lpl):
    L = WIDTHS[lpl]
    bits = 29 * L - 2
    rng = random.Random(lpl)
    for q in (H.random_odd_modulus(bits, rng), H.random_odd_modulus(bits - 7, rng), 5 if lpl == 5 else H.random_odd_modulus(bits // 2 + 300, rng)):
        if H.width_for_bits(q.bit_length()) != lpl:
            continue
        pairs = _edge_pairs(min(2048, bits)) + _edge_pairs(2048) + [(rng.getrandbits(2048), rng.getrandbits(q.bit_length())) for _ in range(6)]
        for e1, e2 in pairs:
            for base in (0, 1, q - 1, q, q + 1, (1 << 2048) - 1, rng.getrandbits(2048)):
                r1, r2, _ = twin_model(q, L, base, e1, e2)
                assert (r1, r2) == (pow(base, e1, q), pow(base, e2, q)), (lpl, base, e1, e2)


def test_operation_count_is_the_documented_figure():
    q = H.rfc_prime(2048)
    full = (1 << 2048) - 1
    _, _, ops = twin_model(q, 72, 3, full, full)
    assert ops == {"entry": 1, "square": 2044, "bucket": 1024, "combine": 56, "exit": 2}
    total = sum(ops.values())
    assert total == 3127
    # two k_rt_dual_exp chains over a 16-entry table each: 14 table products + per exponent 2044 squarings + 511 window
    # products + 1 exit, and the entry of the base
    two_chains = 2 * (1 + 14 + 2044 + 511 + 1)
    assert two_chains == 5142
    # random exponents as long as q: a digit is 0 in one window of 16, for one share; a wave of 16 shares skips nothing
    rng = random.Random(1)
    e1, e2 = rng.getrandbits(2048) | 1 << 2047, rng.getrandbits(2048) | 1 << 2047
    _, _, ops = twin_model(q, 72, 3, e1, e2)
    assert 900 <= ops["bucket"] <= 1024 and ops["square"] == 2044
    design = open(os.path.join(os.path.dirname(H.HERE), "DESIGN.md")).read()
    sec13 = design[design.index("## 13"):]
    assert re.search(r"\b3 ?127\b", sec13) and re.search(r"\b5 ?142\b", sec13), "DESIGN section 13 must quote the model's counts"


def test_cost_follows_the_operands():
    q = H.small_safe_primes()[256]
    _, _, ops = twin_model(q, 20, 7, (1 << 64) - 1, 5)
    assert ops["square"] == 4 * 15 and ops["bucket"] == 16 + 1
    _, _, ops = twin_model(q, 20, 7, 0, 0)
    assert ops["square"] == 0 and ops["bucket"] == 0 and ops["combine"] == 56
