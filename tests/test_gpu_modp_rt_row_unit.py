"""The run-time row-layout Montgomery product on the device (mpvss_rs_amd/csrc/bn_row_rt.h through tests/modp_rt_row_unit.hip): one
product and one squaring per operand pair at each of the three widths -- (L, row LPL) = (72, 5), (108, 7), (144, 9) -- against
Python integers, on operands at the bounds of the integer model (tests/test_modp_rt_row_model.py) and a run-time n0inv."""
import os
import random
import struct
import subprocess

import pytest

import modp_rt_helpers as H
import modp_rt_wide_helpers as WH
import modp_rt_4096_helpers as XH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 29
M29 = (1 << W) - 1
LIM = M29 + 512
ROW_LPL = {18: 5, 27: 7, 36: 9}


def moduli(ql):
    """the RFC 3526 prime of the width (n0inv = 1) and a random odd modulus of the width's capacity (another n0inv)"""
    rfc = {18: lambda: H.rfc_prime(2048), 27: WH.group15, 36: XH.group16}[ql]()
    return [rfc, H.random_odd_modulus(W * 4 * ql - 2, random.Random(ql))]


@pytest.mark.parametrize("ql", sorted(ROW_LPL))
def test_row_product_and_square_on_edge_operands(tmp_path, ql):
    exe = os.path.join(ROOT, "tests", "_build", "modp_rt_row_unit")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mpvss_rs_amd", "csrc"), "../../tests/_build/modp_rt_row_unit"])
    L, lpl = 4 * ql, ROW_LPL[ql]
    R = 1 << (W * L)
    fmt = f"<{L}I"
    canon = lambda v: [(v >> (W * j)) & M29 for j in range(L)]
    value = lambda l: sum(x << (W * j) for j, x in enumerate(l))
    for which_n, N in enumerate(moduli(ql)):
        rng = random.Random(0x50E + ql + which_n)
        n0inv = (-pow(N, -1, 1 << W)) % (1 << W)
        assert 4 * N < R and (n0inv != 1) == bool(which_n)

        def loose():      # a value below 2N whose limbs are "almost normalised" (up to 2^29 - 1 + 2^9), as a product leaves them
            while True:
                l = canon(rng.randrange(2 * N))
                for j in range(L - 1):
                    if rng.random() < 0.3 and l[j + 1] > 0:
                        l[j] += 1 << W
                        l[j + 1] -= 1
                        l[j] = min(l[j], LIM)
                if value(l) < 2 * N:
                    return l
        maxl = [LIM] * L                                   # every limb at the bound, the top ones lowered until below 2N
        j = L - 1
        while value(maxl) >= 2 * N:
            if maxl[j] == 0:
                j -= 1
            maxl[j] //= 2
        k = 3 * lpl                                        # 2^(29 k): the lowest limb of lane 3; 14 lpl: of lane 14, below N
        assert all(value(canon(v)) == v for v in ((1 << (W * (14 * lpl))) + 1, 2 * N - 1)) and (1 << (W * (14 * lpl))) + 1 < N
        named = [canon(v) for v in (0, 1, N - 1, N, N + 1, 2 * N - 1, (1 << (W * k)) - 1, 1 << (W * k), (1 << (W * k)) + 1,
                                    (1 << (W * (14 * lpl))) - 1, (1 << (W * (14 * lpl))) + 1)] + [maxl]
        pairs = [(a, b) for a in named for b in named]
        pairs += [(canon(rng.randrange(2 * N)), canon(rng.randrange(2 * N))) for _ in range(300)]
        pairs += [(loose(), loose()) for _ in range(300)]
        pairs.append((maxl, maxl))
        n = len(pairs)
        assert n % 4 != 0                                                    # the last wave is ragged
        inp, outp = tmp_path / f"in{which_n}.bin", tmp_path / f"out{which_n}.bin"
        with open(inp, "wb") as f:
            f.write(struct.pack("<I", n0inv) + struct.pack(fmt, *canon(N)))
            for a, b in pairs:
                f.write(struct.pack(fmt, *a) + struct.pack(fmt, *b))
        res = subprocess.run(["timeout", "-k", "10", "120", exe, str(ql), str(inp), str(outp), str(n)], capture_output=True, text=True,
                             timeout=150)
        assert res.returncode == 0, res.stdout + res.stderr
        raw = open(outp, "rb").read()
        assert len(raw) == n * 2 * 4 * L
        Rinv = pow(R, -1, N)
        for i, (a, b) in enumerate(pairs):
            x, y = value(a), value(b)
            for which, (p, q) in enumerate(((x, y), (x, x))):
                limbs = struct.unpack_from(fmt, raw, (2 * i + which) * 4 * L)
                v = value(limbs)
                assert max(limbs) <= LIM, (ql, which_n, i, which, hex(max(limbs)))
                assert v < 2 * N and v % N == p * q * Rinv % N, (ql, which_n, i, which)
