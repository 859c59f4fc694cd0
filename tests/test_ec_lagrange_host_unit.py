"""The lane body of k_ec_lagrange on the CPU: tests/ec_lagrange_unit.cpp is a stand-alone host program (its own main) that includes
mpvss_rs_amd/csrc/ec_lagrange.h and ec_scalar.h and calls the very inline functions the kernel calls -- ScalarField::mont_step_u64,
the two product loops over staged tiles with the lane's own index skipped, the Fermat inverse, the sign, the byte order.  Every case
of tests/ec_lagrange_cases.py, both orders, against Python integers; and the m = 4097 list of the GPU module.  No GPU."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

import ec_lagrange_cases as LC

EXE = os.path.join(HERE, "_build", "ec_lagrange_unit")


@pytest.fixture(scope="module")
def unit():
    """the program, built by the library's Makefile (`make examples`); rebuilt here when a source is newer"""
    csrc = os.path.join(HERE, "..", "mpvss_rs_amd", "csrc")
    src = os.path.join(HERE, "ec_lagrange_unit.cpp")
    deps = [src] + [os.path.join(csrc, h) for h in ("ec_lagrange.h", "ec_scalar.h", "ec_consts.h", "ec_field.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", EXE])

    def run(lists):
        text = "".join(f"{len(xs)} " + " ".join(map(str, xs)) + "\n" for xs in lists)
        out = subprocess.run([EXE], input=text, capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 2 * sum(len(xs) for xs in lists)
        res, k = [], 0
        for xs in lists:
            rows = out[k:k + 2 * len(xs)]
            k += 2 * len(xs)
            res.append({"secp256k1": bytes.fromhex("".join(rows[0::2])), "ristretto255": bytes.fromhex("".join(rows[1::2]))})
        return res

    return run


def test_every_case_both_orders(unit):
    cases = LC.cases()
    got = unit([xs for _, xs in cases])
    for (cid, xs), g in zip(cases, got):
        for name in LC.CURVES:
            assert g[name] == LC.expected_of(name, cid, xs), (name, cid)


def test_seventeen_staging_trips(unit):
    xs = LC.shape_positions(LC.BIG_M)
    g = unit([xs])[0]
    for name in LC.CURVES:
        assert g[name] == LC.expected_of(name, f"shuffled-{LC.BIG_M}", xs), name


def test_a_zero_difference_neither_faults_nor_loops(unit):
    """duplicates never reach the kernel (the host refuses them): the lane body must merely end.  The two lanes of the duplicate
    have a zero denominator and give 0; the others give some value nobody uses."""
    g = unit([[3, 5, 3, 9]])[0]
    for name in LC.CURVES:
        assert len(g[name]) == 128 and g[name][0:32] == bytes(32) and g[name][64:96] == bytes(32)
