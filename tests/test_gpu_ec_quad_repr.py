"""The lane-parallel point additions of mpvss_rs_amd/csrc/ec_quad.h (QuadSecp, QuadRist, OctSecp) on weakly reduced operands:
the raw mode of tests/ec_quad_unit.hip takes P = a G and Q = b G as limb words -- the cases of tests/ec_repr_cases.py, so
doublings, P + (-P) and every non-canonical identity arrive on either side at saturated limbs -- and returns P + Q, (-P) + Q
and the stepping recurrence D <- D + Q after 1, 2 and 64 steps through Q::load, Q::neg, Q::add, Q::out_words and the one-lane
encode (pinned by tests/test_gpu_ec_repr.py); the bytes are compared with oracle/ec_ref.c's."""
import os

import pytest

import ec_repr_cases as R

pytestmark = pytest.mark.gpu
EXE = os.path.join(R.HERE, "_build", "ec_quad_unit")
RESULTS = ("P + Q", "(-P) + Q", "D after 1 step", "D after 2 steps", "D after 64 steps")


@pytest.mark.parametrize("group,name", [(11, "secp256k1"), (12, "ristretto255"), (13, "secp256k1")],
                         ids=["QuadSecp", "QuadRist", "OctSecp"])
def test_lane_parallel_addition_on_weak_operands(tmp_path, group, name):
    rc = R.repr_cases(name)
    n, L = len(rc.cases), rc.L
    assert n > 16 and n % 16 != 0 and n % 8 != 0            # several workgroups, the last one partly filled
    got = R.run_unit(EXE, group, b"".join(R.words(c.P) + R.words(c.Q) for c in rc.cases), n, tmp_path)
    assert len(got) == n * 5 * L
    for i, case in enumerate(rc.cases):
        a, b = case.a, case.b
        for r, k in enumerate((a + b, b - a, a + b, a + 2 * b, a + 64 * b)):
            assert got[(i * 5 + r) * L:(i * 5 + r + 1) * L] == rc.enc(k), (RESULTS[r], case.tag)
