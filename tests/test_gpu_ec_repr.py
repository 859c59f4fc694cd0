"""The one-lane point formulas of ec_curves.h on weakly reduced operands, on the device: tests/ec_repr_unit.hip runs the body
of tests/ec_repr_ops.h (the one tests/test_ec_repr_host.py runs on the CPU) on every case of tests/ec_repr_cases.py, one
case per lane; every encoding is compared byte for byte with oracle/ec_ref.c's."""
import os

import pytest

import ec_repr_cases as R

pytestmark = pytest.mark.gpu
EXE = os.path.join(R.HERE, "_build", "ec_repr_unit")


@pytest.mark.parametrize("mode,name", [(1, "secp256k1"), (2, "ristretto255")])
def test_point_formulas_on_weak_operands(tmp_path, mode, name):
    """add, dbl, neg, add_affine and add_cached with both signs, cmov, encode, ks_is_identity and 64 steps of acc += Q /
    acc = 2 acc: more than one workgroup, the last one partly filled"""
    rc = R.repr_cases(name)
    n, stride = len(rc.cases), 11 * rc.L
    assert n > 64 and n % 64 != 0
    got = R.run_unit(EXE, mode, b"".join(R.words(c.P) + R.words(c.Q) for c in rc.cases), n, tmp_path)
    assert len(got) == n * stride
    for i, case in enumerate(rc.cases):
        for s, want in enumerate(R.expected_slots(rc, case)):
            assert got[i * stride + s * rc.L:i * stride + (s + 1) * rc.L] == want, (R.SLOT_NAMES[s], case.tag)


def test_secp256k1_batched_encoding_with_weak_and_vanishing_z(tmp_path):
    """encode_batch<8>: a weak-Z point, an identity written with a non-zero zero (first, last, in the middle) and ordinary
    points share one inversion"""
    rc = R.repr_cases("secp256k1")
    batches = rc.batches()
    got = R.run_unit(EXE, 3, b"".join(R.words(pt) for _, row in batches for _, pt in row), len(batches), tmp_path)
    assert len(got) == len(batches) * 8 * 33
    for i, (tag, row) in enumerate(batches):
        assert got[i * 264:(i + 1) * 264] == b"".join(rc.enc(k) for k, _ in row), tag
