"""The curve groups' forward-difference X path on degenerate polynomials, hostile first positions and the edges of its shape rule.

tests/test_gpu_ec_fd.py sends random commitments from small first positions through the stepping variants; here the identity -- the
value the group law treats specially -- goes through the difference tables, the stepping recurrences (one workgroup per chain, the
quad-lane pipelines of ec_quad.h, the two-level seeding chain), the tagged words between pipeline stages and Secp::encode_batch:
zero coefficients, polynomials of lower degree (whole levels of the table are the identity), roots inside the run (X_i is the
identity and the steps around it are P + (-P) and 0 + P), +-C and all-equal commitments; runs that cross 2^32, start at 2^61 - 1
(the last admissible first position), at 2^61 and below zero; (t, n) on both sides of every bound of ec_fd_shape; t = 17 and 33.

tests/ec_fd_edge_child.py holds the cases and the references (P(i) G through the fixed-base comb for ALL positions, the oracle's
commitment_eval on up to 24 of them); one child process per configuration, because the switches are read once per process.  Here:
every child ends well, and every case's bytes are the same in every configuration as under Horner's rule."""
import os
import signal
import subprocess
import sys
import time

import pytest

import ec_fd_edge_child as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on an MI355X: horner 4.9 s, quad 4.8 s, quad-l1 3.2 s, chain-l1 3.7 s per child (16.7 s for the module; much of a child is
# torch's import, the engine's start and the oracle's workers).  The limit, 24 times the slowest, only has to end a child that hangs
# and leaves room for a loaded machine.
CHILD_TIMEOUT = 120
_DONE = {}            # configuration -> {(curve, case id): (sha256, fd counters)}
_FAILED = {}          # configuration -> why its child failed: it is not started a second time
_TROUBLE = []         # a child that ended by signal, by abort, with a HIP fault or at its time limit: nothing more is started
HIP_FAULTS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure", "unspecified launch failure",
              "Segmentation fault", "Aborted", "core dumped")


def child(config):
    if _TROUBLE:
        pytest.fail(f"not started: {_TROUBLE[0]}")
    if config in _FAILED:
        pytest.fail(f"not started again: {_FAILED[config]}")
    if config in _DONE:
        return _DONE[config]
    cmd = [sys.executable, os.path.join(ROOT, "tests", "ec_fd_edge_child.py"), config]
    t0 = time.time()
    # a session of its own: at the time limit the child's oracle workers end with it
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, **K.CONFIGS[config]),
                            start_new_session=True)
    try:
        stdout, stderr = proc.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        stdout, stderr = proc.communicate()
        _TROUBLE.append(f"the {config} child did not end within {CHILD_TIMEOUT} s")
        pytest.fail(_TROUBLE[0] + "\n" + stdout[-1500:] + stderr[-3000:])
    rc = proc.returncode
    if rc < 0 or rc in (134, 139, 124, 137) or any(f in stderr for f in HIP_FAULTS):
        _TROUBLE.append(f"the {config} child ended with status {rc}" + (" and a GPU fault in its output" if rc in (0, 1) else ""))
        pytest.fail(_TROUBLE[0] + "\n" + stdout[-1500:] + stderr[-3000:])
    print(f"{config} child: {time.time() - t0:.1f} s")
    if rc != 0 or f"ec fd edges {config} ok" not in stdout:
        _FAILED[config] = f"the {config} child failed with status {rc}"
        pytest.fail(_FAILED[config] + "\n" + stdout[-1500:] + stderr[-3000:])
    res = {}
    for line in stdout.splitlines():
        w = line.split()
        if w and w[0] == "case":
            assert len(w) == 5 and len(w[3]) == 64 and (w[1], w[2]) not in res, line
            res[(w[1], w[2])] = (w[3], w[4])
    _DONE[config] = res
    return res


def x_cases():
    return [(curve, c.id) for curve in K.CURVES for c in K.build_cases(curve)]


def test_horner_child_every_case_against_the_comb_and_the_oracle():
    """MPVSS_EC_FD=0: Horner's rule (small_scalar_mul with the position's bit length) for every case, whole boxes included"""
    res = child("horner")
    assert set(x_cases()) <= set(res)
    assert all(fd == "fd=0,0" for _, fd in res.values())


@pytest.mark.parametrize("config", ["quad", "quad-l1", "chain-l1"])
def test_forward_differences_on_degenerate_polynomials_equal_horner(config):
    """every case of the child (it has compared them with the comb; `quad` with the oracle too) has the bytes Horner's rule gave;
    where the quad-lane pipelines run (MPVSS_EC_FD_QUAD=2) every verifier's box was counted as one forward-difference block that
    held -- the only evidence that the pipelines computed the bytes and did not leave them to the gated Horner launch."""
    base = child("horner")
    res = child(config)
    assert set(x_cases()) <= set(res)
    for key, (sha, fd) in res.items():
        if key in base:
            assert sha == base[key][0], (config, key)
        else:
            assert key[1] in ("many", "many-tampered") and config in ("quad", "chain-l1"), key
        if key[1].startswith("box-"):
            assert fd == ("fd=1,0" if config.startswith("quad") else "fd=0,0"), (config, key, fd)
        if key[1].startswith("many"):
            assert fd == ("fd=4,0" if config == "quad" else "fd=0,0"), (config, key, fd)
    for curve in K.CURVES:
        assert {(curve, "box-" + c) for c in K.BOX_CASES} <= set(res)
        if config in ("quad", "chain-l1"):
            assert {(curve, "many"), (curve, "many-tampered")} <= set(res)
    if config == "chain-l1":       # the batched X paths of both configurations agree
        quad = child("quad")
        for curve in K.CURVES:
            for what in ("many", "many-tampered"):
                assert res[(curve, what)][0] == quad[(curve, what)][0], (curve, what)
