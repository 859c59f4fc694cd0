"""The forward-difference X path of the run-time MODP groups at its edges: the largest workgroups of every width, degenerate
polynomials, roots inside the run, chain geometries without steps, first positions up to 2^63 - n and around q - 1, moduli on the
limb-count boundaries, state kept in the context between calls, whole boxes, and calls whose chunks take different paths.

tests/test_gpu_modp_rt_fd.py sends random unit commitments from small first positions through k_rt_commit_eval_mont,
k_rt_fd_chain and k_rt_from_mont; tests/modp_rt_fd_edge_child.py holds the cases here and their references (mode 2 against mode 0
byte for byte at all positions, Python integers at the positions each case fixes).  One child process per width -- the contexts
and their workspaces are the child's own -- and one with MPVSS_MAX_CHUNK=64, which is read once per process.  Here: every child
ends well and reports every case of build_cases() with the path the host gate owes it."""
import os
import signal
import subprocess
import sys
import time

import pytest

import modp_rt_fd_edge_child as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on an MI355X: 5: 4.1 s, 9: 4.4 s, 18: 11.1 s, 27: 14.7 s, chunks: 3.2 s per child (42.7 s for the module; 10.4 s and 12.3 s
# for 18 and 27 within the whole suite, since family B's powers of 4 go through fixed-base rows; most
# of the wide children is Python's integers: 484 positions of the clamped 241-chain case, the products of a non-unit case, and
# torch's import and the engine's start in every child).  The slowest is below the 20 s from which family C would be thinned.  The
# limit, twenty times the slowest, only has to end a child that hangs, and leaves room for a loaded machine.
CHILD_TIMEOUT = 300
_DONE = {}            # child -> {case id: (sha256, path)}
_FAILED = {}          # child -> why it failed: it is not started a second time
_TROUBLE = []         # a child that ended by signal, by abort, with a HIP fault or at its time limit: nothing more is started
HIP_FAULTS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure", "unspecified launch failure",
              "Segmentation fault", "Aborted", "core dumped")


def child(width):
    if _TROUBLE:
        pytest.fail(f"not started: {_TROUBLE[0]}")
    if width in _FAILED:
        pytest.fail(f"not started again: {_FAILED[width]}")
    if width in _DONE:
        return _DONE[width]
    cmd = [sys.executable, os.path.join(ROOT, "tests", "modp_rt_fd_edge_child.py"), width]
    env = dict(os.environ)
    env.pop("MPVSS_MAX_CHUNK", None)
    if width == "chunks":
        env["MPVSS_MAX_CHUNK"] = str(K.CHUNK)
    t0 = time.time()
    # a session of its own: at the time limit whatever the child started ends with it
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        stdout, stderr = proc.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        stdout, stderr = proc.communicate()
        _TROUBLE.append(f"the {width} child did not end within {CHILD_TIMEOUT} s")
        pytest.fail(_TROUBLE[0] + "\n" + stdout[-1500:] + stderr[-3000:])
    rc = proc.returncode
    if rc < 0 or rc in (134, 139, 124, 137) or any(f in stderr for f in HIP_FAULTS):
        _TROUBLE.append(f"the {width} child ended with status {rc}" + (" and a GPU fault in its output" if rc in (0, 1) else ""))
        pytest.fail(_TROUBLE[0] + "\n" + stdout[-1500:] + stderr[-3000:])
    print(f"{width} child: {time.time() - t0:.1f} s")
    if rc != 0 or f"modp rt fd edges {width} ok" not in stdout:
        _FAILED[width] = f"the {width} child failed with status {rc}"
        pytest.fail(_FAILED[width] + "\n" + stdout[-1500:] + stderr[-3000:])
    res = {}
    for line in stdout.splitlines():
        w = line.split()
        if w and w[0] == "case":
            assert len(w) == 4 and len(w[2]) == 64 and w[1] not in res, line
            res[w[1]] = (w[2], w[3])
    _DONE[width] = res
    return res


@pytest.mark.parametrize("width", K.WIDTHS)
def test_every_case_of_a_width_equals_horner_and_python_integers(width):
    """the child has compared every case under mode 2 with mode 0 at all positions and with Python integers at the case's own;
    it took the path the host gate owes the case"""
    res = child(width)
    want = K.expected(width)
    assert set(want) <= set(res), sorted(set(want) - set(res))[:8]
    wrong = {cid: (res[cid][1], path) for cid, path in want.items() if res[cid][1] != path}
    assert not wrong, wrong


def test_the_largest_workgroup_of_every_width_ran_by_forward_differences():
    """t = fd_max_t (256 / 256 / 256 / 128 levels: 16, 16, 16 and 8 waves in one workgroup) on every modulus of every width"""
    for width in K.WIDTHS:
        res = child(width)
        ids = [c.id for c in K.build_cases(width) if c.id.startswith("C-tmax-")]
        assert len(ids) >= 3 and all(c.t == K.FD_MAX_T[int(width)] for c in K.build_cases(width) if c.id in ids)
        for cid in ids + (["E-1-tmax"] if width in ("18", "27") else []):
            assert cid in res and res[cid][1] == "fd", (width, cid, res.get(cid))


def test_chunks_of_one_call_on_different_paths():
    """MPVSS_MAX_CHUNK=64: a last chunk below t takes Horner after chunks by forward differences; chunks of exactly t positions
    are seeds only; t above the chunk leaves the whole call to Horner"""
    res = child("chunks")
    want = K.expected("chunks")
    assert set(want) == set(res)
    assert {cid: path for cid, (_, path) in res.items()} == want
    assert res["chunks-n133-t7-verify"][1] == "fd=2,horner=1"
