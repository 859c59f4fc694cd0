"""One block slot meets both plans of the forward-difference X path (fdplan::plan in host_fd_plan.h, followed by eval_x in
mpvss_capi.cpp): a box that has the GPU to itself and a box among others differ in chains and seeding levels, and the workspace is
sized for both at once (fdplan::sized).  Shape t = 16, n = 1024 with MPVSS_FD_MIN_SHARES=256 on one Engine:

  1. a lone verify_distribution: 16 chains, Horner's rule for all 256 seeds (one seeding level);
  2. verify_block_compute calls back to back, then their absorbs.  A block is among others when at least two are in flight ahead of
     it (mpvss_ctx::busy_with_others), so it takes three calls for one of them to be: the third gets 4 chains and two-level seeding
     with m0 = 64;
  3. one more lone call -- in the slot the box among others has just left (the most recently released slot is taken first).

Every X, a1 and a2, the verdict and the digest are the oracle's: the reference's operation order for every share (oracle/modp_ref.c
on threads: 20 exponentiations per share), its transcript and verdict rule (oracle/mpvss_oracle.py), computed once.  fd_stats counts
every block on the forward-difference path and no fall-back.  The plans themselves (chains, m0, levels at this shape) are pinned on
the CPU by tests/test_fd_plan_host.py.  The box is dealt by the engine's dealer, whose X_i = g^P(i) come from the comb."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import concurrent.futures, hashlib, random, sys
[sys.path.insert(0, p) for p in %r]
import mpvss_oracle as O
from helpers import worker_count
from modp_ref import ModpRef
from mpvss_rs_amd import Engine, capi
n, t, EB = 1024, 16, 256
g = O.ModpGroup()
rng = random.Random(n * t)
fx = lambda v: v.to_bytes(EB, "big")
sc = lambda k: b"".join(fx(rng.randrange(1, 1 << 2040)) for _ in range(k))
row = lambda b, i: b[i * EB:(i + 1) * EB]
eng = Engine(0)
pos = list(range(1, n + 1))
pk, coeffs = eng.batch_exp_fixed_base(fx(2), sc(n)), sc(t)
d = eng.deal(coeffs, pos, pk, sc(n))
cm = eng.batch_exp_fixed_base(fx(4), coeffs)
args = (cm, pos, pk, d["Y"], d["responses"], d["challenge"])

ref = ModpRef()
with concurrent.futures.ThreadPoolExecutor(max_workers=worker_count(16)) as ex:      # ctypes releases the GIL
    work = list(ex.map(lambda i: ref.share_work(cm, pos[i], row(pk, i), row(d["Y"], i), row(d["responses"], i), d["challenge"]), range(n)))
h = hashlib.sha256()
for i, (x, a1, a2) in enumerate(work):
    h.update(O.append_transcript(g, *(int.from_bytes(v, "big") for v in (x, row(d["Y"], i), a1, a2))))
verdict = g.hash_to_scalar(h.digest()) == int.from_bytes(d["challenge"], "big")
want = (verdict, h.digest()) + tuple(b"".join(w[k] for w in work) for k in range(3))
assert verdict is True, "the oracle accepts the dealt box"

def lone(step):
    assert eng.blocks_in_flight() == (0, 0)
    r = eng.verify_distribution(*args, dump=True)
    assert (r["verdict"], r["digest"], r["X"], r["a1"], r["a2"]) == want, step

f0 = eng.fd_stats()
lone("first lone call")
blocks = 3
for _ in range(blocks):
    eng.verify_block_compute(*args)
for k in range(blocks):
    st, X, a1, a2 = eng.verify_block_absorb_dump(capi.transcript_init(), n)
    assert tuple(capi.transcript_verdict(st, d["challenge"])) + (X, a1, a2) == want, ("block", k)
lone("lone call after the blocks")
f1 = eng.fd_stats()
eng.close()
print("fd", f1[0] - f0[0], f1[1] - f0[1])
'''


def test_a_slot_meets_the_lone_and_the_busy_plan():
    code = CHILD % [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MPVSS_FD_MIN_SHARES="256"))
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    # two lone calls and three blocks on the forward-difference path, none fell back
    assert out.stdout.strip().split("\n")[-1] == "fd 5 0"
