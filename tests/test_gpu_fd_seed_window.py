"""Two-level seeding of the forward-difference X path with the Horner seeds in the MIDDLE of the seed window (eval_x in
mpvss_capi.cpp): the stride-1 chain steps forward and backward from positions w1 .. w1 + t - 1 of the window's m0 = S t, with
w1 = (m0 - t) / 2.  Every X must be Horner's, bit for bit, at the smallest shapes where that index arithmetic can go wrong; the
integer model of the same arithmetic is tests/test_fd_seed_window_model.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (t, n, first position, statement that doctors the commitments)
CASES = [(16, 256, 1, ""),                    # S = 4, m0 = 64: the minimum
         (17, 300, 777, ""),                  # m0 - t odd, ragged chains
         (33, 16 * 33, 5, ""),                # n = 16 t exactly
         (16, 131072, 1, ""),                 # S = 16
         (64, 2048, 1 << 40, ""),             # wide positions
         (256, 8192, 1, ""),                  # the headline's t at its smallest n
         (64, 1100, 1, "cm[5] = 0"),          # degenerate commitments reach the gate and fall back
         (64, 1100, 1, "cm[0] = Q"),
         (64, 2048, 1, "")]                   # the shape of the fault-injection child below
FD_ENV = {"MPVSS_FD": "1", "MPVSS_FD_L1": "2", "MPVSS_FD_MIN_SHARES": "256"}

# one process evaluates every case (importing torch and creating the context once) and prints one hash per case
CODE = r'''
%s
import os, sys, random, hashlib
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import mpvss_oracle as O
from helpers import modp_fast_share
from mpvss_rs_amd import Engine
G = O.ModpGroup(); Q = G.q
fx = lambda v: v.to_bytes(256, "big")
eng = Engine(0)
for t, n, p0, extra in %r:
    rng = random.Random(t * 1000 + n)
    raw = eng.batch_exp_fixed_base(fx(4), b"".join(fx(rng.randrange(Q - 1)) for _ in range(t)))
    cm = [int.from_bytes(raw[k * 256:(k + 1) * 256], "big") for k in range(t)]
    exec(extra)
    pos = list(range(p0, p0 + n))
    cmb = b"".join(map(fx, cm))
    out = eng.commit_eval(cmb, pos)
    for i in ((0, t, n - 1) if os.environ.get("CHECK_ORACLE") else ()):
        got = out[i * 256:(i + 1) * 256]
        if t < 100:
            assert int.from_bytes(got, "big") == O.commitment_eval(G, cm, pos[i]), (t, n, i)
        else:
            assert got == modp_fast_share((cmb, pos[i], fx(1), fx(1), fx(0), fx(0)))[0], (t, n, i)
    print(hashlib.sha256(out).hexdigest())
'''

# boxes dealt by the engine (its dealer computes X_i = g^P(i) through the comb: no forward differences), verified in one process
BOXES = r'''
def sc(rng, k):
    return b"".join(rng.randrange(1, 1 << 2040).to_bytes(256, "big") for _ in range(k))

def dealt(rng, n, t, first, pk):
    pos = list(range(first, first + n))
    coeffs = sc(rng, t)
    d = eng.deal(coeffs, pos, pk, sc(rng, n))
    return dict(commitments=eng.batch_exp_fixed_base(fx(4), coeffs), positions=pos, pubkeys=pk, shares=d["Y"], responses=d["responses"],
                challenge=d["challenge"], digest=d["digest"])
'''

# MPVSS_FD_TEST_FAULT=3: a stage of the stride-1 seeding chain gives up; the X of a commit_eval and of one verified box are Horner's
FAULT = BOXES + r'''
rng = random.Random(64 * 2048)
box = dealt(rng, 2048, 64, 1, eng.batch_exp_fixed_base(fx(2), sc(rng, 2048)))
before = eng.fd_stats()
res = eng.verify_distribution(box["commitments"], box["positions"], box["pubkeys"], box["shares"], box["responses"], box["challenge"])
after = eng.fd_stats()
assert res["verdict"] is True and res["digest"] == box["digest"], "verdict / digest after the fall-back"
print("fd_stats", after[0] - before[0], after[1] - before[1])
'''

# three (300, 17) boxes of three dealers against ONE key array in HBM in one mpvss_modp_verify_many call (the grouped form: the box is
# the launches' second grid dimension), then each box in a call of its own
GROUP = BOXES + r'''
import ctypes as C
from mpvss_rs_amd import capi
rng = random.Random(300 * 17)
n, t = 300, 17
pk = eng.batch_exp_fixed_base(fx(2), sc(rng, n))
boxes = [dealt(rng, n, t, 5, pk) for _ in range(3)]
keep = []
def dev(b):
    keep.append(torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0"))
    return keep[-1].data_ptr()
d_pk = dev(pk)
keep.append(torch.tensor(boxes[0]["positions"], dtype=torch.int64, device="cuda:0"))
d_pos = keep[-1].data_ptr()
def array(bs):
    arr = (capi.ModpBox * len(bs))()
    for i, b in enumerate(bs):
        ch = (C.c_uint8 * 256).from_buffer_copy(b["challenge"]); keep.append(ch)
        arr[i] = capi.ModpBox(dev(b["commitments"]), t, d_pos, d_pk, dev(b["shares"]), dev(b["responses"]), n, C.cast(ch, C.c_void_p), None, 0)
    torch.cuda.synchronize()
    return arr
def run(bs):
    arr, k = array(bs), len(bs)
    verdicts, digests = (C.c_int * k)(), (C.c_uint8 * (32 * k))()
    eng._check(eng.lib.mpvss_modp_verify_many(eng.ctx, capi.MPVSS_DEVICE, arr, k, 4, 3, verdicts, C.cast(digests, C.c_void_p)), "verify_many")
    raw = bytes(digests)
    return [(bool(verdicts[i]), raw[32 * i:32 * i + 32]) for i in range(k)]
before = eng.fd_stats()
together = run(boxes)
alone = [run([b])[0] for b in boxes]
after = eng.fd_stats()
assert together == alone, "grouped call against one-box calls"
assert together == [(True, b["digest"]) for b in boxes], "verdicts / dealers' digests"
assert after[0] > before[0] and after[1] == before[1], ("forward differences used and held", before, after)
print("group ok")
'''


def run(cases, env_extra, tail="", first=""):
    # first: torch ships its own HIP runtime and must be loaded before the engine's library when the process uses both
    code = CODE % (first, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), cases) + tail
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env_extra), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def horner():
    return run(CASES, {"MPVSS_FD": "0"})


@pytest.fixture(scope="module")
def stepped():
    """every case with the two-level seeding forced, three positions of each against the oracle, then the grouped call"""
    return run(CASES, dict(FD_ENV, CHECK_ORACLE="1"), GROUP, "import torch")


def test_seed_window_from_its_middle_equals_horner(horner, stepped):
    assert len(horner) == len(CASES) and len(stepped) == len(CASES) + 1 and all(len(h) == 64 for h in horner)
    for case, a, b in zip(CASES, stepped, horner):
        assert a == b, case


def test_grouped_boxes_take_the_same_seeding(stepped):
    assert stepped[-1] == "group ok"


def test_seeding_stage_that_gives_up_falls_back_to_horner(horner):
    out = run([(64, 2048, 1, "")], dict(FD_ENV, MPVSS_FD_TEST_FAULT="3"), FAULT)
    assert out[0] == horner[CASES.index((64, 2048, 1, ""))]
    assert out[1] == "fd_stats 1 1"
