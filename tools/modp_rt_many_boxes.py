#!/usr/bin/env python3
"""Run-time MODP groups: the boxes of one round through ONE mpvss_modp_group_verify_many call, against the loop of
mpvss_modp_group_verify_distribution (or _keyset) calls over the same boxes -- the only way there was before.  One GPU, warm
context, group_prepare done; both sides go straight to the C ABI over buffers made once; every figure is the median of REPS
repetitions after one warm-up.  The results of the two sides are compared before anything is printed.

    python tools/modp_rt_many_boxes.py > profiles/modp_rt_many_boxes.txt"""
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):      # modp_rt_helpers: the RFC primes
    sys.path.insert(0, _p)
import torch  # noqa: E402
from mpvss_rs_amd import Engine, ModpGroup, capi  # noqa: E402
import modp_rt_helpers as H  # noqa: E402

REPS = 3
SHAPES = ((5, 3, 400), (100, 34, 200), (1024, 32, 60))      # n, t, boxes
DISTINCT = 8                                                  # boxes dealt per shape, taken in turn

eng = Engine(0)
EB = 256
cat = lambda vals: b"".join(v.to_bytes(EB, "big") for v in vals)


def median_ms(fn):
    fn()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3


print(f"# {torch.cuda.get_device_name(0)}; median of {REPS} after one warm-up; ms for all boxes of the call")
print("# bits  n     t   boxes space  keys    loop_ms   many_ms  speedup  groups grouped single")
for bits in (1024, 2048):
    q = H.rfc_prime(bits)
    grp = ModpGroup(q)
    eng.group_prepare(grp)
    rng = random.Random(bits)
    for n, t, K in SHAPES:
        pos = list(range(1, n + 1))
        pks = cat([rng.randrange(2, q) for _ in range(n)])
        dealt = []
        for _ in range(DISTINCT):
            co, ws = cat([rng.randrange(1, q - 1) for _ in range(t)]), cat([rng.randrange(1, q - 1) for _ in range(n)])
            d = eng.group_deal(grp, co, pos, pks, ws)
            dealt.append(dict(commitments=eng.group_batch_exp_fixed_base(grp, cat([4]), co), shares=d["Y"], responses=d["responses"],
                              challenge=d["challenge"], digest=d["digest"]))
        ks = eng.group_keyset_create(grp, pks)
        posb = (C.c_int64 * n)(*pos)
        for space in (capi.MPVSS_HOST, capi.MPVSS_DEVICE):
            keep = []

            def place(b):
                if space == capi.MPVSS_HOST:
                    arr = (C.c_uint8 * len(b)).from_buffer_copy(b)
                    keep.append(arr)
                    return C.addressof(arr)
                tns = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
                keep.append(tns)
                return tns.data_ptr()

            if space == capi.MPVSS_HOST:
                ppos = C.addressof(posb)
            else:
                tpos = torch.tensor(pos, dtype=torch.int64).cuda()
                keep.append(tpos)
                ppos = tpos.data_ptr()
            ppk = place(pks)
            ptrs = []
            for b in dealt:
                ch = (C.c_uint8 * EB).from_buffer_copy(b["challenge"])
                keep.append(ch)
                ptrs.append((place(b["commitments"]), place(b["shares"]), place(b["responses"]), C.addressof(ch)))
            torch.cuda.synchronize()
            for keyed in (False, True):
                arr = (capi.GroupBox * K)()
                for i in range(K):
                    pc, pY, pr, pch = ptrs[i % DISTINCT]
                    arr[i] = capi.GroupBox(pc, t, ppos, None if keyed else ppk, pY, pr, n, pch, ks.handle if keyed else None, 0)
                v_many, d_many = (C.c_int * K)(), (C.c_uint8 * (32 * K))()
                v_loop, d_loop = (C.c_int * K)(), (C.c_uint8 * (32 * K))()

                def many():
                    eng._check(eng.lib.mpvss_modp_group_verify_many(eng.ctx, grp.handle, space, arr, K, 0, v_many, C.cast(d_many, C.c_void_p)),
                               "group_verify_many")

                def loop():
                    one = C.c_int(0)
                    for i in range(K):
                        b = arr[i]
                        dig = C.c_void_p(C.addressof(d_loop) + 32 * i)
                        if keyed:
                            rc = eng.lib.mpvss_modp_group_verify_distribution_keyset(
                                eng.ctx, grp.handle, space, b.commitments, t, b.positions, ks.handle, 0, b.shares, b.responses, n,
                                b.challenge_host, C.byref(one), dig, None, None, None)
                        else:
                            rc = eng.lib.mpvss_modp_group_verify_distribution(
                                eng.ctx, grp.handle, space, b.commitments, t, b.positions, b.pubkeys, b.shares, b.responses, n,
                                b.challenge_host, C.byref(one), dig, None, None, None)
                        eng._check(rc, "group_verify_distribution")
                        v_loop[i] = one.value
                s0 = eng.group_verify_many_stats()
                many()
                s1 = eng.group_verify_many_stats()
                loop()
                assert list(v_many) == list(v_loop) == [1] * K and bytes(d_many) == bytes(d_loop)
                assert all(bytes(d_many)[32 * i:32 * i + 32] == dealt[i % DISTINCT]["digest"] for i in range(K))
                t_loop, t_many = median_ms(loop), median_ms(many)
                print(f"  {bits:4d} {n:5d} {t:3d} {K:5d} {'host' if space == capi.MPVSS_HOST else 'device':6s} {'keyset' if keyed else 'arrays':6s} "
                      f"{t_loop:9.2f} {t_many:9.2f} {t_loop / t_many:8.2f} {s1['groups'] - s0['groups']:6d} "
                      f"{s1['grouped_boxes'] - s0['grouped_boxes']:7d} {s1['single_boxes'] - s0['single_boxes']:6d}", flush=True)
        ks.close()
eng.close()
