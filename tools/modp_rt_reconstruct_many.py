#!/usr/bin/env python3
"""Run-time MODP groups: the secrets of one round through ONE mpvss_modp_group_reconstruct_many call, against the loop of
mpvss_modp_group_reconstruct calls over the same secrets -- the only way there was before.  One GPU, warm context, group_prepare
done; both sides go straight to the C ABI over buffers made once; every figure is the median of REPS repetitions after one
warm-up.  The results of the two sides are compared before anything is printed.  Every shape runs once with the same position
list for all its secrets and once with a list of its own for each, so that the share of the Lagrange cache shows.

    python tools/modp_rt_reconstruct_many.py > profiles/modp_rt_reconstruct_many.txt
    python tools/modp_rt_reconstruct_many.py --bits 2048 --shapes 3 --spaces host      (a part of the table: shape 3 is 60 x 1024)"""
import argparse
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
SHAPES = ((400, 3), (200, 34), (60, 32), (60, 1024))        # secrets, m
POOL = 2048                                                   # shares made per group; a secret takes m consecutive ones

ap = argparse.ArgumentParser()
ap.add_argument("--bits", default="1024,2048")
ap.add_argument("--shapes", default="0,1,2,3")
ap.add_argument("--spaces", default="host,device")
args = ap.parse_args()

eng = Engine(0)
EB = 256


def median_ms(fn):
    fn()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3


print(f"# {torch.cuda.get_device_name(0)}; median of {REPS} after one warm-up; ms for all secrets of the call")
print("# bits secrets    m space  lists      loop_ms   many_ms  speedup  passes grouped single", flush=True)
for bits in (int(b) for b in args.bits.split(",")):
    q = H.rfc_prime(bits)
    grp = ModpGroup(q)
    eng.group_prepare(grp)
    rng = random.Random(bits)
    pool = eng.group_batch_exp_fixed_base(grp, (4).to_bytes(EB, "big"), b"".join(rng.randrange(1, q - 1).to_bytes(EB, "big") for _ in range(POOL)))
    host_pool = (C.c_uint8 * len(pool)).from_buffer_copy(pool)
    dev_pool = torch.frombuffer(bytearray(pool), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for K, m in (SHAPES[int(s)] for s in args.shapes.split(",")):
        for space in (dict(host=capi.MPVSS_HOST, device=capi.MPVSS_DEVICE)[s] for s in args.spaces.split(",")):
            base = C.addressof(host_pool) if space == capi.MPVSS_HOST else dev_pool.data_ptr()
            for lists in ("equal", "distinct"):
                pos = [(C.c_int64 * m)(*range(1 + (i if lists == "distinct" else 0), m + 1 + (i if lists == "distinct" else 0)))
                       for i in range(K)]
                arr = (capi.GroupSecret * K)()
                for i in range(K):
                    arr[i] = capi.GroupSecret(C.addressof(pos[i]), base + ((i * m) % (POOL - m + 1)) * EB, m)
                st = (C.c_int * K)()
                g_many, m_many = (C.c_uint8 * (EB * K))(), (C.c_uint8 * (32 * K))()
                g_loop, m_loop = (C.c_uint8 * (EB * K))(), (C.c_uint8 * (32 * K))()

                def many():
                    eng._check(eng.lib.mpvss_modp_group_reconstruct_many(eng.ctx, grp.handle, space, arr, K, 0, st, C.cast(g_many, C.c_void_p),
                                                                         C.cast(m_many, C.c_void_p)), "group_reconstruct_many")

                def loop():
                    for i in range(K):
                        s = arr[i]
                        eng._check(eng.lib.mpvss_modp_group_reconstruct(eng.ctx, grp.handle, space, s.positions_host, s.shares, m,
                                                                        C.c_void_p(C.addressof(g_loop) + EB * i),
                                                                        C.c_void_p(C.addressof(m_loop) + 32 * i)), "group_reconstruct")

                s0 = eng.group_reconstruct_many_stats()
                t_many = median_ms(many)
                s1 = eng.group_reconstruct_many_stats()
                t_loop = median_ms(loop)
                assert list(st) == [0] * K and bytes(g_many) == bytes(g_loop) and bytes(m_many) == bytes(m_loop)
                assert len({bytes(g_many)[EB * i:EB * i + EB] for i in range(K)}) > 1
                calls = REPS + 1
                print(f"  {bits:4d} {K:7d} {m:4d} {'host' if space == capi.MPVSS_HOST else 'device':6s} {lists:8s} "
                      f"{t_loop:9.2f} {t_many:9.2f} {t_loop / t_many:8.2f} {(s1['passes'] - s0['passes']) // calls:7d} "
                      f"{(s1['grouped_secrets'] - s0['grouped_secrets']) // calls:7d} "
                      f"{(s1['single_secrets'] - s0['single_secrets']) // calls:6d}", flush=True)
    assert dev_pool.cpu().numpy().tobytes() == pool, "the share pool in HBM changed"
eng.close()
