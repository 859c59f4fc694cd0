#!/usr/bin/env python3
"""Curve groups: the secrets of one round through ONE mpvss_ec_reconstruct_many call, against the loop of mpvss_ec_reconstruct
calls over the same secrets -- the only way there was before.  One GPU, warm context; both sides go straight to the C ABI over
buffers made once; every figure is the median of REPS repetitions after one warm-up, and the spread (min .. max) of the loop's
repetitions stands beside it.  The results of the two sides are compared before anything is printed.  Every shape runs once with
the same position list for all its secrets and once with a list of its own for each, so that the share of the Lagrange cache shows.

    python tools/ec_reconstruct_many.py > profiles/ec_reconstruct_many.txt
    python tools/ec_reconstruct_many.py --curves secp256k1 --shapes 3 --spaces host --lists equal   (a part of the table: shape 3 is 8 x 16384)

--lagrange {host,device,auto} sets where the Lagrange coefficients are computed (mpvss_ctx_set_ec_lagrange; a library of an older
commit, MPVSS_HIP_LIB, has no such switch and is reported as "parent").  --no-loop leaves the loop of one-secret calls out -- at
16384 shares with a list per secret it takes minutes on the host -- and prints a digest of the call's results instead, so that
runs of different builds and modes can be compared line by line (profiles/ec_lagrange_device.txt).  Shapes 4 to 7 are 60 x 4096
and ONE secret of 1024, 4096 and 16384 shares: a call of one secret is the one-secret path, mpvss_ec_reconstruct."""
import argparse
import ctypes as C
import hashlib
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mpvss_rs_amd import Engine, capi  # noqa: E402

REPS = 3
SHAPES = ((400, 3), (200, 34), (60, 1024), (8, 16384), (60, 4096), (1, 1024), (1, 4096), (1, 16384))       # secrets, m
POOL = 16384 + 512                                           # shares made per curve; a secret takes m consecutive ones
GID = {"secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}
ORDER = {"secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
         "ristretto255": 2 ** 252 + 27742317777372353535851937790883648493}

ap = argparse.ArgumentParser()
ap.add_argument("--curves", default="secp256k1,ristretto255")
ap.add_argument("--shapes", default="0,1,2")
ap.add_argument("--spaces", default="host,device")
ap.add_argument("--lists", default="equal,distinct")
ap.add_argument("--lagrange", choices=("host", "device", "auto"), default=None)
ap.add_argument("--no-loop", action="store_true")
args = ap.parse_args()

eng = Engine(0)
HAS_MODE = hasattr(eng.lib, "mpvss_ec_lagrange_scalars")
MODE = (args.lagrange or "auto") if HAS_MODE else "parent"
if HAS_MODE and args.lagrange:
    eng.set_ec_lagrange(("host", "auto", "device").index(args.lagrange))
eng.lib.mpvss_last_kernel_ms.restype = C.c_double


def timed(fn):
    """(median, min, max) in ms of REPS repetitions after one warm-up"""
    fn()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
        print(f"    ... {times[-1]:.1f} ms", file=sys.stderr, flush=True)
    return statistics.median(times), min(times), max(times)


print(f"# {torch.cuda.get_device_name(0)}; median of {REPS} after one warm-up; ms for all secrets of the call; loop_min / loop_max: the spread of the loop's {REPS} runs")
print("# lagrange: where the coefficients are computed; dev_l / host_l: position lists per call computed on either side; k_ms: k_ec_lagrange's own time in the last call (hipEvents)")
print("# curve        secrets     m space  lists      loop_ms  loop_min  loop_max   many_ms  many_min  many_max  speedup  passes grouped single lagrange  dev_l host_l    k_ms  digest",
      flush=True)
for curve in args.curves.split(","):
    group, L = GID[curve], capi.EC_ENC[GID[curve]]
    rng = random.Random(curve)
    scalars = b"".join(rng.randrange(1, ORDER[curve]).to_bytes(32, "big" if curve == "secp256k1" else "little") for _ in range(POOL))
    pool = eng.ec_batch_exp_generator(group, scalars)
    host_pool = (C.c_uint8 * len(pool)).from_buffer_copy(pool)
    dev_pool = torch.frombuffer(bytearray(pool), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for K, m in (SHAPES[int(s)] for s in args.shapes.split(",")):
        for space in (dict(host=capi.MPVSS_HOST, device=capi.MPVSS_DEVICE)[s] for s in args.spaces.split(",")):
            base = C.addressof(host_pool) if space == capi.MPVSS_HOST else dev_pool.data_ptr()
            for lists in args.lists.split(","):
                pos = [(C.c_int64 * m)(*range(1 + (i if lists == "distinct" else 0), m + 1 + (i if lists == "distinct" else 0)))
                       for i in range(K)]
                arr = (capi.EcSecret * K)()
                for i in range(K):
                    arr[i] = capi.EcSecret(C.addressof(pos[i]), base + ((i * 61) % (POOL - m + 1)) * L, m)
                st = (C.c_int * K)()
                g_many, m_many = (C.c_uint8 * (L * K))(), (C.c_uint8 * (32 * K))()
                g_loop, m_loop = (C.c_uint8 * (L * K))(), (C.c_uint8 * (32 * K))()

                def many():
                    eng._check(eng.lib.mpvss_ec_reconstruct_many(eng.ctx, group, space, arr, K, 0, st, C.cast(g_many, C.c_void_p),
                                                                 C.cast(m_many, C.c_void_p)), "ec_reconstruct_many")

                def loop():
                    for i in range(K):
                        s = arr[i]
                        eng._check(eng.lib.mpvss_ec_reconstruct(eng.ctx, group, space, s.positions_host, s.shares, m,
                                                                C.c_void_p(C.addressof(g_loop) + L * i),
                                                                C.c_void_p(C.addressof(m_loop) + 32 * i)), "ec_reconstruct")

                print(f"  {curve} {K} x {m} {lists}: many, then loop", file=sys.stderr, flush=True)
                s0 = eng.ec_reconstruct_many_stats()
                l0 = eng.ec_lagrange_stats() if HAS_MODE else dict(device=0, host=0)
                t_many, many_lo, many_hi = timed(many)
                k_ms = eng.lib.mpvss_last_kernel_ms(eng.ctx, 4)
                s1 = eng.ec_reconstruct_many_stats()
                l1 = eng.ec_lagrange_stats() if HAS_MODE else dict(device=0, host=0)
                assert list(st) == [0] * K
                if args.no_loop:
                    t_loop = lo = hi = float("nan")
                else:
                    t_loop, lo, hi = timed(loop)
                    assert bytes(g_many) == bytes(g_loop) and bytes(m_many) == bytes(m_loop)
                assert K == 1 or len({bytes(g_many)[L * i:L * i + L] for i in range(K)}) > 1
                calls = REPS + 1
                print(f"  {curve:12s} {K:7d} {m:5d} {'host' if space == capi.MPVSS_HOST else 'device':6s} {lists:8s} "
                      f"{t_loop:9.2f} {lo:9.2f} {hi:9.2f} {t_many:9.2f} {many_lo:9.2f} {many_hi:9.2f} {t_loop / t_many:8.2f} {(s1['passes'] - s0['passes']) // calls:7d} "
                      f"{(s1['grouped_secrets'] - s0['grouped_secrets']) // calls:7d} "
                      f"{(s1['single_secrets'] - s0['single_secrets']) // calls:6d} {MODE:8s} {(l1['device'] - l0['device']) // calls:6d} "
                      f"{(l1['host'] - l0['host']) // calls:6d} {k_ms:7.3f}  {hashlib.sha256(bytes(g_many) + bytes(m_many)).hexdigest()[:16]}", flush=True)
    assert dev_pool.cpu().numpy().tobytes() == pool, "the share pool in HBM changed"
eng.close()
