#!/usr/bin/env python3
"""Run-time MODP groups: the secrets of one round through ONE mpvss_modp_group_reconstruct_many call, against the loop of
mpvss_modp_group_reconstruct calls over the same secrets -- the only way there was before.  One GPU, warm context, group_prepare
done; both sides go straight to the C ABI over buffers made once; every figure is the median of REPS repetitions after one
warm-up.  The results of the two sides are compared before anything is printed.  Every shape runs once with the same position
list for all its secrets and once with a list of its own for each, so that the share of the Lagrange cache shows.

    python tools/modp_rt_reconstruct_many.py > profiles/modp_rt_reconstruct_many.txt
    python tools/modp_rt_reconstruct_many.py --bits 2048 --shapes 3 --spaces host      (a part of the table: shape 3 is 60 x 1024)

--lagrange {host,device,auto} sets where the Lagrange exponents are computed (mpvss_ctx_set_rt_lagrange; a library of an older
commit, MPVSS_HIP_LIB, has no such switch and is reported as "parent").  --no-loop leaves the loop of one-secret calls out -- at
16384 shares it takes minutes on the host -- and every row carries a digest of the call's results, so that runs of different
builds and modes can be compared line by line (profiles/modp_rt_lagrange_device.txt).  Shapes 4 to 6 are ONE secret of 1024 and of
16384 shares (a call of one secret is the one-secret path, mpvss_modp_group_reconstruct) and 8 secrets of 16384; --bits 3072 and
4096 are RFC 3526 groups 15 and 16 through the wide handles."""
import argparse
import ctypes as C
import hashlib
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
SHAPES = ((400, 3), (200, 34), (60, 32), (60, 1024), (1, 1024), (1, 16384), (8, 16384))        # secrets, m

ap = argparse.ArgumentParser()
ap.add_argument("--bits", default="1024,2048")
ap.add_argument("--shapes", default="0,1,2,3")
ap.add_argument("--spaces", default="host,device")
ap.add_argument("--lists", default="equal,distinct")
ap.add_argument("--lagrange", choices=("host", "device", "auto"), default=None)
ap.add_argument("--no-loop", action="store_true")
args = ap.parse_args()

eng = Engine(0)
HAS_MODE = hasattr(eng.lib, "mpvss_modp_group_lagrange_exponents")
MODE = (args.lagrange or "auto") if HAS_MODE else "parent"
if HAS_MODE and args.lagrange:
    eng.set_rt_lagrange(("host", "auto", "device").index(args.lagrange))
# shares made per group; a secret takes m consecutive ones
POOL = 2048 if max(SHAPES[int(s)][1] for s in args.shapes.split(",")) <= 1024 else 16384 + 512


def modulus(bits):
    """(q, bytes of an element) of the RFC group of `bits` bits"""
    if bits == 3072:
        import modp_rt_wide_helpers as WH
        return WH.group15(), WH.EB
    if bits == 4096:
        import modp_rt_4096_helpers as H4
        return H4.group16(), H4.EB
    return H.rfc_prime(bits), 256


def timed(fn):
    """(median, min, max) in ms of REPS repetitions after one warm-up"""
    fn()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


print(f"# {torch.cuda.get_device_name(0)}; median of {REPS} after one warm-up; ms for all secrets of the call; min / max: the spread of the {REPS} runs")
print("# lagrange: where the exponents are computed; dev_l / host_l / fb_l: position lists per call computed on either side and those done again on the host; k4_ms: kernel kind 4 in the last call (hipEvents)")
print("# bits secrets     m space  lists      loop_ms   many_ms  many_min  many_max  speedup  passes grouped single lagrange  dev_l host_l   fb_l    k4_ms  digest",
      flush=True)
for bits in (int(b) for b in args.bits.split(",")):
    q, EB = modulus(bits)
    grp = ModpGroup(q, elem_bytes=EB)
    eng.group_prepare(grp)
    rng = random.Random(bits)
    pool = eng.group_batch_exp_fixed_base(grp, (4).to_bytes(EB, "big"), b"".join(rng.randrange(1, q - 1).to_bytes(EB, "big") for _ in range(POOL)))
    host_pool = (C.c_uint8 * len(pool)).from_buffer_copy(pool)
    dev_pool = torch.frombuffer(bytearray(pool), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for K, m in (SHAPES[int(s)] for s in args.shapes.split(",")):
        for space in (dict(host=capi.MPVSS_HOST, device=capi.MPVSS_DEVICE)[s] for s in args.spaces.split(",")):
            base = C.addressof(host_pool) if space == capi.MPVSS_HOST else dev_pool.data_ptr()
            for lists in args.lists.split(","):
                pos = [(C.c_int64 * m)(*range(1 + (i if lists == "distinct" else 0), m + 1 + (i if lists == "distinct" else 0)))
                       for i in range(K)]
                arr = (capi.GroupSecret * K)()
                for i in range(K):
                    arr[i] = capi.GroupSecret(C.addressof(pos[i]), base + ((i * m if m <= 1024 else i * 61) % (POOL - m + 1)) * EB, m)
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

                zero = dict(device=0, host=0, fallback=0)
                s0 = eng.group_reconstruct_many_stats()
                l0 = eng.group_lagrange_stats() if HAS_MODE else zero
                t_many, many_lo, many_hi = timed(many)
                k_ms = eng.kernel_ms(4)
                s1 = eng.group_reconstruct_many_stats()
                l1 = eng.group_lagrange_stats() if HAS_MODE else zero
                assert list(st) == [0] * K
                if args.no_loop:
                    t_loop = float("nan")
                else:
                    t_loop = timed(loop)[0]
                    assert bytes(g_many) == bytes(g_loop) and bytes(m_many) == bytes(m_loop)
                assert K == 1 or len({bytes(g_many)[EB * i:EB * i + EB] for i in range(K)}) > 1
                calls = REPS + 1
                print(f"  {bits:4d} {K:7d} {m:5d} {'host' if space == capi.MPVSS_HOST else 'device':6s} {lists:8s} "
                      f"{t_loop:9.2f} {t_many:9.2f} {many_lo:9.2f} {many_hi:9.2f} {t_loop / t_many:8.2f} {(s1['passes'] - s0['passes']) // calls:7d} "
                      f"{(s1['grouped_secrets'] - s0['grouped_secrets']) // calls:7d} "
                      f"{(s1['single_secrets'] - s0['single_secrets']) // calls:6d} {MODE:8s} {(l1['device'] - l0['device']) // calls:6d} "
                      f"{(l1['host'] - l0['host']) // calls:6d} {(l1['fallback'] - l0['fallback']) // calls:6d} {k_ms:8.3f}  "
                      f"{hashlib.sha256(bytes(g_many) + bytes(m_many)).hexdigest()[:16]}", flush=True)
    assert dev_pool.cpu().numpy().tobytes() == pool, "the share pool in HBM changed"
eng.close()
