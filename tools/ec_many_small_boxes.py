#!/usr/bin/env python3
"""Curve groups: the boxes of one round through ONE mpvss_ec_verify_many call -- runs of small boxes as one dense batch -- against
the same call of a build of the parent commit (every box through a block slot of its own), in alternating fresh processes.  One
GPU; both sides go straight to the C ABI over buffers made once from the same seeds; every figure is the median of REPS calls
after one warm-up, with min .. max beside it; ROUNDS rounds, each a fresh process per side.  The results of the two sides
(verdicts and digests) are compared before anything is printed.  The new build is also measured under mode 0
(mpvss_ctx_set_ec_box_groups), and both sides record the loop of one-box calls (mpvss_ec_verify_distribution).

    python tools/ec_many_small_boxes.py --ab ab_libs/libmpvss_hip_parent.so > profiles/ec_many_small_boxes.txt
    python tools/ec_many_small_boxes.py --curves secp256k1 --shapes 0 --spaces host       (this build alone, a part of the table)"""
import argparse
import ctypes as C
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 3
ROUNDS = 2
SHAPES = ((400, 5, 3), (200, 100, 34), (60, 1024, 32))       # boxes, n, t
DISTINCT = 8                                                 # dealt boxes per shape; the call cycles through them
WORKER_LIMIT = 420                                           # seconds for one fresh process (all its shapes)
ORDER = {"secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
         "ristretto255": 2 ** 252 + 27742317777372353535851937790883648493}

ap = argparse.ArgumentParser()
ap.add_argument("--curves", default="secp256k1,ristretto255")
ap.add_argument("--shapes", default="0,1,2")
ap.add_argument("--spaces", default="host,device")
ap.add_argument("--ab", default=None, metavar="PARENT_LIB", help="libmpvss_hip.so of a build of the parent commit: the other side")
ap.add_argument("--worker", default=None, metavar="SIDE", help="(internal) measure in this process and print one JSON row per figure")
args = ap.parse_args()


def worker(side):
    import torch
    from mpvss_rs_amd import Engine, capi
    eng = Engine(0)
    lib = eng.lib
    grouped = hasattr(lib, "mpvss_ec_verify_many_stats")
    gid = {"secp256k1": capi.GROUP_SECP256K1, "ristretto255": capi.GROUP_RISTRETTO255}

    def timed(fn):
        fn()
        times = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times), min(times), max(times)

    for curve in args.curves.split(","):
        group, L = gid[curve], capi.EC_ENC[gid[curve]]
        for K, n, t in (SHAPES[int(s)] for s in args.shapes.split(",")):
            rng = random.Random(f"{curve}-{n}-{t}")
            sc = lambda k: b"".join(rng.randrange(1, ORDER[curve]).to_bytes(32, "big" if curve == "secp256k1" else "little") for _ in range(k))
            dealt = []
            for d in range(min(DISTINCT, K)):
                coeffs, privs, ws = sc(t), sc(n), sc(n)
                pubkeys = eng.ec_batch_exp_generator(group, privs)
                out = eng.ec_deal(group, coeffs, list(range(1, n + 1)), pubkeys, ws)
                resp = bytearray(out["responses"])
                if d == 1:
                    resp[40] ^= 1                             # one box of the cycle is answered `false`
                dealt.append(dict(commitments=eng.ec_batch_exp_generator(group, coeffs), pubkeys=pubkeys, shares=out["Y"],
                                  responses=bytes(resp), challenge=out["challenge"]))
            pos = (C.c_int64 * n)(*range(1, n + 1))
            for space_name in args.spaces.split(","):
                space = capi.MPVSS_HOST if space_name == "host" else capi.MPVSS_DEVICE
                keep, ptrs = [], []
                for b in dealt:
                    p = {}
                    for k in ("commitments", "pubkeys", "shares", "responses"):
                        if space == capi.MPVSS_HOST:
                            buf = (C.c_uint8 * len(b[k])).from_buffer_copy(b[k])
                            p[k] = C.addressof(buf)
                        else:
                            buf = torch.frombuffer(bytearray(b[k]), dtype=torch.uint8).cuda()
                            p[k] = buf.data_ptr()
                        keep.append(buf)
                    if space == capi.MPVSS_HOST:
                        p["positions"] = C.addressof(pos)
                    else:
                        dpos = torch.arange(1, n + 1, dtype=torch.int64).cuda()
                        keep.append(dpos)
                        p["positions"] = dpos.data_ptr()
                    ch = (C.c_uint8 * 32).from_buffer_copy(b["challenge"])
                    keep.append(ch)
                    p["challenge"] = C.addressof(ch)
                    ptrs.append(p)
                torch.cuda.synchronize()
                arr = (capi.EcBox * K)()
                for i in range(K):
                    p = ptrs[i % len(ptrs)]
                    arr[i] = capi.EcBox(p["commitments"], t, p["positions"], p["pubkeys"], p["shares"], p["responses"], n, p["challenge"])
                verdicts, digests = (C.c_int * K)(), (C.c_uint8 * (32 * K))()
                lv, ld = (C.c_int * K)(), (C.c_uint8 * (32 * K))()

                def many():
                    eng._check(lib.mpvss_ec_verify_many(eng.ctx, group, space, arr, K, 6, 3, verdicts, C.cast(digests, C.c_void_p)), "ec_verify_many")

                def loop():
                    for i in range(K):
                        b = arr[i]
                        v = C.c_int(0)
                        eng._check(lib.mpvss_ec_verify_distribution(eng.ctx, group, space, b.commitments, t, b.positions, b.pubkeys, b.shares,
                                                                    b.responses, n, b.challenge_host, C.byref(v),
                                                                    C.c_void_p(C.addressof(ld) + 32 * i), None, None, None), "ec_verify_distribution")
                        lv[i] = v.value

                def row(what, fig, stats=None):
                    res = hashlib.sha256(bytes(verdicts) + bytes(digests)).hexdigest()
                    print(json.dumps(dict(side=side, curve=curve, K=K, n=n, t=t, space=space_name, what=what, med=fig[0], lo=fig[1], hi=fig[2],
                                          results=res, good=sum(verdicts), stats=stats)), flush=True)

                print(f"  {side} {curve} {K} x ({n}, {t}) {space_name}", file=sys.stderr, flush=True)
                if grouped:
                    eng.set_ec_box_groups(1)
                    s0 = eng.ec_verify_many_stats()
                    fig = timed(many)
                    s1 = eng.ec_verify_many_stats()
                    row("many", fig, {k: (s1[k] - s0[k]) // (REPS + 1) for k in s0})
                    eng.set_ec_box_groups(0)
                    row("many_mode0", timed(many))
                else:
                    row("many", timed(many))
                fig = timed(loop)
                assert list(lv) == list(verdicts) and bytes(ld) == bytes(digests), "the loop of one-box calls and the many-box call differ"
                assert 0 < sum(verdicts) < K
                row("loop", fig)
    eng.close()


def run_worker(side, lib):
    env = dict(os.environ)
    if lib:
        env["MPVSS_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--curves", args.curves, "--shapes", args.shapes, "--spaces", args.spaces]
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=WORKER_LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit(f"ec_many_small_boxes: the {side} process did not end within {WORKER_LIMIT} s; nothing more is started")
    if r.returncode != 0:
        sys.exit(f"ec_many_small_boxes: the {side} process ended with {r.returncode}; nothing more is started")
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def main():
    rows = []
    for rnd in range(ROUNDS):
        for side, lib in ((("parent", args.ab),) if args.ab else ()) + (("new", None),):
            for row in run_worker(side, lib):
                row["round"] = rnd
                rows.append(row)
    keys = []
    for r in rows:
        k = (r["curve"], r["K"], r["n"], r["t"], r["space"])
        if k not in keys:
            keys.append(k)
    print(f"# median of {REPS} calls after one warm-up, ms for all boxes of the call (min .. max of the {REPS}); {ROUNDS} rounds, a fresh process per side and round")
    print("# parent: mpvss_ec_verify_many of a build of the parent commit; grouped / mode0: this build under mpvss_ctx_set_ec_box_groups 1 / 0;")
    print("# loop: one mpvss_ec_verify_distribution call per box (this build); ratio: parent's best round / grouped's worst round")
    lost = []
    for k in keys:
        mine = [r for r in rows if (r["curve"], r["K"], r["n"], r["t"], r["space"]) == k]
        assert len({r["results"] for r in mine}) == 1, f"{k}: the sides give different verdicts or digests"
        print(f"{k[0]:12s} {k[1]:4d} x ({k[2]}, {k[3]}) {k[4]:6s}  boxes answered true: {mine[0]['good']}")
        for what, side in (("many", "parent"), ("many", "new"), ("many_mode0", "new"), ("loop", "parent"), ("loop", "new")):
            sel = [r for r in mine if r["what"] == what and r["side"] == side]
            if not sel:
                continue
            name = {("many", "parent"): "parent", ("many", "new"): "grouped", ("many_mode0", "new"): "mode0",
                    ("loop", "parent"): "loop (parent)", ("loop", "new"): "loop"}[(what, side)]
            figs = "   ".join(f"round {r['round']}: {r['med']:9.2f} ({r['lo']:.2f} .. {r['hi']:.2f})" for r in sel)
            extra = f"   stats per call {sel[0]['stats']}" if sel[0].get("stats") else ""
            print(f"    {name:14s} {figs}{extra}")
        par = [r["med"] for r in mine if r["what"] == "many" and r["side"] == "parent"]
        new = [r["med"] for r in mine if r["what"] == "many" and r["side"] == "new"]
        if par and new:
            print(f"    ratio          {min(par) / max(new):9.2f}   (parent's rounds {min(par):.2f} .. {max(par):.2f}, grouped's {min(new):.2f} .. {max(new):.2f})")
            if max(new) > max(par):
                lost.append((k, max(new), max(par)))
    if args.ab:
        print("# shapes at which the grouped path was slower than the parent beyond the spread of the parent's rounds: " +
              (", ".join(f"{k} {a:.2f} > {b:.2f} ms" for k, a, b in lost) if lost else "none"))


if __name__ == "__main__":
    if args.worker:
        worker(args.worker)
    else:
        main()
