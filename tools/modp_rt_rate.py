"""Rates of the run-time MODP group entry points (include/mpvss_hip.h, mpvss_modp_group_*) on one GPU.

  batch_exp   n = 65536 bases and exponents as long as the modulus, at 512, 1024, 1536 and 2048 bits, beside the group-14
              entry point mpvss_modp_batch_exp on the same shape (random 2048-bit exponents)
  verify      mpvss_modp_group_verify_distribution at (n, t) = (4096, 64) and (65536, 256) for 1024, 1536 and 2048 bits:
              share verifications per second (random box contents: the same work as a valid box, the verdict is 0)

  twin        (--legs twin) two powers of one base, kernels alone (mpvss_last_kernel_ms): mpvss_modp_group_batch_twin_exp as the
              loaded library dispatches it, beside the baseline a caller had before it: two mpvss_modp_group_batch_exp calls
              over the same bases, at n = 256 .. 65536 for 1024 and 2048 bits (--twin-parts call / baseline: one of the two)
  deal        (--legs deal) mpvss_modp_group_deal and mpvss_modp_group_extract_shares as whole calls from host buffers at
              (n, t) = (4096, 64) and (65536, 256) for 1024 and 2048 bits: shares per second and the kernels' time inside the
              call.  host_scalar_retimed_ms is NOT measured inside the call: it is a separate timing, afterwards, of the
              scalar-ring entry points on operands of the same size (P(i) and the responses, or the n products w / x);
              rest_ms = call - kernels - that figure (hashing, staging, copies)
  --ab PARENT the interleaved A/B behind the crossover constant (rt_twin_min_shares, capi_modp_rt.inc) and the 1.2x gate.
              Needs `make -C mpvss_rs_amd/csrc twin-ab` (ab_libs/libmpvss_hip_twin.so and _sets.so: the dispatch pinned to
              either path) and PARENT, a built checkout of the commit before the twin path (git worktree add PARENT <commit>;
              make -C PARENT/mpvss_rs_amd/csrc).  Each round runs three fresh processes of this tool one after the other:
              the twin build, the sets build, and the baseline under PARENT's own bindings and library; the best of all
              rounds per (path, bits, n) makes the table, the crossover per width is the smallest measured n from which the
              twin kernel beats the sets at every measured n above, and the gate is twin against PARENT's two batch_exp calls
              at n = 65536.  Then the deal leg runs under the default library.  All lines go to profiles/modp_rt_deal_rate.txt.

  row         (--row) the row layout for small calls (mpvss_ctx_set_rt_row): modes 0 and 2 of the loaded library in turns on one
              warm context, results compared first, median of 5 -- kernels alone (timer 3) of group_batch_exp with full-width
              exponents at 2048 / 3072 / 4096 bits and n = 1 .. 16384, and whole one-box calls (verify_distribution, deal,
              extract_shares, verify_shares) at (5, 3) and (64, 22).  Written to profiles/modp_rt_row_rate.txt.

  comb        (--comb, or --legs comb) the fixed-base power g^e of a run-time group, kernels alone (mpvss_last_kernel_ms), at
              n = 1 .. 65536 for 1024 and 2048 bits.  --comb-parts parent: the launch a caller had before the comb -- a1_i = g^w_i
              inside mpvss_modp_group_deal (t = 1), timer 1: the 16-entry table of g and the left-to-right kernel.  --comb-parts
              comb: mpvss_modp_group_batch_exp_fixed_base under the tuning build of `make -C mpvss_rs_amd/csrc comb-ab`
              (ab_libs/libmpvss_hip_comb.so: every call builds the comb of a base it has not cached) -- cold: a base the
              context has not seen, build + comb launch (timers 2 + 1); warm: the same base again, the comb launch alone.
  --comb --ab PARENT  the interleaved A/B behind rt_comb_min_shares (capi_modp_rt.inc) and the 3x kernel gate: each round runs
              the parent part under PARENT's own bindings and library and the comb part under the tuning build, each in a fresh
              process; the best of all rounds per (part, bits, n) makes the table.  The crossover per width is the smallest
              measured n from which the cold call is no slower than the parent's launch at every measured n above (1 if that
              holds everywhere); the gate is warm against parent at n = 65536.  Then group_deal / group_extract_shares at
              (65536, 256) and group_verify_distribution at (4096, 64) run as whole calls under PARENT and under the default
              library (no gate).  All lines go to profiles/modp_rt_comb_rate.txt.

Host buffers in and out (the calls' own staging included), best of `--reps` after one warm-up call.  One JSON line per
measurement.  Usage: python tools/modp_rt_rate.py [--quick] [--reps 3] [--legs rates,twin,deal,comb,verify] [--comb | --fd | --scalar | --keyset | --share-hash] [--ab PARENT [--rounds 2]]
  fd          (--fd) X_i of a run-time group by forward differences: timer 0 of group_commit_eval at (4096, 64), (16384, 128),
              (65536, 256), 1024 and 2048 bits, per chain count, and whole group_verify_distribution calls; --fd --ab PARENT takes
              turns with a built checkout of the parent commit and writes profiles/modp_rt_fd_rate.txt (one 3072-bit row too).
  scalar      (--scalar) the scalar ring Z/(q-1) of a run-time group on the device: whole group_deal calls at (1024, 32), (4096, 64),
              (16384, 128), (65536, 256) and whole group_extract_shares calls at n = 1024, 4096, 65536, for 1024 and 2048 bits
              (--scalar-wide: the one 3072-bit row, group_deal at (4096, 64)).  --scalar-parts parent: the library under test as it
              is (host threads before this path existed); mode2: mpvss_ctx_set_rt_scalar(2), with the time of the scalar-ring
              kernels (timer 4).  --scalar --ab PARENT: fresh processes of a built checkout of the parent commit and of this
              build under mode 2 take turns, best of the rounds, into profiles/modp_rt_scalar_rate.txt; rt_scalar_min_shares of
              a width is the smallest measured n from which mode 2's whole call is no slower than the parent's at every larger
              measured n (1 if that holds everywhere).  No speed gate.
  keyset      (--keyset) key sets of a run-time group, kernels alone, at n = 4096, 16384, 65536 for 1024 and 2048 bits (--keyset-wide:
              the one 3072-bit row, n = 16384); exponents as long as q, c of 256 bits.  --keyset-parts parent: what a caller has
              without a set -- the a2 launch of group_dleq_commitments (timer 3) and the twin launch inside group_deal (t = 1,
              timer 3); keyset: the build (timer 2) and its bytes, the launch of group_keyset_dual_exp with h2 and a shared c, and of
              group_keyset_twin_exp (timer 3).  At (65536, 256) both parts also time whole group_verify_distribution and group_deal
              calls (the key-set forms in the keyset part; the build is not in them).
  --keyset --ab PARENT  fresh processes of a built checkout of the parent commit and of this build take turns, best of the rounds,
              into profiles/modp_rt_keyset_rate.txt.  The gate, at n = 65536 and 2048 bits: the key-set a2 launch against the
              parent's a2 launch, at least 2x required (the operation counts say 3.65x); below 1x the kernels do not ship.  The
              twin ratio is recorded and not gated.
  share-hash  (--share-hash) the per-share DLEQ hash of a run-time group on the device: whole group_verify_shares and
              group_extract_shares calls at n = 1024, 4096, 65536 for 1024 and 2048 bits from host buffers, plus one row with the
              arrays in device memory (group_verify_shares, 2048 bits, n = 65536; torch tensors); --share-hash-wide: the one 3072-bit
              row, both calls at n = 16384.  --share-hash-parts parent: the library under test as it is (every share hashed on the
              host before this path existed); mode2: mpvss_ctx_set_rt_share_hash(2), with the time of the hash launches (timer 5).
  w4096       (--legs w4096) 4096 bits (512-byte handle) beside 3072 bits (384-byte handle) in one session: kernels alone for
              group_batch_exp and whole group_verify_distribution calls (t = 64) at n = 1024 and 65536, and their ratios beside the
              count-derived 2.37; recorded in profiles/modp_rt_4096_rate.txt, no gate.
  --share-hash --ab PARENT  fresh processes of a built checkout of the parent commit and of this build under mode 2 take turns,
              best of the rounds, into profiles/modp_rt_share_hash_rate.txt.  rt_share_hash_min_shares is the smallest measured n
              from which mode 2's whole call is no slower than the parent's at every larger measured n (1 if that holds
              everywhere).  The gate, at n = 65536: mode 2 no slower than the parent beyond the spread of the parent's own rounds."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import modp_rt_helpers as H  # noqa: E402

Engine = ModpGroup = capi = None          # bound by load_package(): from this checkout, or from --package-root


def load_package(root):
    global Engine, ModpGroup, capi
    if root:
        sys.path.insert(0, os.path.abspath(root))
    import mpvss_rs_amd
    Engine, ModpGroup, capi = mpvss_rs_amd.Engine, mpvss_rs_amd.ModpGroup, mpvss_rs_amd.capi


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def kernel_ms(eng):
    """GPU time of the last call's kernels (hipEvents around each launch, summed over the kinds of mpvss_last_kernel_ms)"""
    return round(sum(max(0.0, eng.kernel_ms(k)) for k in range(4)), 3)


def rand_bytes(rng, n, bits):
    return b"".join(rng.getrandbits(bits).to_bytes(256, "big") for _ in range(n))


def twin_leg(eng, a, rng):
    lib = os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH)
    sizes = [256, 4096] if a.quick else [256, 1024, 4096, 8192, 16384, 32768, 65536]
    for bits in (1024, 2048):
        grp = ModpGroup(H.rfc_prime(bits))
        for n in sizes:
            B, E1, E2 = rand_bytes(rng, n, 2048), rand_bytes(rng, n, bits), rand_bytes(rng, n, bits)
            row = {"what": "twin", "lib": lib, "bits": bits, "n": n}
            if "call" in a.twin_parts:
                ts = []
                for _ in range(a.reps + 1):
                    eng.group_batch_twin_exp(grp, B, E1, E2)
                    ts.append(kernel_ms(eng))
                row["twin_call_kernel_ms"] = min(ts[1:])
            if "baseline" in a.twin_parts:
                ts = []
                for _ in range(a.reps + 1):
                    eng.group_batch_exp(grp, B, E1)
                    k = kernel_ms(eng)
                    eng.group_batch_exp(grp, B, E2)
                    ts.append(round(k + kernel_ms(eng), 3))
                row["two_batch_exp_kernel_ms"] = min(ts[1:])
            if "twin_call_kernel_ms" in row and "two_batch_exp_kernel_ms" in row:
                row["speedup"] = round(row["two_batch_exp_kernel_ms"] / row["twin_call_kernel_ms"], 3)
            print(json.dumps(row), flush=True)


def deal_leg(eng, a, rng):
    shapes = [(4096, 64)] if a.quick else [(4096, 64), (65536, 256)]
    for bits in (1024, 2048):
        q = H.rfc_prime(bits)
        grp = ModpGroup(q)
        for n, t in shapes:
            coeffs, pos = rand_bytes(rng, t, bits - 1), list(range(1, n + 1))
            y, w = rand_bytes(rng, n, bits - 1), rand_bytes(rng, n, bits - 1)
            s = best(lambda: eng.group_deal(grp, coeffs, pos, y, w), a.reps)
            kms = kernel_ms(eng)
            t0 = time.perf_counter()
            P = capi.group_poly_eval(grp, coeffs, pos)
            capi.group_dleq_responses(grp, w, P, rand_bytes(rng, 1, 255))
            host = time.perf_counter() - t0
            print(json.dumps({"what": "group_deal", "bits": bits, "n": n, "t": t, "s": round(s, 4), "shares_per_s": round(n / s),
                              "kernel_ms": kms, "host_scalar_retimed_ms": round(host * 1e3, 1),
                              "rest_ms": round(s * 1e3 - host * 1e3 - kms, 1)}), flush=True)
            xinv = rand_bytes(rng, n, bits - 1)
            s = best(lambda: eng.group_extract_shares(grp, y, y, xinv, w), a.reps)
            kms = kernel_ms(eng)
            t0 = time.perf_counter()
            capi.group_dleq_responses(grp, w, w, xinv)          # n products mod (q-1): the cost of e2 = w / x
            host = time.perf_counter() - t0
            print(json.dumps({"what": "group_extract_shares", "bits": bits, "n": n, "s": round(s, 4), "shares_per_s": round(n / s),
                              "kernel_ms": kms, "host_scalar_retimed_ms": round(host * 1e3, 1),
                              "rest_ms": round(s * 1e3 - host * 1e3 - kms, 1)}), flush=True)


COMB_SIZES = [1, 16, 256, 1024, 4096, 16384, 65536]


def comb_leg(eng, a, rng):
    lib = os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH)
    sizes = [1, 256, 4096] if a.quick else COMB_SIZES
    fresh = 5                                     # bases 5, 6, ..: never a generator, a new one for every cold call
    for bits in (1024, 2048):
        grp = ModpGroup(H.rfc_prime(bits))
        for n in sizes:
            w = rand_bytes(random.Random(bits * 100003 + n), n, bits)
            row = {"what": "comb", "lib": lib, "bits": bits, "n": n}
            if "parent" in a.comb_parts:
                y, pos, coeffs = rand_bytes(rng, n, bits - 1), list(range(1, n + 1)), rand_bytes(rng, 1, bits - 1)
                ts = []
                for _ in range(a.reps + 1):
                    eng.group_deal(grp, coeffs, pos, y, w)
                    ts.append(round(max(0.0, eng.kernel_ms(1)), 3))
                row["parent_fixed_base_kernel_ms"] = min(ts[1:])
            if "comb" in a.comb_parts:
                if grp.comb_min_shares != 1:
                    sys.exit("modp_rt_rate --comb: the comb part needs the tuning build (make -C mpvss_rs_amd/csrc comb-ab, "
                             "MPVSS_HIP_LIB=ab_libs/libmpvss_hip_comb.so)")
                cold, build, warm = [], [], []
                for _ in range(a.reps + 1):
                    base = fresh.to_bytes(256, "big")
                    fresh += 1
                    eng.group_batch_exp_fixed_base(grp, base, w)
                    build.append(round(max(0.0, eng.kernel_ms(2)), 3))
                    cold.append(round(build[-1] + max(0.0, eng.kernel_ms(1)), 3))
                    eng.group_batch_exp_fixed_base(grp, base, w)
                    warm.append(round(max(0.0, eng.kernel_ms(1)), 3))
                row.update(comb_cold_kernel_ms=min(cold[1:]), comb_build_kernel_ms=min(build[1:]), comb_warm_kernel_ms=min(warm[1:]))
            print(json.dumps(row), flush=True)


def verify_leg(eng, a, rng):
    for bits in (1024, 2048):
        grp = ModpGroup(H.rfc_prime(bits))
        nn, t = 4096, 64
        cm, pos = rand_bytes(rng, t, bits), list(range(1, nn + 1))
        y, Y, r = rand_bytes(rng, nn, bits), rand_bytes(rng, nn, bits), rand_bytes(rng, nn, bits)
        c = rng.getrandbits(min(bits - 2, 256)).to_bytes(256, "big")
        s = best(lambda: eng.group_verify_distribution(grp, cm, pos, y, Y, r, c), a.reps)
        print(json.dumps({"what": "group_verify_distribution", "bits": bits, "n": nn, "t": t, "s": round(s, 4),
                          "share_verifications_per_s": round(nn / s), "kernel_ms": kernel_ms(eng)}), flush=True)


FD_SHAPES = [(4096, 64), (16384, 128), (65536, 256)]
FD_CHAINS = [4, 8, 16, 32, 64]


def fd_leg(eng, a, rng):
    """timer 0 alone (the whole X path of mpvss_modp_group_commit_eval) and whole group_verify_distribution calls.  --fd-parts
    parent: Horner's rule as the library under test has it (a parent build knows nothing else); fd: mode 2 at each chain count,
    and mode 0 of the same build beside it."""
    parts = a.fd_parts.split(",")
    shapes = [(4096, 64)] if a.quick else FD_SHAPES
    groups = [(1024, ModpGroup(H.rfc_prime(1024))), (2048, ModpGroup(H.rfc_prime(2048)))]
    if a.fd_wide:
        groups = [(3072, ModpGroup(H.random_odd_modulus(3072, random.Random(3072)), elem_bytes=384))]
        shapes = [(16384, 128)]
    for bits, grp in groups:
        EB = grp.elem_bytes
        for nn, t in shapes:
            cm = b"".join((rng.getrandbits(bits - 1) | 1).to_bytes(EB, "big") for _ in range(t))
            pos = list(range(1, nn + 1))

            def x_ms():
                ts = []
                for _ in range(a.reps + 1):
                    eng.group_commit_eval(grp, cm, pos)
                    ts.append(round(max(0.0, eng.kernel_ms(0)), 3))
                return min(ts[1:])

            row = {"what": "fd", "bits": bits, "n": nn, "t": t}
            if "parent" in parts:
                row["horner_kernel_ms"] = x_ms()
            if "fd" in parts:
                eng.set_rt_fd(0, 0)
                row["mode0_kernel_ms"] = x_ms()
                for ch in FD_CHAINS:
                    eng.set_rt_fd(2, ch)
                    before = eng.group_fd_stats()["fd"]
                    row[f"fd_chains_{ch}_kernel_ms"] = x_ms()
                    assert eng.group_fd_stats()["fd"] > before, "the call did not take forward differences"
                eng.set_rt_fd(2, 0)
            if not a.fd_wide:
                y, Y, r = (b"".join(rng.getrandbits(bits - 1).to_bytes(EB, "big") for _ in range(nn)) for _ in range(3))
                c = rng.getrandbits(256).to_bytes(EB, "big")
                s = best(lambda: eng.group_verify_distribution(grp, cm, pos, y, Y, r, c), a.reps)
                row["verify_s"] = round(s, 4)
                row["share_verifications_per_s"] = round(nn / s)
            print(json.dumps(row), flush=True)


def child(args, lib, out, limit):
    """one fresh process of this tool (the GPU is opened there only); its JSON lines, also echoed.  A child that fails ends
    the whole run: nothing more is started on the GPU after it.  `limit`: seconds this leg may take."""
    env = dict(os.environ)
    if lib:
        env["MPVSS_HIP_LIB"] = lib
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"modp_rt_rate: {args} under {lib or 'the default library'} did not end within {limit} s; nothing more is started")
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    for row in rows:
        print(json.dumps(row), flush=True)
    out += rows
    if r.returncode != 0:
        sys.exit(f"modp_rt_rate: {args} under {lib or 'the default library'} ended with {r.returncode}")
    return rows


def ab(a):
    libs = {k: os.path.join(ROOT, "ab_libs", f"libmpvss_hip_{k}.so") for k in ("twin", "sets")}
    for f in list(libs.values()) + [os.path.join(a.ab, "mpvss_rs_amd", "libmpvss_hip.so")]:
        if not os.path.exists(f):
            sys.exit(f"modp_rt_rate --ab: {f} is missing (see the head of this file)")
    common = ["--legs", "twin", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    lines, ms = [], {}
    for rnd in range(a.rounds):
        for path in ("twin", "sets", "parent"):
            if path == "parent":
                rows = child(common + ["--twin-parts", "baseline", "--package-root", a.ab], None, [], a.twin_limit)
            else:
                rows = child(common + ["--twin-parts", "call"], libs[path], [], a.twin_limit)
            for row in rows:
                row.update(path=path, round=rnd)
                v = row.get("twin_call_kernel_ms", row.get("two_batch_exp_kernel_ms"))
                key = (path, row["bits"], row["n"])
                ms[key] = min(ms.get(key, v), v)
            lines += rows
    for bits in sorted({k[1] for k in ms}):
        sizes = sorted({k[2] for k in ms if k[1] == bits})
        wins = []
        for n in sizes:
            tw, st, pa = ms["twin", bits, n], ms["sets", bits, n], ms["parent", bits, n]
            wins.append(tw < st)
            lines.append({"what": "twin_ab", "bits": bits, "n": n, "twin_kernel_ms": tw, "sets_kernel_ms": st,
                          "parent_two_batch_exp_kernel_ms": pa, "twin_over_parent": round(pa / tw, 3),
                          "sets_over_parent": round(pa / st, 3), "twin_over_sets": round(st / tw, 3)})
        first = next((n for i, n in enumerate(sizes) if all(wins[i:])), None)
        lines.append({"what": "twin_crossover", "bits": bits, "min_shares": first, "measured_sizes": sizes})
        top = sizes[-1]
        lines.append({"what": "twin_gate", "bits": bits, "n": top, "twin_over_parent": round(ms["parent", bits, top] / ms["twin", bits, top], 3),
                      "required": 1.2, "met": ms["parent", bits, top] / ms["twin", bits, top] >= 1.2})
    for row in lines:
        if row["what"].startswith("twin_"):
            print(json.dumps(row), flush=True)
    child(["--legs", "deal", "--reps", str(a.reps)] + (["--quick"] if a.quick else []), None, lines, a.deal_limit)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


def ab_comb(a):
    lib = os.path.join(ROOT, "ab_libs", "libmpvss_hip_comb.so")
    for f in (lib, os.path.join(a.ab, "mpvss_rs_amd", "libmpvss_hip.so")):
        if not os.path.exists(f):
            sys.exit(f"modp_rt_rate --comb --ab: {f} is missing (see the head of this file)")
    common = ["--legs", "comb", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    lines, ms = [], {}
    for rnd in range(a.rounds):
        for part in ("parent", "comb"):
            if part == "parent":
                rows = child(common + ["--comb-parts", "parent", "--package-root", a.ab], None, [], a.twin_limit)
            else:
                rows = child(common + ["--comb-parts", "comb"], lib, [], a.twin_limit)
            for row in rows:
                row.update(part=part, round=rnd)
                for k, v in row.items():
                    if k.endswith("_kernel_ms"):
                        key = (k, row["bits"], row["n"])
                        ms[key] = min(ms.get(key, v), v)
            lines += rows
    for bits in sorted({k[1] for k in ms}):
        sizes = sorted({k[2] for k in ms if k[1] == bits})
        ok = []
        for n in sizes:
            pa, cold = ms["parent_fixed_base_kernel_ms", bits, n], ms["comb_cold_kernel_ms", bits, n]
            warm, build = ms["comb_warm_kernel_ms", bits, n], ms["comb_build_kernel_ms", bits, n]
            ok.append(cold <= pa)
            lines.append({"what": "comb_ab", "bits": bits, "n": n, "parent_fixed_base_kernel_ms": pa, "comb_cold_kernel_ms": cold,
                          "comb_build_kernel_ms": build, "comb_warm_kernel_ms": warm, "parent_over_cold": round(pa / cold, 3),
                          "parent_over_warm": round(pa / warm, 3)})
        first = next((n for i, n in enumerate(sizes) if all(ok[i:])), None)
        lines.append({"what": "comb_crossover", "bits": bits, "min_shares": first, "measured_sizes": sizes})
        top = sizes[-1]
        ratio = ms["parent_fixed_base_kernel_ms", bits, top] / ms["comb_warm_kernel_ms", bits, top]
        lines.append({"what": "comb_gate", "bits": bits, "n": top, "parent_over_warm": round(ratio, 3), "required": 3.0,
                      "met": ratio >= 3.0})
    for row in lines:
        if row["what"].startswith("comb_"):
            print(json.dumps(row), flush=True)
    whole = ["--legs", "deal,verify", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    for side, extra in (("parent", ["--package-root", a.ab]), ("change", [])):
        for row in child(whole + extra, None, [], a.deal_limit):
            row["side"] = side
            lines.append(row)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


SCALAR_DEAL = [(1024, 32), (4096, 64), (16384, 128), (65536, 256)]
SCALAR_EXTRACT = [1024, 4096, 65536]


def scalar_leg(eng, a, rng):
    mode2 = a.scalar_parts == "mode2"
    if mode2:
        eng.set_rt_scalar(2)
    if a.scalar_wide:
        import modp_rt_wide_helpers as WH
        groups = [(3072, ModpGroup(WH.group15(), elem_bytes=WH.EB), WH.EB)]
        deal, extract = [(4096, 64)], []
    else:
        groups = [(bits, ModpGroup(H.rfc_prime(bits)), 256) for bits in (1024, 2048)]
        deal, extract = (SCALAR_DEAL[:2], SCALAR_EXTRACT[:1]) if a.quick else (SCALAR_DEAL, SCALAR_EXTRACT)

    def rb(n, bits, eb):
        return b"".join(rng.getrandbits(bits).to_bytes(eb, "big") for _ in range(n))

    for bits, grp, eb in groups:
        for n, t in deal:
            coeffs, pos = rb(t, bits - 1, eb), list(range(1, n + 1))
            y, w = rb(n, bits - 1, eb), rb(n, bits - 1, eb)
            s = best(lambda: eng.group_deal(grp, coeffs, pos, y, w), a.reps)
            row = {"what": "scalar", "call": "group_deal", "bits": bits, "n": n, "t": t, "whole_s": round(s, 5)}
            if mode2:
                row["scalar_kernel_ms"] = round(max(0.0, eng.kernel_ms(4)), 3)
            print(json.dumps(row), flush=True)
        for n in extract:
            pk, y, xi, w = (rb(n, bits - 1, eb) for _ in range(4))
            s = best(lambda: eng.group_extract_shares(grp, pk, y, xi, w), a.reps)
            row = {"what": "scalar", "call": "group_extract_shares", "bits": bits, "n": n, "t": 0, "whole_s": round(s, 5)}
            if mode2:
                row["scalar_kernel_ms"] = round(max(0.0, eng.kernel_ms(4)), 3)
            print(json.dumps(row), flush=True)


def ab_scalar(a):
    """--scalar --ab PARENT: fresh processes of the parent build and of this build under mode 2 take turns; best of the rounds"""
    if not os.path.exists(os.path.join(a.ab, "mpvss_rs_amd", "libmpvss_hip.so")):
        sys.exit("modp_rt_rate --scalar --ab: the parent checkout is not built")
    common = ["--legs", "scalar", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    lines, ms, kern = [], {}, {}
    for wide in ([], ["--scalar-wide"]):
        for rnd in range(a.rounds):
            for part, extra in (("parent", ["--package-root", a.ab]), ("mode2", [])):
                for row in child(common + wide + ["--scalar-parts", part] + extra, None, [], a.deal_limit):
                    row.update(part=part, round=rnd)
                    key = (part, row["call"], row["bits"], row["n"], row["t"])
                    ms[key] = min(ms.get(key, row["whole_s"]), row["whole_s"])
                    if "scalar_kernel_ms" in row:
                        kern[key] = min(kern.get(key, row["scalar_kernel_ms"]), row["scalar_kernel_ms"])
                    lines.append(row)
    for bits in sorted({k[2] for k in ms}):
        for call in ("group_deal", "group_extract_shares"):
            shapes = sorted({k[3:] for k in ms if k[1] == call and k[2] == bits})
            ok = []
            for n, t in shapes:
                pa, m2 = ms["parent", call, bits, n, t], ms["mode2", call, bits, n, t]
                ok.append(m2 <= pa)
                lines.append({"what": "scalar_ab", "call": call, "bits": bits, "n": n, "t": t, "parent_whole_s": pa, "mode2_whole_s": m2,
                              "mode2_scalar_kernel_ms": kern.get(("mode2", call, bits, n, t)), "parent_over_mode2": round(pa / m2, 3)})
            if shapes:
                first = next((shapes[i][0] for i in range(len(shapes)) if all(ok[i:])), None)
                lines.append({"what": "scalar_crossover", "call": call, "bits": bits,
                              "min_shares": 1 if first == shapes[0][0] else first, "measured_shapes": shapes})
    for row in lines:
        if row["what"].startswith("scalar_"):
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


SHARE_HASH_SIZES = [1024, 4096, 65536]


def share_hash_leg(eng, a, rng):
    mode2 = a.share_hash_parts == "mode2"
    if mode2:
        eng.set_rt_share_hash(2)
    if a.share_hash_wide:
        import modp_rt_wide_helpers as WH
        groups, sizes = [(3072, ModpGroup(WH.group15(), elem_bytes=WH.EB), WH.EB)], [4096 if a.quick else 16384]
    else:
        groups = [(bits, ModpGroup(H.rfc_prime(bits)), 256) for bits in (1024, 2048)]
        sizes = SHARE_HASH_SIZES[:2] if a.quick else SHARE_HASH_SIZES

    def rb(n, bits, eb):
        return b"".join(rng.getrandbits(bits).to_bytes(eb, "big") for _ in range(n))

    def emit(call, bits, n, space, s):
        row = {"what": "share_hash", "call": call, "bits": bits, "n": n, "space": space, "whole_s": round(s, 5)}
        if mode2:
            row["hash_kernel_ms"] = round(max(0.0, eng.kernel_ms(5)), 3)
            row["hash_launches"] = eng.kernel_launches(5)
        print(json.dumps(row), flush=True)

    for bits, grp, eb in groups:
        for n in sizes:
            pk, s_, y, r = (rb(n, bits - 1, eb) for _ in range(4))
            c = rb(n, 256, eb)
            emit("group_verify_shares", bits, n, "host", best(lambda: eng.group_verify_shares(grp, pk, s_, y, c, r), a.reps))
            xi, w = rb(n, bits - 1, eb), rb(n, bits - 1, eb)
            emit("group_extract_shares", bits, n, "host", best(lambda: eng.group_extract_shares(grp, pk, y, xi, w), a.reps))
            if bits == 2048 and n == sizes[-1]:                 # the one device-space row: the five arrays are torch tensors
                import ctypes as C
                import torch
                dev = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in (pk, s_, y, c, r)]
                out = (C.c_uint8 * n)()
                torch.cuda.synchronize()

                def call():
                    rc = eng.lib.mpvss_modp_group_verify_shares(eng.ctx, grp.handle, capi.MPVSS_DEVICE, *(C.c_void_p(t.data_ptr()) for t in dev),
                                                                n, out)
                    assert rc == 0, eng.last_error()

                emit("group_verify_shares", bits, n, "device", best(call, a.reps))


def ab_share_hash(a):
    """--share-hash --ab PARENT: fresh processes of the parent build and of this build under mode 2 take turns; best of the rounds"""
    if not os.path.exists(os.path.join(a.ab, "mpvss_rs_amd", "libmpvss_hip.so")):
        sys.exit("modp_rt_rate --share-hash --ab: the parent checkout is not built")
    common = ["--legs", "share_hash", "--share-hash", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    lines, per_round, kern = [], {}, {}
    for wide in ([], ["--share-hash-wide"]):
        for rnd in range(a.rounds):
            for part, extra in (("parent", ["--package-root", a.ab]), ("mode2", [])):
                for row in child(common + wide + ["--share-hash-parts", part] + extra, None, [], a.deal_limit):
                    row.update(part=part, round=rnd)
                    key = (part, row["call"], row["bits"], row["space"], row["n"])
                    per_round.setdefault(key, []).append(row["whole_s"])
                    if "hash_kernel_ms" in row:
                        kern[key] = min(kern.get(key, row["hash_kernel_ms"]), row["hash_kernel_ms"])
                    lines.append(row)
    shapes = sorted({k[1:4] for k in per_round})
    for call, bits, space in shapes:
        sizes = sorted({k[4] for k in per_round if k[1:4] == (call, bits, space)})
        ok = []
        for n in sizes:
            pa, m2 = per_round["parent", call, bits, space, n], per_round["mode2", call, bits, space, n]
            spread = round(max(pa) - min(pa), 5)
            ok.append(min(m2) <= min(pa))
            lines.append({"what": "share_hash_ab", "call": call, "bits": bits, "space": space, "n": n, "parent_whole_s": min(pa),
                          "parent_rounds_s": pa, "parent_spread_s": spread, "mode2_whole_s": min(m2), "mode2_rounds_s": m2,
                          "mode2_hash_kernel_ms": kern.get(("mode2", call, bits, space, n)), "parent_over_mode2": round(min(pa) / min(m2), 3)})
            if n == 65536:
                lines.append({"what": "share_hash_gate", "call": call, "bits": bits, "space": space, "n": n,
                              "mode2_minus_parent_s": round(min(m2) - min(pa), 5), "parent_spread_s": spread,
                              "met": min(m2) <= min(pa) + spread})
        if space == "host":
            first = next((sizes[i] for i in range(len(sizes)) if all(ok[i:])), None)
            lines.append({"what": "share_hash_crossover", "call": call, "bits": bits, "min_shares": 1 if first == sizes[0] else first,
                          "measured_sizes": sizes})
    for row in lines:
        if row["what"].startswith("share_hash_"):
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


KEYSET_SIZES = [4096, 16384, 65536]


def keyset_leg(eng, a, rng):
    parts = a.keyset_parts.split(",")
    sizes = [4096] if a.quick else KEYSET_SIZES
    groups = [(1024, ModpGroup(H.rfc_prime(1024))), (2048, ModpGroup(H.rfc_prime(2048)))]
    if a.keyset_wide:
        import modp_rt_wide_helpers as WH
        groups, sizes = [(3072, ModpGroup(WH.group15(), elem_bytes=WH.EB))], [4096 if a.quick else 16384]
    for bits, grp in groups:
        EB = grp.elem_bytes

        def rb(n, nbits):
            return b"".join(rng.getrandbits(nbits).to_bytes(EB, "big") for _ in range(n))

        def timer(fn, k):
            ts = []
            for _ in range(a.reps + 1):
                fn()
                ts.append(round(max(0.0, eng.kernel_ms(k)), 3))
            return min(ts[1:])

        for n in sizes:
            y, Y, r, w = rb(n, bits - 1), rb(n, bits - 1), rb(n, bits - 1), rb(n, bits - 1)
            c, g1 = rb(1, 256), (4).to_bytes(EB, "big")
            pos, coef = list(range(1, n + 1)), rb(1, bits - 2)
            whole = n == 65536 and not a.keyset_wide
            t = 256
            cm = b"".join((rng.getrandbits(bits - 2) | 1).to_bytes(EB, "big") for _ in range(t)) if whole else None
            coefs = rb(t, bits - 2) if whole else None
            row = {"what": "keyset", "bits": bits, "n": n}
            if "parent" in parts:
                row["parent_a2_kernel_ms"] = timer(lambda: eng.group_dleq_commitments(grp, g1, Y, y, Y, r, c, False), 3)
                row["parent_twin_kernel_ms"] = timer(lambda: eng.group_deal(grp, coef, pos, y, w), 3)
                if whole:
                    row["verify_s"] = round(best(lambda: eng.group_verify_distribution(grp, cm, pos, y, Y, r, c), a.reps), 4)
                    row["deal_s"] = round(best(lambda: eng.group_deal(grp, coefs, pos, y, w), a.reps), 4)
            if "keyset" in parts:
                builds = []
                for _ in range(2):
                    ks = eng.group_keyset_create(grp, y)
                    builds.append(round(max(0.0, eng.kernel_ms(2)), 3))
                    if len(builds) < 2:
                        ks.close()
                row.update(keyset_build_kernel_ms=min(builds), keyset_bytes=ks.nbytes)
                row["keyset_a2_kernel_ms"] = timer(lambda: eng.group_keyset_dual_exp(grp, ks, 0, r, Y, c, False), 3)
                row["keyset_twin_kernel_ms"] = timer(lambda: eng.group_keyset_twin_exp(grp, ks, 0, r, w), 3)
                if whole:
                    row["verify_s"] = round(best(lambda: eng.group_verify_distribution_keyset(grp, cm, pos, ks, 0, Y, r, c), a.reps), 4)
                    row["deal_s"] = round(best(lambda: eng.group_deal_keyset(grp, coefs, pos, ks, 0, w), a.reps), 4)
                ks.close()
            print(json.dumps(row), flush=True)


def ab_keyset(a):
    """--keyset --ab PARENT: fresh processes of the parent build and of this build take turns; best of the rounds"""
    if not os.path.exists(os.path.join(a.ab, "mpvss_rs_amd", "libmpvss_hip.so")):
        sys.exit("modp_rt_rate --keyset --ab: the parent checkout is not built")
    common = ["--legs", "keyset", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    lines, ms = [], {}
    for wide in ([], ["--keyset-wide"]):
        for rnd in range(a.rounds):
            for part, extra in (("parent", ["--package-root", a.ab]), ("keyset", [])):
                for row in child(common + wide + ["--keyset-parts", part] + extra, None, [], a.deal_limit):
                    row.update(part=part, round=rnd)
                    for k, v in row.items():
                        if k.endswith("_kernel_ms") or k.endswith("_s") or k == "keyset_bytes":
                            key = (part + ":" + k, row["bits"], row["n"])
                            ms[key] = min(ms.get(key, v), v)
                    lines.append(row)
    for bits in sorted({k[1] for k in ms}):
        for n in sorted({k[2] for k in ms if k[1] == bits}):
            pa2, ka2 = ms["parent:parent_a2_kernel_ms", bits, n], ms["keyset:keyset_a2_kernel_ms", bits, n]
            ptw, ktw = ms["parent:parent_twin_kernel_ms", bits, n], ms["keyset:keyset_twin_kernel_ms", bits, n]
            row = {"what": "keyset_ab", "bits": bits, "n": n, "parent_a2_kernel_ms": pa2, "keyset_a2_kernel_ms": ka2,
                   "a2_parent_over_keyset": round(pa2 / ka2, 3), "parent_twin_kernel_ms": ptw, "keyset_twin_kernel_ms": ktw,
                   "twin_parent_over_keyset": round(ptw / ktw, 3),
                   "keyset_build_kernel_ms": ms["keyset:keyset_build_kernel_ms", bits, n], "keyset_bytes": ms["keyset:keyset_bytes", bits, n]}
            if ("parent:verify_s", bits, n) in ms:
                row.update(t=256, parent_verify_s=ms["parent:verify_s", bits, n], keyset_verify_s=ms["keyset:verify_s", bits, n],
                           parent_deal_s=ms["parent:deal_s", bits, n], keyset_deal_s=ms["keyset:deal_s", bits, n])
            lines.append(row)
            if (bits, n) == (2048, 65536):
                ratio = pa2 / ka2
                lines.append({"what": "keyset_gate", "bits": bits, "n": n, "a2_parent_over_keyset": round(ratio, 3), "counts_say": 3.65,
                              "required": 2.0, "met": ratio >= 2.0, "ships": ratio >= 1.0,
                              "twin_parent_over_keyset_not_gated": round(ptw / ktw, 3)})
    for row in lines:
        if row["what"].startswith("keyset_"):
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


def ab_fd(a):
    """--fd --ab PARENT: fresh processes of the parent build (Horner's rule) and of this build (mode 2 per chain count) take turns;
    best of the rounds.  rt_fd_chains is the best chain count per shape, rt_fd_min_shares the smallest measured n from which
    forward differences are no slower than the parent at every larger n; the gate: at most half of the parent's time at
    (65 536, 256) and 2048 bits."""
    if not os.path.exists(os.path.join(a.ab, "mpvss_rs_amd", "libmpvss_hip.so")):
        sys.exit("modp_rt_rate --fd --ab: the parent checkout is not built")
    common = ["--legs", "fd", "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    lines, ms = [], {}
    for wide in ([], ["--fd-wide"]):
        for rnd in range(a.rounds):
            for part, extra in (("parent", ["--package-root", a.ab]), ("fd", [])):
                for row in child(common + wide + ["--fd-parts", part] + extra, None, [], a.deal_limit):
                    row.update(part=part, round=rnd)
                    for k, v in row.items():
                        if k.endswith("_kernel_ms") or k == "verify_s":
                            key = (part + ":" + k, row["bits"], row["n"], row["t"])
                            ms[key] = min(ms.get(key, v), v)
                    lines.append(row)
    for bits in sorted({k[1] for k in ms}):
        shapes = sorted({k[2:] for k in ms if k[1] == bits})
        ok = []
        for n, t in shapes:
            horner = ms["parent:horner_kernel_ms", bits, n, t]
            fd = {ch: ms[f"fd:fd_chains_{ch}_kernel_ms", bits, n, t] for ch in FD_CHAINS}
            bestch = min(fd, key=fd.get)
            ok.append(fd[bestch] <= horner)
            row = {"what": "fd_ab", "bits": bits, "n": n, "t": t, "parent_horner_kernel_ms": horner, "fd_kernel_ms": fd,
                   "best_chains": bestch, "fd_over_horner": round(fd[bestch] / horner, 3)}
            if ("parent:verify_s", bits, n, t) in ms:
                row.update(parent_verify_s=ms["parent:verify_s", bits, n, t], change_mode2_verify_s=ms["fd:verify_s", bits, n, t])
            lines.append(row)
            if (bits, n, t) == (2048, 65536, 256):
                lines.append({"what": "fd_gate", "bits": bits, "n": n, "t": t, "fd_over_horner": round(fd[bestch] / horner, 3),
                              "required": 0.5, "met": fd[bestch] <= 0.5 * horner})
        first = next((shapes[i][0] for i in range(len(shapes)) if all(ok[i:])), None)
        lines.append({"what": "fd_crossover", "bits": bits, "min_shares": first, "measured_shapes": shapes})
    for row in lines:
        if row["what"].startswith("fd_"):
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(a.out, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")


def w4096_leg(eng, a, rng):
    """4096 bits (512-byte handle, 36 limbs per lane) beside 3072 bits (384 bytes, 27) in one session: kernels alone for
    group_batch_exp with full-width exponents, and whole group_verify_distribution calls (t = 64, challenge of 256 bits), at
    n = 1024 and 65536.  The last rows hold the ratios beside the count-derived expectation, (144/108)^2 x 4/3 = 2.37 per
    full-width exponentiation at equal occupancy -- which it is not: 1 wave per SIMD at 36 limbs per lane, 2 at 27."""
    import modp_rt_4096_helpers as XH
    import modp_rt_wide_helpers as WH
    sizes = [256, 1024] if a.quick else [1024, 65536]
    t = 64
    groups = [(3072, ModpGroup(WH.group15(), elem_bytes=WH.EB), WH.EB), (4096, ModpGroup(XH.group16(), elem_bytes=XH.EB), XH.EB)]
    rb = lambda n, bits, eb: b"".join(rng.getrandbits(bits).to_bytes(eb, "big") for _ in range(n))
    exp_ms, ver_s = {}, {}
    for bits, grp, eb in groups:
        for n in sizes:
            B, E = rb(n, bits, eb), rb(n, bits, eb)
            s = best(lambda: eng.group_batch_exp(grp, B, E), a.reps)
            kms = kernel_ms(eng)
            exp_ms[bits, n] = kms
            print(json.dumps({"what": "group_batch_exp", "bits": bits, "limbs_per_lane": grp.limbs_per_lane, "elem_bytes": eb, "n": n,
                              "s": round(s, 4), "kernel_ms": kms, "kernel_exps_per_s": round(n / (kms / 1e3))}), flush=True)
            cm, pos = rb(t, bits, eb), list(range(1, n + 1))
            y, Y, r = rb(n, bits, eb), rb(n, bits, eb), rb(n, bits, eb)
            c = rng.getrandbits(256).to_bytes(eb, "big")
            s = best(lambda: eng.group_verify_distribution(grp, cm, pos, y, Y, r, c), a.reps)
            ver_s[bits, n] = s
            print(json.dumps({"what": "group_verify_distribution", "bits": bits, "elem_bytes": eb, "n": n, "t": t, "s": round(s, 4),
                              "share_verifications_per_s": round(n / s), "kernel_ms": kernel_ms(eng)}), flush=True)
    for n in sizes:
        print(json.dumps({"what": "4096_over_3072", "n": n, "batch_exp_kernel_ms_ratio": round(exp_ms[4096, n] / exp_ms[3072, n], 2),
                          "verify_distribution_s_ratio": round(ver_s[4096, n] / ver_s[3072, n], 2),
                          "expected_per_exponentiation_at_equal_occupancy": round((144 / 108) ** 2 * 4 / 3, 2),
                          "waves_per_simd": {"3072": 2, "4096": 1}}), flush=True)


def row_leg(eng, a, rng):
    """The row layout for small calls (mpvss_ctx_set_rt_row) against the quad layout, modes 0 and 2 of the same library taking turns on
    one warm context (group_prepare done): (1) kernels alone (timer 3) of group_batch_exp with full-width exponents at 2048 / 3072 /
    4096 bits, (2) whole one-box calls at (5, 3) and (64, 22).  Median of --reps (5) after a warm-up of both modes; the results of both
    modes are compared before anything is timed."""
    import statistics
    import modp_rt_4096_helpers as XH
    import modp_rt_wide_helpers as WH
    sizes = [1, 64, 1024] if a.quick else [1, 64, 1024, 4096, 8192, 16384]
    shapes = [(5, 3)] if a.quick else [(5, 3), (64, 22)]
    reps = max(a.reps, 5)
    groups = [(2048, H.rfc_prime(2048), 256), (3072, WH.group15(), WH.EB), (4096, XH.group16(), XH.EB)]
    cat = lambda vals, eb: b"".join(v.to_bytes(eb, "big") for v in vals)
    lines = []

    def emit(row):
        lines.append(row)
        print(json.dumps(row), flush=True)

    def turns(call, figure):
        """{mode: median of figure() after call()} with the modes taking turns; call() gives equal results under both"""
        got = {}
        for mode in (0, 2):
            eng.set_rt_row(mode)
            got[mode] = call()
        assert got[0] == got[2], "the two layouts disagree"
        vals = {0: [], 2: []}
        for _ in range(reps):
            for mode in (0, 2):
                eng.set_rt_row(mode)
                t0 = time.perf_counter()
                call()
                vals[mode].append(figure(t0))
        eng.set_rt_row(0)
        return {m: statistics.median(v) for m, v in vals.items()}

    for bits, q, eb in groups:
        grp = ModpGroup(q, elem_bytes=eb) if eb != 256 else ModpGroup(q)
        eng.group_prepare(grp)
        rb = lambda n: b"".join(rng.getrandbits(bits).to_bytes(eb, "big") for _ in range(n))
        for n in sizes:
            B, E = rb(n), rb(n)
            med = turns(lambda: eng.group_batch_exp(grp, B, E), lambda t0: max(0.0, eng.kernel_ms(3)))
            emit({"what": "group_batch_exp_kernels", "bits": bits, "limbs_per_lane": grp.limbs_per_lane, "n": n,
                              "quad_kernel_ms": round(med[0], 3), "row_kernel_ms": round(med[2], 3),
                              "row_over_quad": round(med[2] / med[0], 3)})
        for n, t in shapes:
            pos = list(range(1, n + 1))
            privs = [rng.randrange(3, q - 1) | 1 for _ in range(n)]
            xinv = cat([pow(k, -1, q - 1) for k in privs], eb)
            pks = eng.group_batch_exp_fixed_base(grp, cat([2], eb), cat(privs, eb))
            coeffs, ws, w2 = rb(t), rb(n), rb(n)
            cm = eng.group_batch_exp_fixed_base(grp, cat([4], eb), coeffs)
            box = eng.group_deal(grp, coeffs, pos, pks, ws)
            S, Cs = eng.group_extract_shares(grp, pks, box["Y"], xinv, w2)
            R = capi.group_dleq_responses(grp, w2, cat(privs, eb), Cs)
            calls = {
                "group_verify_distribution": lambda: eng.group_verify_distribution(grp, cm, pos, pks, box["Y"], box["responses"], box["challenge"]),
                "group_deal": lambda: eng.group_deal(grp, coeffs, pos, pks, ws),
                "group_extract_shares": lambda: eng.group_extract_shares(grp, pks, box["Y"], xinv, w2),
                "group_verify_shares": lambda: bytes(eng.group_verify_shares(grp, pks, S, box["Y"], Cs, R)),
            }
            for what, call in calls.items():
                med = turns(call, lambda t0: (time.perf_counter() - t0) * 1e3)
                emit({"what": what, "bits": bits, "n": n, "t": t, "quad_ms": round(med[0], 3), "row_ms": round(med[2], 3),
                                  "row_over_quad": round(med[2] / med[0], 3)})
        grp.close()
    with open(a.out, "w") as f:
        f.write("# tools/modp_rt_rate.py --row: set_rt_row modes 0 (quad layout) and 2 (row layout) of one library in turns on one warm\n"
                "# context, median of %d after a warm-up of both; kernel_ms = timer 3 of group_batch_exp, full-width exponents; *_ms of the\n"
                "# one-box calls = wall time of the whole call from host buffers\n" % reps)
        for row in lines:
            f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="smaller shapes (a check of the tool, not a measurement)")
    ap.add_argument("--legs", default="rates", help="comma-separated: rates (batch_exp, verify), twin, deal, w4096 (4096 beside 3072 bits)")
    ap.add_argument("--twin-parts", default="call,baseline", help="of the twin leg: call (batch_twin_exp), baseline (two batch_exp)")
    ap.add_argument("--comb", action="store_true", help="the fixed-base comb: alone, the comb leg; with --ab, its interleaved A/B")
    ap.add_argument("--comb-parts", default="comb", help="of the comb leg: parent (g^w inside group_deal), comb (cold and warm)")
    ap.add_argument("--fd", action="store_true", help="forward differences for X: alone, the fd leg; with --ab, its interleaved A/B")
    ap.add_argument("--fd-parts", default="fd", help="of the fd leg: parent (Horner's rule of the library under test), fd (mode 2 per chain count)")
    ap.add_argument("--fd-wide", action="store_true", help="of the fd leg: the one 3072-bit row, (16384, 128)")
    ap.add_argument("--scalar", action="store_true", help="the scalar ring on the device: alone, the scalar leg; with --ab, its interleaved A/B")
    ap.add_argument("--scalar-parts", default="mode2", help="of the scalar leg: parent (the library under test as it is), mode2 (set_rt_scalar(2))")
    ap.add_argument("--scalar-wide", action="store_true", help="of the scalar leg: the one 3072-bit row, group_deal at (4096, 64)")
    ap.add_argument("--keyset", action="store_true", help="key sets of a run-time group: alone, the keyset leg; with --ab, its interleaved A/B")
    ap.add_argument("--keyset-parts", default="keyset", help="of the keyset leg: parent (the launches without a set), keyset (build and launches over a set)")
    ap.add_argument("--keyset-wide", action="store_true", help="of the keyset leg: the one 3072-bit row, n = 16384")
    ap.add_argument("--share-hash", action="store_true", help="the per-share hash on the device: alone, the share-hash leg; with --ab, its interleaved A/B")
    ap.add_argument("--share-hash-parts", default="mode2", help="of the share-hash leg: parent (the library under test as it is), mode2 (set_rt_share_hash(2))")
    ap.add_argument("--share-hash-wide", action="store_true", help="of the share-hash leg: the one 3072-bit row, n = 16384")
    ap.add_argument("--row", action="store_true", help="the row layout for small calls: modes 0 and 2 of set_rt_row in turns (profiles/modp_rt_row_rate.txt)")
    ap.add_argument("--package-root", default=None, help="import mpvss_rs_amd (bindings and library) from this checkout")
    ap.add_argument("--ab", default=None, metavar="PARENT", help="the interleaved A/B against a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2, help="of --ab: how often the three processes take turns")
    ap.add_argument("--twin-limit", type=int, default=300, help="of --ab: seconds one twin-leg process may take")
    ap.add_argument("--deal-limit", type=int, default=900, help="of --ab: seconds the deal-leg process may take (host threads at (65536, 256))")
    ap.add_argument("--out", default=None, help="of --ab: the file written (profiles/modp_rt_deal_rate.txt, or _comb_rate.txt)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "modp_rt_row_rate.txt" if a.row else "modp_rt_share_hash_rate.txt" if a.share_hash else "modp_rt_keyset_rate.txt" if a.keyset else "modp_rt_scalar_rate.txt" if a.scalar else "modp_rt_fd_rate.txt" if a.fd else "modp_rt_comb_rate.txt" if a.comb else "modp_rt_deal_rate.txt")
    if a.ab:
        return ab_share_hash(a) if a.share_hash else ab_keyset(a) if a.keyset else ab_scalar(a) if a.scalar else ab_fd(a) if a.fd else ab_comb(a) if a.comb else ab(a)
    if a.comb:
        a.legs = "comb"
    if a.fd:
        a.legs = "fd"
    if a.scalar:
        a.legs = "scalar"
    if a.keyset:
        a.legs = "keyset"
    if a.row:
        a.legs = "row"
    if a.share_hash:
        a.legs = "share_hash"
        import torch  # noqa: F401  (its own HIP runtime must be loaded before the library's, for the device-space row)
    load_package(a.package_root)
    eng = Engine(0)
    rng = random.Random(1)
    legs = a.legs.split(",")
    if "twin" in legs:
        twin_leg(eng, a, rng)
    if "deal" in legs:
        deal_leg(eng, a, rng)
    if "comb" in legs:
        comb_leg(eng, a, rng)
    if "verify" in legs:
        verify_leg(eng, a, rng)
    if "fd" in legs:
        fd_leg(eng, a, rng)
    if "scalar" in legs:
        scalar_leg(eng, a, rng)
    if "keyset" in legs:
        keyset_leg(eng, a, rng)
    if "share_hash" in legs:
        share_hash_leg(eng, a, rng)
    if "w4096" in legs:
        w4096_leg(eng, a, rng)
    if "row" in legs:
        row_leg(eng, a, rng)
    if "rates" not in legs:
        eng.close()
        return
    n = 4096 if a.quick else 65536
    moduli = {512: H.small_safe_primes()[512], 1024: H.rfc_prime(1024), 1536: H.rfc_prime(1536), 2048: H.rfc_prime(2048)}
    rates = {}
    for bits, q in moduli.items():
        grp = ModpGroup(q)
        B, E = rand_bytes(rng, n, 2048), rand_bytes(rng, n, bits)
        s = best(lambda: eng.group_batch_exp(grp, B, E), a.reps)
        kms = kernel_ms(eng)
        rates[bits] = n / (kms / 1e3)
        print(json.dumps({"what": "group_batch_exp", "bits": bits, "limbs_per_lane": grp.limbs_per_lane, "n": n,
                          "s": round(s, 4), "exps_per_s": round(n / s), "kernel_ms": kms,
                          "kernel_exps_per_s": round(rates[bits])}), flush=True)
    B, E = rand_bytes(rng, n, 2048), rand_bytes(rng, n, 2048)
    s = best(lambda: eng.batch_exp(B, E), a.reps)
    kms = kernel_ms(eng)
    print(json.dumps({"what": "group14_batch_exp", "bits": 2048, "n": n, "s": round(s, 4), "exps_per_s": round(n / s),
                      "kernel_ms": kms, "kernel_exps_per_s": round(n / (kms / 1e3)),
                      "kernel_runtime_2048_over_group14": round(rates[2048] / (n / (kms / 1e3)), 3),
                      "kernel_runtime_1024_over_2048": round(rates[1024] / rates[2048], 2),
                      "kernel_runtime_512_over_2048": round(rates[512] / rates[2048], 2)}), flush=True)
    shapes = [(4096, 64), (8192, 64)] if a.quick else [(4096, 64), (65536, 256)]
    for bits in (1024, 1536, 2048):
        grp = ModpGroup(moduli[bits])
        for nn, t in shapes:
            cm = rand_bytes(rng, t, bits)
            pos = list(range(1, nn + 1))
            y, Y, r = rand_bytes(rng, nn, bits), rand_bytes(rng, nn, bits), rand_bytes(rng, nn, bits)
            c = rng.getrandbits(min(bits - 2, 256)).to_bytes(256, "big")
            s = best(lambda: eng.group_verify_distribution(grp, cm, pos, y, Y, r, c), a.reps)
            print(json.dumps({"what": "group_verify_distribution", "bits": bits, "n": nn, "t": t, "s": round(s, 4),
                              "share_verifications_per_s": round(nn / s), "kernel_ms": kernel_ms(eng)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
