"""Rates of the key sets of the curve groups (include/mpvss_hip.h, "Key sets of a curve group") beside the calls that take the keys
as an array, on one GPU.

For each curve and each n (default 65536 and 1024) ONE fresh child process measures, the two variants of every pair taking turns
round by round (array, key set, array, key set, ...) after one warm-up round of both:

  build     mpvss_ec_keyset_create from host keys: time and the set's bytes (the build is not part of any figure below)
  powers    mpvss_ec_keyset_twin_exp against two mpvss_ec_batch_exp calls over the same keys, host buffers in and out:
            whole calls (host clock; the calls end in a device synchronise) and the kernels' own time inside them
  blocks    16 dealer's blocks in flight, t = 256, device buffers: mpvss_ec_deal_compute_keyset against mpvss_ec_deal_compute,
            enqueue all, absorb all; shares per second of the whole window (blocks), and of the device's part of it alone:
            enqueue all, wait for the GPU, then absorb outside the figure (blocks_gpu_part)
  deal      one mpvss_ec_deal_keyset call against one mpvss_ec_deal call, t = 256 (t = n below 256), host buffers

The baseline of every pair is the array path of the SAME library.  Every child runs under a time limit of its own and the tool
stops at the first child that fails.  One JSON line per measurement: best and median of the rounds and the ratio of the medians.
Usage: python tools/ec_keyset_rate.py [--sizes 65536,1024] [--rounds 7] [--out profiles/ec_keyset_rate.txt]"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

NAMES = {"secp256k1": 1, "ristretto255": 2}
BLOCKS = 16
CHILD_LIMIT_S = 420


def kernel_ms(eng):
    return round(sum(max(0.0, eng.kernel_ms(k)) for k in range(4)), 3)


def take_turns(variants, rounds):
    """variants: [(tag, fn)], fn() -> optional extra figure; one warm-up round, then `rounds` rounds in which the variants alternate.
    {tag: {"ms": [...], "extra": [...]}}"""
    for _, fn in variants:
        fn()
    out = {tag: {"ms": [], "extra": []} for tag, _ in variants}
    for _ in range(rounds):
        for tag, fn in variants:
            t0 = time.perf_counter()
            extra = fn()
            out[tag]["ms"].append((time.perf_counter() - t0) * 1e3)
            out[tag]["extra"].append(extra)
    return out


def summary(ms):
    return {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "worst_ms": round(max(ms), 3)}


def child(name, n, rounds):
    import torch
    import mpvss_oracle as O
    from mpvss_rs_amd import Engine, capi

    gid = NAMES[name]
    G = O.GROUPS[name]()
    order, L = G.group_order_int(), G.elem_len
    sb = G.scalar_to_fixed
    rng = random.Random(1000 * gid + n)
    rs = lambda count, lo=0: b"".join(sb(rng.randrange(lo, order)) for _ in range(count))
    eng = Engine(0)
    keys = eng.ec_batch_exp_generator(gid, rs(n, 1))
    lines = []

    def emit(what, **kw):
        d = dict(curve=name, n=n, what=what, rounds=rounds, **kw)
        lines.append(d)
        print(json.dumps(d), flush=True)

    # build
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        ks = eng.ec_keyset_create(gid, keys)
        ms.append((time.perf_counter() - t0) * 1e3)
        nbytes = ks.nbytes
        ks.close()
    emit("build", set_bytes=nbytes, keys_per_s=round(n / (min(ms) / 1e3)), **summary(ms))
    ks = eng.ec_keyset_create(gid, keys)

    def ratio(r, base, new):
        return round(statistics.median(r[base]["ms"]) / statistics.median(r[new]["ms"]), 3)

    # powers
    e1, e2 = rs(n), rs(n)
    results = {}

    def array_powers():
        a = eng.ec_batch_exp(gid, keys, e1)
        k = kernel_ms(eng)
        b = eng.ec_batch_exp(gid, keys, e2)
        results["array"] = (a, b)
        return k + kernel_ms(eng)

    def keyset_powers():
        results["keyset"] = eng.ec_keyset_twin_exp(gid, ks, 0, e1, e2)
        return kernel_ms(eng)

    r = take_turns([("array", array_powers), ("keyset", keyset_powers)], rounds)
    assert results["array"] == results["keyset"], "twin_exp differs from two batch_exp calls"
    emit("powers", array=summary(r["array"]["ms"]), keyset=summary(r["keyset"]["ms"]), speedup_whole_calls=ratio(r, "array", "keyset"),
         array_kernels_ms=round(statistics.median(r["array"]["extra"]), 3), keyset_kernels_ms=round(statistics.median(r["keyset"]["extra"]), 3),
         speedup_kernels=round(statistics.median(r["array"]["extra"]) / statistics.median(r["keyset"]["extra"]), 3))

    # dealer blocks
    t = min(256, n)
    coeffs = rs(t)
    wits = rs(n, 1)
    pos = list(range(1, n + 1))
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")
    d_pos = torch.tensor(pos, dtype=torch.int64, device="cuda:0")
    d_pk, d_w = dev(keys), dev(wits)
    d_p = [torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0") for _ in range(BLOCKS)]
    torch.cuda.synchronize()
    digests = {}

    def blocks(form, drain):
        """drain: wait for the GPU before the first absorb and return that time -- the device's share of the window, without the
        host's transcript hash (one thread here) that the absorbs add"""
        def run():
            t0 = time.perf_counter()
            for k in range(BLOCKS):
                if form == "array":
                    eng.ec_deal_compute(gid, coeffs, d_pos.data_ptr(), d_pk.data_ptr(), d_w.data_ptr(), n, d_p[k].data_ptr())
                else:
                    eng.ec_deal_compute_keyset(gid, coeffs, d_pos.data_ptr(), ks, 0, d_w.data_ptr(), n, d_p[k].data_ptr())
            gpu_ms = None
            if drain:
                eng._check(eng.lib.mpvss_ctx_synchronize(eng.ctx), "ctx_synchronize")
                gpu_ms = (time.perf_counter() - t0) * 1e3
            for k in range(BLOCKS):
                st = eng.ec_distribute_absorb(gid, capi.transcript_init(), n)[0]
            digests[form] = capi.ec_transcript_verdict(gid, st, bytes(32))[1]
            return gpu_ms
        return run

    r = take_turns([("array", blocks("array", False)), ("keyset", blocks("keyset", False))], rounds)
    assert digests["array"] == digests["keyset"], "the key-set blocks hash to another digest"
    per_s = lambda tag: round(BLOCKS * n / (statistics.median(r[tag]["ms"]) / 1e3))
    emit("blocks", blocks_in_flight=BLOCKS, t=t, array=summary(r["array"]["ms"]), keyset=summary(r["keyset"]["ms"]),
         array_shares_per_s=per_s("array"), keyset_shares_per_s=per_s("keyset"), speedup=ratio(r, "array", "keyset"))
    r = take_turns([("array", blocks("array", True)), ("keyset", blocks("keyset", True))], rounds)
    g = {tag: r[tag]["extra"] for tag in r}
    per_s = lambda tag: round(BLOCKS * n / (statistics.median(g[tag]) / 1e3))
    emit("blocks_gpu_part", blocks_in_flight=BLOCKS, t=t, array=summary(g["array"]), keyset=summary(g["keyset"]),
         array_shares_per_s=per_s("array"), keyset_shares_per_s=per_s("keyset"),
         speedup=round(statistics.median(g["array"]) / statistics.median(g["keyset"]), 3))

    # one-call dealer
    call_a, out_a = eng.ec_deal_call(gid, coeffs, pos, keys, wits)
    call_k, out_k = eng.ec_deal_keyset_call(gid, coeffs, pos, ks, 0, wits)
    r = take_turns([("array", call_a), ("keyset", call_k)], rounds)
    assert out_a() == out_k(), "deal_keyset differs from deal"
    per_s = lambda tag: round(n / (statistics.median(r[tag]["ms"]) / 1e3))
    emit("deal", t=t, array=summary(r["array"]["ms"]), keyset=summary(r["keyset"]["ms"]), array_shares_per_s=per_s("array"),
         keyset_shares_per_s=per_s("keyset"), speedup=ratio(r, "array", "keyset"))
    ks.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ec_keyset_rate.txt"))
    ap.add_argument("--child", nargs=2, metavar=("CURVE", "N"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.rounds)
        return 0
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "8")          # the block pipeline's setting
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        for name in NAMES:
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds),
                   "--child", name, str(n)]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env)
            lines += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.stderr.write("\nec_keyset_rate: %s n = %d ended with status %d; nothing further is started\n" % (name, n, p.returncode))
                return 1
    head = ["# tools/ec_keyset_rate.py: key sets of the curve groups beside the array calls of the same library, one MI355X.",
            "# One fresh process per (curve, n); in every pair the variants take turns, %d rounds after a warm-up round; times in ms." % a.rounds,
            "# speedup = median of the array variant / median of the key-set variant."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
