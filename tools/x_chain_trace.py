#!/usr/bin/env python3
"""The serial chain of a box's X path from a rocprofv3 --kernel-trace CSV of `python bench.py --gpus 1`.

  tools/x_chain_trace.py KERNEL_TRACE.csv [--line LINE.json] [--last 24] [--queues N]

Every slot of the verifier puts its X path on its own high-priority stream (eval_x in mpvss_capi.cpp): Horner seeds, an
inversion tree (with a host round trip), the one-chain difference table and the stride-1 seeding chain (level 1), a second
tree, the S-chain table and the stepping (level 2), then from_mont, X's odd-power table and a1.  This walks each stream's
kernels in launch order, cuts them into those phases and prints, for the last `--last` boxes (the timed steps of a plain run):
the span from the first X-path kernel to the end of a1, the phases, how many stepping launches and how many X paths are on
the chip at the same time, and -- given the run's JSON line -- chain / (chains open at once) against ms_per_step.

A box among others hands its tail (X's table, a1, the copies) to another stream of its slot.  The CHAIN of a box is what holds
its first stream's hardware queue: first X-path kernel to the end of the last kernel of the box on that stream (from_mont and the
gated Horner fall-back when the tail is elsewhere; a1 when it is not, as in traces of earlier revisions, which parse as before).
The TAIL -- end of the level-2 stepping to the end of a1 -- is reported beside it with the stream and queue it ran on, found as a
table build directly followed by an a1 kernel on another stream, between this box's chain and the next box of the same stream.
"Open at once" counts chains.
"""
import argparse
import csv
import json
import statistics as st

TREE = ("binv", "from_mont", "to_mont", "apply_ok", "gather", "rocclr")      # rocclr: the copies of the root to the host and back


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append({"name": r["Kernel_Name"], "s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]),
                     "stream": r.get("Stream_Id", r.get("Queue_Id")), "queue": r.get("Queue_Id"),
                     "grid": int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)})
    rows.sort(key=lambda r: r["s"])
    return rows


def is_a1(nm):
    """a1 = g^r X^c: the comb kernel, or the pair layout's scheduled power times g^r (a2's kernels are call_rows_ / w6 / keyset ones)"""
    return "comb_dual_exp" in nm or "exp_mul" in nm


def attach_tails(rows, boxes, detached):
    """the tails of chains whose stream does not hold them: (build_table, a1) pairs on other streams.  A slot pairs one first stream
    with one tail stream, and a slot serves one box at a time: the tail stream of a first stream is the one that has exactly one
    pair between each of its chains and the next box there; failing that, the earliest unclaimed pair behind the chain."""
    if not detached:
        return
    firsts = {b["stream"] for b in boxes} | {b["stream"] for b in detached}
    by_stream = {}
    for r in rows:
        by_stream.setdefault(r["stream"], []).append(r)
    pairs = {}
    for stream, ks in by_stream.items():
        if stream in firsts:
            continue
        for a, b in zip(ks, ks[1:]):
            if "build_table" in a["name"] and is_a1(b["name"]):
                pairs.setdefault(stream, []).append({"s": a["s"], "e": b["e"], "ks": [a, b], "stream": stream, "queue": b["queue"], "used": False})
    inf = float("inf")
    window = lambda c: (c["chain_end"], c.get("next_on_stream", inf))
    inside = lambda p, c: p["s"] >= window(c)[0] and p["e"] <= window(c)[1]
    by_first = {}
    for c in detached:
        by_first.setdefault(c["stream"], []).append(c)
    for first, chains in by_first.items():
        best = None
        for stream, ps in pairs.items():
            hits = [[p for p in ps if not p["used"] and inside(p, c)] for c in chains]
            if all(len(h) == 1 for h in hits):
                delay = sum(h[0]["s"] - c["chain_end"] for h, c in zip(hits, chains))
                if best is None or delay < best[0]:
                    best = (delay, [h[0] for h in hits])
        for i, c in enumerate(chains):
            p = best[1][i] if best else min((p for ps in pairs.values() for p in ps if not p["used"] and p["s"] >= c["chain_end"]),
                                            key=lambda p: p["s"], default=None)
            if p is None:
                continue                                  # (a chain at the very end of the trace)
            p["used"] = True
            c["tail"] = c["tail"] + p["ks"]
            c["a1_kernel"], c["end"] = p["ks"][1]["name"], p["e"]
            c["tail_stream"], c["tail_queue"] = p["stream"], p["queue"]
            boxes.append(c)


def cut_boxes(rows):
    """state machine over one stream's kernels -> list of boxes {phase: (start, end)}, trees with their largest inner gap"""
    boxes, detached = [], []
    by_stream = {}
    for r in rows:
        by_stream.setdefault(r["stream"], []).append(r)
    for stream, ks in by_stream.items():
        state, cur = "idle", None
        for k in ks:
            nm = k["name"]
            if state in ("idle", "tree1") and "commit_eval" in nm:
                cur = {"stream": stream, "queue": k["queue"], "horner": (k["s"], k["e"]), "horner_kernel": nm, "tree1": [], "tree2": [], "tail": []}
                state = "tree1"
            elif state == "tree1":
                if "fd_table" in nm:
                    cur["l1_table"], state = (k["s"], k["e"]), "l1step"
                elif any(x in nm for x in TREE):
                    cur["tree1"].append(k)
                else:
                    state, cur = "idle", None            # Horner for every share: no chain to look at
            elif state == "l1step" and "fd_step" in nm:
                cur["l1_step"], state = (k["s"], k["e"]), "tree2"
            elif state == "tree2":
                if "fd_table" in nm:
                    cur["l2_table"], state = (k["s"], k["e"]), "l2step"
                elif any(x in nm for x in TREE) and k["grid"] < 65536:
                    cur["tree2"].append(k)
                else:                                     # one level only (a box that had the chip to itself): not a pipelined box
                    state, cur = "idle", None
            elif state == "l2step" and "fd_step" in nm:
                cur["l2_step"], state = (k["s"], k["e"]), "tail"
            elif state == "tail":
                if is_a1(nm):                             # the whole box on one stream
                    cur["tail"].append(k)
                    cur["a1_kernel"] = nm
                    cur["end"] = cur["chain_end"] = k["e"]
                    cur["tail_stream"], cur["tail_queue"] = stream, k["queue"]
                    boxes.append(cur)
                    state, cur = "idle", None
                elif "from_mont" in nm or "build_table" in nm or ("commit_eval" in nm and "row" not in nm and not cur.get("gated")):
                    cur["gated"] = cur.get("gated", False) or "commit_eval" in nm
                    cur["tail"].append(k)
                else:                                     # something else's kernel: this box's tail is on another stream
                    cur["chain_end"] = cur["tail"][-1]["e"] if cur["tail"] else cur["l2_step"][1]
                    cur["next_on_stream"] = k["s"]
                    detached.append(cur)
                    state, cur = "idle", None
                    if "commit_eval" in nm:               # (the next box's seeds at once)
                        cur = {"stream": stream, "queue": k["queue"], "horner": (k["s"], k["e"]), "horner_kernel": nm, "tree1": [], "tree2": [],
                               "tail": []}
                        state = "tree1"
        if state == "tail":                               # the trace ends behind this chain
            cur["chain_end"] = cur["tail"][-1]["e"] if cur["tail"] else cur["l2_step"][1]
            detached.append(cur)
    attach_tails(rows, boxes, detached)
    boxes.sort(key=lambda b: b["end"])
    return boxes


def tree_gap(before_end, ks, after_start):
    edges = [before_end] + [x for k in ks for x in (k["s"], k["e"])] + [after_start]
    return max((edges[i + 1] - edges[i] for i in range(0, len(edges), 2)), default=0)


def concurrency(intervals, lo, hi):
    """time-weighted median, mean and maximum of the number of intervals open, over the time inside [lo, hi] at which any is"""
    ev = []
    for s, e in intervals:
        s, e = max(s, lo), min(e, hi)
        if e > s:
            ev += [(s, 1), (e, -1)]
    ev.sort()
    hist, n, prev = {}, 0, None
    for tme, d in ev:
        if prev is not None and n > 0:
            hist[n] = hist.get(n, 0) + tme - prev
        n += d
        prev = tme
    total = sum(hist.values())
    if not total:
        return 0, 0.0, 0
    acc, med = 0, 0
    for lvl in sorted(hist):
        acc += hist[lvl]
        if acc * 2 >= total:
            med = lvl
            break
    return med, sum(k * v for k, v in hist.items()) / total, max(hist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--line", help="the run's JSON line (ms_per_step, value)")
    ap.add_argument("--last", type=int, default=24, help="boxes looked at: the last ones to finish (the timed steps)")
    ap.add_argument("--l1-steps", type=int, default=0, help="serial steps of the level-1 stepping launch (for us per step)")
    ap.add_argument("--l2-steps", type=int, default=0, help="serial steps of the level-2 stepping launch")
    ap.add_argument("--queues", default="?", help="GPU_MAX_HW_QUEUES of the run, for the header")
    a = ap.parse_args()
    rows = load(a.csv)
    boxes = cut_boxes(rows)
    timed = boxes[-a.last:]
    if not timed:
        raise SystemExit("no two-level X path found in the trace")
    ms = lambda ns: ns / 1e6
    lo, hi = min(b["horner"][0] for b in timed), max(b["end"] for b in timed)
    print(f"GPU_MAX_HW_QUEUES={a.queues}   kernels={len(rows)}   two-level X paths found={len(boxes)}   looked at: the last {len(timed)}")
    print(f"seed kernel: {timed[-1]['horner_kernel'][:40]}   a1 kernel: {timed[-1]['a1_kernel'][:40]}")
    print(f"streams of those boxes: {len({b['stream'] for b in timed})}   hardware queues they ran on: {len({b['queue'] for b in timed})}")
    moved = [b for b in timed if b["tail_stream"] != b["stream"]]
    print(f"tails on another stream than their chain: {len(moved)} of {len(timed)}"
          + (f"   tail streams: {len({b['tail_stream'] for b in moved})}   hardware queues the tails ran on: {len({b['tail_queue'] for b in moved})}"
             if moved else ""))
    cols = ("chain", "span", "horner", "tree1", "gap1", "l1_tab", "l1_step", "tree2", "gap2", "l2_tab", "l2_step", "tail", "run", "wait")
    table = []
    for b in timed:
        t1 = b["l1_table"][0] - b["horner"][1]
        t2 = b["l2_table"][0] - b["l1_step"][1]
        table.append({"chain": ms(b["chain_end"] - b["horner"][0]), "span": ms(b["end"] - b["horner"][0]), "horner": ms(b["horner"][1] - b["horner"][0]), "tree1": ms(t1),
                      "gap1": ms(tree_gap(b["horner"][1], b["tree1"], b["l1_table"][0])),
                      "l1_tab": ms(b["l1_step"][0] - b["l1_table"][0]), "l1_step": ms(b["l1_step"][1] - b["l1_step"][0]),
                      "tree2": ms(t2), "gap2": ms(tree_gap(b["l1_step"][1], b["tree2"], b["l2_table"][0])),
                      "l2_tab": ms(b["l2_step"][0] - b["l2_table"][0]), "l2_step": ms(b["l2_step"][1] - b["l2_step"][0]),
                      "tail": ms(b["end"] - b["l2_step"][1])})
        run = sum(e - s_ for s_, e in (b["horner"], b["l1_table"], b["l1_step"], b["l2_table"], b["l2_step"]))
        run += sum(k["e"] - k["s"] for k in b["tree1"] + b["tree2"] + b["tail"])
        table[-1]["run"] = ms(run)
        table[-1]["wait"] = table[-1]["span"] - ms(run)
    print("\nper box, ms (chain: first X-path kernel to the end of the box's last kernel on that stream = what holds its hardware queue;")
    print("tail: end of the level-2 stepping to the end of a1, with the stream / queue it ran on behind the row;")
    print("span: first X-path kernel to the end of a1; tree1/tree2: end of the phase before to the start of the table launch,")
    print("gap1/gap2: the longest pause between two kernels inside it = the host round trip; l*_tab: table launch up to the start of the stepping;")
    print("run: sum of the durations of the box's X-path kernels; wait = span - run: time in which none of them was on the chip)")
    print(" box " + " ".join(f"{c:>8}" for c in cols))
    for i, row in enumerate(table):
        print(f"{i:4d} " + " ".join(f"{row[c]:8.2f}" for c in cols) + f"   {timed[i]['tail_stream']}/{timed[i]['tail_queue']}"
              + ("" if timed[i]["tail_stream"] != timed[i]["stream"] else " (chain's)"))
    print("\n med " + " ".join(f"{st.median(r[c] for r in table):8.2f}" for c in cols))
    print(" min " + " ".join(f"{min(r[c] for r in table):8.2f}" for c in cols))
    print(" max " + " ".join(f"{max(r[c] for r in table):8.2f}" for c in cols))
    print(f"tail: median {st.median(r['tail'] for r in table):.2f}, mean {st.mean(r['tail'] for r in table):.2f} ms")
    # what the queue gains: from the end of a box's stepping to the next seed kernel on the same hardware queue
    seeds = sorted((b["horner"][0], b["queue"]) for b in boxes)
    waits = []
    for b in timed:
        nxt = [s_ for s_, q in seeds if q == b["queue"] and s_ > b["l2_step"][1]]
        if nxt:
            waits.append(ms(nxt[0] - b["l2_step"][1]))
    if waits:
        print(f"end of the stepping to the next box's seed kernel on the same queue: median {st.median(waits):.2f}, mean {st.mean(waits):.2f} ms"
              f" ({len(waits)} boxes)")
    if a.l1_steps:
        print(f"level-1 stepping: {a.l1_steps} serial steps, median {st.median(r['l1_step'] for r in table) * 1e3 / a.l1_steps:.2f} us per step")
    if a.l2_steps:
        print(f"level-2 stepping: {a.l2_steps} serial steps, median {st.median(r['l2_step'] for r in table) * 1e3 / a.l2_steps:.2f} us per step")
    steps = [(r["s"], r["e"]) for r in rows if "fd_step" in r["name"]]
    med, mean, mx = concurrency(steps, lo, hi)
    print(f"\nk_modp_fd_step launches on the chip at once (time-weighted, while any runs): median {med}, mean {mean:.2f}, maximum {mx}")
    xmed, xmean, xmx = concurrency([(b["horner"][0], b["chain_end"]) for b in boxes], lo, hi)
    print(f"chains (first kernel .. last kernel on the chain's stream) open at once: median {xmed}, mean {xmean:.2f}, maximum {xmx}")
    span = st.median(r["chain"] for r in table)
    print(f"rate of the timed window from the trace: {ms(hi - lo) / len(timed):.2f} ms per box")
    if a.line:
        line = json.loads([l for l in open(a.line) if l.startswith("{")][-1])
        per = line["ms_per_step"]
        ratio = span / max(xmean, 1e-9) / per
        print(f"value {line['value']:.0f}   ms_per_step {per:.2f}")
        print(f"chain / chains open at once = {span:.1f} / {xmean:.2f} = {span / xmean:.2f} ms against ms_per_step {per:.2f}: ratio {ratio:.2f}")
        print("verdict: " + ("within 20 %: the chain binds -- a box cannot come sooner than its chain's span over the chains that advance at once"
                             if 0.8 <= ratio <= 1.2 else "not within 20 %: the chain does not bind by this measure (the chip is issue-bound)"))


if __name__ == "__main__":
    main()
