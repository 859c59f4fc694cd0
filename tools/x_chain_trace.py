#!/usr/bin/env python3
"""The serial chain of a box's X path from a rocprofv3 --kernel-trace CSV of `python bench.py --gpus 1`.

  tools/x_chain_trace.py KERNEL_TRACE.csv [--line LINE.json] [--last 24] [--queues N]

Every slot of the verifier puts its X path on its own high-priority stream (eval_x in mpvss_capi.cpp): Horner seeds, an
inversion tree (with a host round trip), the one-chain difference table and the stride-1 seeding chain (level 1), a second
tree, the S-chain table and the stepping (level 2), then from_mont, X's odd-power table and a1.  This walks each stream's
kernels in launch order, cuts them into those phases and prints, for the last `--last` boxes (the timed steps of a plain run):
the span from the first X-path kernel to the end of a1, the phases, how many stepping launches and how many X paths are on
the chip at the same time, and -- given the run's JSON line -- span / (overlapping X paths) against ms_per_step.
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


def cut_boxes(rows):
    """state machine over one stream's kernels -> list of boxes {phase: (start, end)}, trees with their largest inner gap"""
    boxes = []
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
                cur["tail"].append(k)
                if "dual_exp" in nm or "exp_mul" in nm:
                    cur["a1_kernel"] = nm
                    cur["end"] = k["e"]
                    boxes.append(cur)
                    state, cur = "idle", None
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
    cols = ("span", "horner", "tree1", "gap1", "l1_tab", "l1_step", "tree2", "gap2", "l2_tab", "l2_step", "tail", "run", "wait")
    table = []
    for b in timed:
        t1 = b["l1_table"][0] - b["horner"][1]
        t2 = b["l2_table"][0] - b["l1_step"][1]
        table.append({"span": ms(b["end"] - b["horner"][0]), "horner": ms(b["horner"][1] - b["horner"][0]), "tree1": ms(t1),
                      "gap1": ms(tree_gap(b["horner"][1], b["tree1"], b["l1_table"][0])),
                      "l1_tab": ms(b["l1_step"][0] - b["l1_table"][0]), "l1_step": ms(b["l1_step"][1] - b["l1_step"][0]),
                      "tree2": ms(t2), "gap2": ms(tree_gap(b["l1_step"][1], b["tree2"], b["l2_table"][0])),
                      "l2_tab": ms(b["l2_step"][0] - b["l2_table"][0]), "l2_step": ms(b["l2_step"][1] - b["l2_step"][0]),
                      "tail": ms(b["end"] - b["l2_step"][1])})
        run = sum(e - s_ for s_, e in (b["horner"], b["l1_table"], b["l1_step"], b["l2_table"], b["l2_step"]))
        run += sum(k["e"] - k["s"] for k in b["tree1"] + b["tree2"] + b["tail"])
        table[-1]["run"] = ms(run)
        table[-1]["wait"] = table[-1]["span"] - ms(run)
    print("\nper box, ms (span: first X-path kernel to the end of a1; tree1/tree2: end of the phase before to the start of the table launch,")
    print("gap1/gap2: the longest pause between two kernels inside it = the host round trip; l*_tab: table launch up to the start of the stepping;")
    print("run: sum of the durations of the box's X-path kernels; wait = span - run: time in which none of them was on the chip)")
    print(" box " + " ".join(f"{c:>8}" for c in cols))
    for i, row in enumerate(table):
        print(f"{i:4d} " + " ".join(f"{row[c]:8.2f}" for c in cols))
    print("\n med " + " ".join(f"{st.median(r[c] for r in table):8.2f}" for c in cols))
    print(" min " + " ".join(f"{min(r[c] for r in table):8.2f}" for c in cols))
    print(" max " + " ".join(f"{max(r[c] for r in table):8.2f}" for c in cols))
    if a.l1_steps:
        print(f"level-1 stepping: {a.l1_steps} serial steps, median {st.median(r['l1_step'] for r in table) * 1e3 / a.l1_steps:.2f} us per step")
    if a.l2_steps:
        print(f"level-2 stepping: {a.l2_steps} serial steps, median {st.median(r['l2_step'] for r in table) * 1e3 / a.l2_steps:.2f} us per step")
    steps = [(r["s"], r["e"]) for r in rows if "fd_step" in r["name"]]
    med, mean, mx = concurrency(steps, lo, hi)
    print(f"\nk_modp_fd_step launches on the chip at once (time-weighted, while any runs): median {med}, mean {mean:.2f}, maximum {mx}")
    xmed, xmean, xmx = concurrency([(b["horner"][0], b["end"]) for b in boxes], lo, hi)
    print(f"X paths (first kernel .. a1) open at once: median {xmed}, mean {xmean:.2f}, maximum {xmx}")
    span = st.median(r["span"] for r in table)
    print(f"rate of the timed window from the trace: {ms(hi - lo) / len(timed):.2f} ms per box")
    if a.line:
        line = json.loads([l for l in open(a.line) if l.startswith("{")][-1])
        per = line["ms_per_step"]
        ratio = span / max(xmean, 1e-9) / per
        print(f"value {line['value']:.0f}   ms_per_step {per:.2f}")
        print(f"span / overlapping X paths = {span:.1f} / {xmean:.2f} = {span / xmean:.2f} ms against ms_per_step {per:.2f}: ratio {ratio:.2f}")
        print("verdict: " + ("within 20 %: the chain binds -- a box cannot come sooner than its X path's span over the X paths that advance at once"
                             if 0.8 <= ratio <= 1.2 else "not within 20 %: the chain does not bind by this measure (the chip is issue-bound)"))


if __name__ == "__main__":
    main()
