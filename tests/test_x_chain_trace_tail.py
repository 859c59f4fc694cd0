"""tools/x_chain_trace.py on a synthetic kernel trace: two boxes whose tails (X's table and a1) run on another stream and hardware
queue than their chains, and one box of the earlier shape with everything on one stream.  The chain ends with the box's last kernel
on the chain's stream, the tail is found on the other stream and reported with its stream and queue, "open at once" counts chains,
and the earlier shape cuts as it always did.  (The raw trace behind profiles/x_chain_trace_parent.txt is not in the tree, only its
report: the earlier format is pinned by the third box here.)"""
import csv
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = 1_000_000


def load_tool():
    spec = importlib.util.spec_from_file_location("x_chain_trace", os.path.join(ROOT, "tools", "x_chain_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Trace:
    def __init__(self):
        self.rows = []

    def k(self, name, stream, queue, start_ms, dur_ms, grid=4096):
        self.rows.append({"Kernel_Name": name, "Start_Timestamp": int(start_ms * MS), "End_Timestamp": int((start_ms + dur_ms) * MS),
                          "Stream_Id": stream, "Queue_Id": queue, "Grid_Size_X": grid})
        return start_ms + dur_ms

    def chain(self, stream, queue, t0):
        """seeds .. level-2 stepping .. from_mont .. gated Horner on one stream; returns (end of the stepping, end of the chain)"""
        t = self.k("k_modp_commit_eval_row", stream, queue, t0, 30)
        for nm in ("k_modp_binv_up", "k_modp_from_mont", "__amd_rocclr_copyBuffer", "k_modp_to_mont", "k_modp_binv_down"):
            t = self.k(nm, stream, queue, t + 0.01, 0.2, 64)
        t = self.k("k_modp_fd_table", stream, queue, t + 0.01, 5)
        t = self.k("k_modp_fd_step", stream, queue, t + 0.01, 25)
        for nm in ("k_modp_binv_up", "k_modp_from_mont", "k_modp_to_mont", "k_modp_binv_down"):
            t = self.k(nm, stream, queue, t + 0.01, 0.3, 64)
        t = self.k("k_modp_fd_table", stream, queue, t + 0.01, 10)
        step_end = self.k("k_modp_fd_step", stream, queue, t + 0.01, 50)
        t = self.k("k_modp_from_mont", stream, queue, step_end + 0.01, 1, 65536 * 4)
        t = self.k("k_modp_commit_eval", stream, queue, t + 0.01, 0.01, 65536)
        return step_end, t

    def side(self, stream, queue, t0):
        t = self.k("k_modp_build_table", stream, queue, t0, 3)
        t = self.k("k_modp_rows2_dual_exp_pair", stream, queue, t + 0.01, 60)
        return self.k("k_modp_comb_dual_exp", stream, queue, t + 0.01, 8)          # g^r

    def tail(self, stream, queue, t0):
        t = self.k("k_modp_build_table", stream, queue, t0, 4)
        return self.k("k_modp_comb_dual_exp", stream, queue, t + 0.01, 12)         # a1

    def write(self, path):
        with open(path, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(self.rows[0]))
            w.writeheader()
            w.writerows(self.rows)


def synthetic(path):
    tr = Trace()
    # box 0: chain on stream 1 / queue 1, side work and tail on stream 2 / queue 2
    step0, end0 = tr.chain(1, 1, 0)
    tr.side(2, 2, 1)
    tail0 = tr.tail(2, 2, end0 + 5)
    # box 1: chain on stream 3, which shares queue 1 and so starts behind box 0's chain; tail on stream 4 / queue 3
    step1, end1 = tr.chain(3, 1, end0 + 0.5)
    tr.side(4, 3, end0 + 1)
    tail1 = tr.tail(4, 3, end1 + 2)
    # the next occupant of stream 1 closes box 0's chain there (its commitments, then its seeds)
    tr.k("k_modp_to_mont", 1, 1, tail0 + 1, 0.1, 64)
    # box 2, the earlier shape: everything on stream 5 / queue 4
    step2, end2 = tr.chain(5, 4, 10)
    tail2 = tr.tail(5, 4, end2 + 0.01)
    tr.write(path)
    return dict(step=[step0, step1, step2], chain_end=[end0, end1, tail2], tail_end=[tail0, tail1, tail2], start=[0, end0 + 0.5, 10])


def test_chains_and_detached_tails(tmp_path, capsys, monkeypatch):
    tool = load_tool()
    path = str(tmp_path / "kernel_trace.csv")
    want = synthetic(path)
    boxes = sorted(tool.cut_boxes(tool.load(path)), key=lambda b: b["horner"][0])
    assert len(boxes) == 3
    by_start = sorted(range(3), key=lambda i: want["start"][i])
    for b, i in zip(boxes, by_start):
        assert b["horner"][0] == int(want["start"][i] * MS)
        assert b["l2_step"][1] == int(want["step"][i] * MS)
        assert b["chain_end"] == int(want["chain_end"][i] * MS), i
        assert b["end"] == int(want["tail_end"][i] * MS), i
        assert "comb_dual_exp" in b["a1_kernel"]
    b0, b2, b1 = boxes                                       # by start: box 0 (0 ms), box 2 (10 ms), box 1
    assert (b0["stream"], b0["tail_stream"], b0["tail_queue"]) == ("1", "2", "2")
    assert (b1["stream"], b1["tail_stream"], b1["tail_queue"]) == ("3", "4", "3")
    assert (b2["stream"], b2["tail_stream"], b2["tail_queue"]) == ("5", "5", "4")
    # the tail of a detached box is not part of its chain, g^r is nobody's a1, and every tail is table + a1
    for b in (b0, b1):
        assert b["chain_end"] < b["end"] and [k["name"] for k in b["tail"][-2:]] == ["k_modp_build_table", "k_modp_comb_dual_exp"]
        assert b["tail"][-2]["s"] >= b["chain_end"]
    # the report: old columns kept, the new ones beside them
    line = tmp_path / "line.json"
    line.write_text(json.dumps({"value": 1.0e6, "ms_per_step": 60.0}) + "\n")
    monkeypatch.setattr(sys, "argv", ["x_chain_trace.py", path, "--line", str(line), "--last", "3", "--queues", "4"])
    tool.main()
    out = capsys.readouterr().out
    assert "tails on another stream than their chain: 2 of 3" in out
    assert "tail streams: 2" in out and "hardware queues the tails ran on: 2" in out
    head = [l for l in out.splitlines() if l.startswith(" box ")][0].split()
    assert head[:3] == ["box", "chain", "span"] and head[3:] == ["horner", "tree1", "gap1", "l1_tab", "l1_step", "tree2", "gap2", "l2_tab",
                                                                 "l2_step", "tail", "run", "wait"]
    rows = [l for l in out.splitlines() if l[:4].strip().isdigit()]
    assert len(rows) == 3 and sum("(chain's)" in r for r in rows) == 1 and any(r.rstrip().endswith("2/2") for r in rows)
    # two chains share queue 1 one after the other and the third overlaps both: never three chains at once there, but the old span would
    assert "chains (first kernel .. last kernel on the chain's stream) open at once: median 2" in out
    assert "end of the stepping to the next box's seed kernel on the same queue" in out
    assert "chain / chains open at once" in out and "ratio" in out
