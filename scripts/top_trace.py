#!/usr/bin/env python3
"""Per-kernel times of the top-hits selection (profiles/top_kernels.json), from a kernel trace:

    rocprofv3 --kernel-trace -d DIR -o top -- python scripts/top_trace.py run
    python scripts/top_trace.py summary DIR/top_results.db --out profiles/top_kernels.json

`run` makes `--calls` sw_top_hits_device calls each at k = 64 and k = 4096 over one row of
1,021,952 seeded scores, uniform in [30, 80) (a DNA batch's band).  `summary` reads the trace's
database: every call is 9 stream operations in order (the memset of the state, 6 x top_hist,
top_select, top_order), and the median, minimum and maximum of each kind are reported per k.
Needs a gfx950 GPU for `run`; `summary` needs only the database.
"""
import argparse
import json
import os
import sqlite3
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "smith-waterman-fpga-module_amd"))

N = 1_021_952
KS = (64, 4096)
OPS = (("memset", (0,)), ("top_hist", (1, 2, 3, 4, 5, 6)), ("top_select", (7,)),
       ("top_order", (8,)))


def run(args):
    import numpy as np
    import torch

    import swbank as S
    scores = np.random.default_rng(1).integers(30, 80, N).astype(np.int32)
    d = torch.from_numpy(scores).cuda()
    hits = torch.zeros(max(KS), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with S.ScoreBank() as bank:
        for k in KS:
            for _ in range(args.calls):
                bank.top_hits_device(d.data_ptr(), N, k, hits.data_ptr())
            bank.sync()


def summary(args):
    db = sqlite3.connect(args.db)
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    ops = [(name, (end - start) / 1000.0) for name, start, end in rows
           if "swk::top_" in name or "fillBuffer" in name]
    calls, rest = divmod(len(ops), 9 * len(KS))
    shaped = all("fillBuffer" in ops[c * 9][0] and "top_order" in ops[c * 9 + 8][0]
                 for c in range(calls * len(KS)))
    if rest or not calls or not shaped:
        raise SystemExit(f"{args.db}: not {len(KS)} x calls x 9 operations of the selection")
    out = []
    for i, k in enumerate(KS):
        for name, idx in OPS:
            x = [ops[(i * calls + c) * 9 + j][1] for c in range(calls) for j in idx]
            out.append({"n": N, "k": k, "operation": name, "per_call": len(idx), "calls": calls,
                        "median_us": round(statistics.median(x), 1), "min_us": round(min(x), 1),
                        "max_us": round(max(x), 1)})
    text = "[\n" + ",\n".join(" " + json.dumps(r) for r in out) + "\n]\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--calls", type=int, default=20)
    s = sub.add_parser("summary")
    s.add_argument("db")
    s.add_argument("--out")
    args = ap.parse_args()
    (run if args.mode == "run" else summary)(args)


if __name__ == "__main__":
    main()
