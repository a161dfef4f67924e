#!/usr/bin/env python3
"""Time the top-hits selection (sw_top_hits_device) against the score kernel it serves:

* headline   query100.fa x 1,021,952 seeded uniform-ACGT 128-bp targets (bench.py's default
             batch), 5/-4/-12/-4, merged gaps: one row of 1,021,952 scores, k = 64, 1024, 4096
* reads      131,072 seeded 150-bp reads x a query set of 16 seeded 1-kbp slices (bench.py's
             reads150x1k): 16 rows of 131,072 scores, k = 1024

The batch is scored on the device and the scores stay there.  Per case, with `--warmup` calls
first and the median and range of `--reps` calls reported:

* top_ms     sw_top_hits_device, by the bank's HIP events (sw_bank_set_timing brackets the whole
             selection as one launch)
* score_ms   the yardstick it has to be small against: the score kernel's own time for that
             batch, by the same events, in the same run
* topk_ms    the eager-PyTorch way to the same exact answer on the same tensor, by torch events:
             torch.topk(k), then, since topk breaks ties in no stated order, the positions
             reaching the k-th value, a stable descending sort of their scores, and the first k.
             Row by row, with a host synchronisation per row (torch.nonzero): for several rows
             most of this figure is host time, not GPU work
* topk_key_ms  the fairer GPU-side line: one batched torch.topk over [nq, n] 64-bit keys
             (score << 32 | 2^32 - 1 - position, built inside the timed region), which is exact and
             ordered by itself and never returns to the host

and ratio = top_ms / score_ms.  The three answers are compared before anything is timed.  One
JSON line per case on stdout, the list in --out if given.  Needs a gfx950 GPU; there is no CPU
path.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "smith-waterman-fpga-module_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import swbank as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

PEN = (5, -4, -12, -4)


def workloads(args):
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    n = args.targets
    yield ("headline", f"query100.fa x {n} seeded 128-bp targets", [q],
           O.random_codes(1000, n * 128, 4).reshape(n, 128), (64, 1024, 4096))
    n = args.reads
    yield ("reads", f"{n} seeded 150-bp reads x 16 seeded 1-kbp slices (a query set)",
           list(O.random_codes(77, 16 * 1000, 4).reshape(16, 1000)),
           O.random_codes(2000, n * 150, 4).reshape(n, 150), (1024,))


def exact_topk(torch, scores, k):
    """[nq, k] positions: torch.topk, then the stable order of ties an exact answer needs."""
    out = []
    for row in scores:
        kth = torch.topk(row, k).values[-1]
        pos = torch.nonzero(row >= kth).reshape(-1)  # ascending positions
        order = torch.sort(row[pos], descending=True, stable=True).indices[:k]
        out.append(pos[order])
    return torch.stack(out)


def key_topk(torch, scores, k):
    """[nq, k] positions from one batched torch.topk over the 64-bit keys."""
    n = scores.shape[1]
    low = 0xFFFFFFFF - torch.arange(n, dtype=torch.int64, device=scores.device)
    keys = (scores.to(torch.int64) << 32) + low
    return 0xFFFFFFFF - (torch.topk(keys, k, dim=1).values & 0xFFFFFFFF)


def torch_ms(torch, call, warmup, reps):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def spread(xs):
    return round(statistics.median(xs), 4), [round(min(xs), 4), round(max(xs), 4)]


def run(name, desc, queries, batch, ks, args, torch):
    dev = torch.device("cuda", args.device)
    n, L = batch.shape
    nq = len(queries)
    res = np.ascontiguousarray(batch).reshape(-1)
    d_res = torch.from_numpy(res).to(dev)
    d_offs = torch.from_numpy((np.arange(n, dtype=np.uint64) * L).view(np.int64)).to(dev)
    d_lens = torch.from_numpy(np.full(n, L, np.uint32).view(np.int32)).to(dev)
    d_scores = torch.zeros((nq, n), dtype=torch.int32, device=dev)
    rows = []
    with S.ScoreBank(device=args.device) as bank:
        bank.set_penalties(*PEN)
        if nq == 1:
            bank.load_query(queries[0])
        else:
            bank.load_queries(queries)
        torch.cuda.synchronize()
        bank.set_timing(True)

        def timed(call):
            for _ in range(args.warmup):
                call()
            bank.sync()
            bank.timing()
            out = []
            for _ in range(args.reps):
                call()
                bank.sync()
                out.append(bank.timing()[2])
            return out

        score = timed(lambda: bank.score_batch_device(
            d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L, d_scores.data_ptr(),
            min_len=L))
        score_kernel = bank.last_kernel()
        for k in ks:
            d_hits = torch.zeros((nq, k), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            top = lambda: bank.top_hits_device(d_scores.data_ptr(), n, k, d_hits.data_ptr(), nq=nq)
            top()
            bank.sync()
            want = exact_topk(torch, d_scores, k)
            assert torch.equal(d_hits, want), "sw_top_hits_device vs torch.topk + stable ties"
            ties = [int((r == r[h[-1]]).sum()) for r, h in zip(d_scores, d_hits)]
            top_ms = timed(top)
            assert torch.equal(key_topk(torch, d_scores, k), want), "batched key topk"
            tk = torch_ms(torch, lambda: exact_topk(torch, d_scores, k), args.warmup, args.reps)
            tkk = torch_ms(torch, lambda: key_topk(torch, d_scores, k), args.warmup, args.reps)
            row = {"case": name, "desc": desc, "n": n, "nq": nq, "k": k, "warmup": args.warmup,
                   "reps": args.reps, "ties_at_cut_max": max(ties)}
            for key, xs in (("top_ms", top_ms), ("score_ms", score), ("topk_ms", tk),
                            ("topk_key_ms", tkk)):
                row[key], row[key + "_min_max"] = spread(xs)
            row["ratio"] = round(row["top_ms"] / row["score_ms"], 4)
            row["kernel"], row["score_kernel"] = bank.last_kernel(), score_kernel
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--targets", type=int, default=499 * 2048)
    ap.add_argument("--reads", type=int, default=131072)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=["headline", "reads"])
    ap.add_argument("--out", help="also write the rows as a JSON list to this file "
                    "(profiles/top_bench.json is such a file)")
    args = ap.parse_args()
    if S.device_count() == 0:
        raise SystemExit("top_bench: no gfx950 device (there is no CPU path)")
    import torch
    rows = [r for w in workloads(args) if args.only in (None, w[0]) for r in run(*w, args, torch)]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # a JSON list, one case per line
            f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
