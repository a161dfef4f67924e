#!/usr/bin/env python3
"""Time the shuffled-library estimate (sw_estimate_statistics_device, 1 round) against the
scoring pass it contains, on the headline batch: query100.fa x 1,021,952 seeded uniform-ACGT
128-bp targets (bench.py's default batch), 5/-4/-12/-4, merged gaps.

With `--warmup` calls first and the median and range of `--reps` calls reported, in one process:

* estimate_ms   wall time of one sw_estimate_statistics_device call (it returns after
                synchronising: shuffle, score, histogram, the counters' copy and the host fit)
* score_ms      wall time of one sw_score_batch_device_range of the same batch plus sw_bank_sync
* score_dev_ms, shuffle_dev_ms, hist_dev_ms
                the device time of the score kernel, of sw_shuffle_batch_device and of
                sw_score_histogram_device on that batch, by the bank's HIP events
                (sw_bank_set_timing)

and ratio = estimate_ms / score_ms.  One JSON line on stdout, also written to --out if given.
Needs a gfx950 GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "smith-waterman-fpga-module_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import swbank as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

PEN = (5, -4, -12, -4)


def spread(xs):
    return round(statistics.median(xs), 4), [round(min(xs), 4), round(max(xs), 4)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--targets", type=int, default=499 * 2048)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", help="also write the row to this file (profiles/stats_bench.json)")
    args = ap.parse_args()
    if S.device_count() == 0:
        raise SystemExit("stats_bench: no gfx950 device (there is no CPU path)")
    import torch
    dev = torch.device("cuda", args.device)
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    n, L = args.targets, 128
    d_res = torch.from_numpy(O.random_codes(1000, n * L, 4)).to(dev)
    d_offs = torch.from_numpy((np.arange(n, dtype=np.uint64) * L).view(np.int64)).to(dev)
    d_lens = torch.from_numpy(np.full(n, L, np.uint32).view(np.int32)).to(dev)
    d_scores = torch.zeros(n, dtype=torch.int32, device=dev)
    d_shuf = torch.zeros(n * L, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(2 * S.STAT_BINS + 1, dtype=torch.int64, device=dev)
    batch = (d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr())
    with S.ScoreBank(device=args.device) as bank:
        bank.set_penalties(*PEN)
        bank.load_query(q)
        torch.cuda.synchronize()

        def score():
            bank.score_batch_device(*batch, n, L, d_scores.data_ptr(), min_len=L)
            bank.sync()

        def estimate():
            return bank.estimate_statistics_device(*batch, n, L, seed=1, rounds=1, min_len=L)[0]

        def wall(call):
            for _ in range(args.warmup):
                call()
            out = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                out.append((time.perf_counter() - t0) * 1e3)
            return out

        def device(call):
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

        st = estimate()
        stats_kernel = bank.last_kernel()
        row = {"case": "headline", "desc": f"query100.fa x {n} seeded 128-bp targets, 1 round",
               "n": n, "warmup": args.warmup, "reps": args.reps, "lambda": round(st.lambda_, 6),
               "K": round(st.K, 6), "n_samples": int(st.n_samples)}
        times = {"estimate_ms": wall(estimate), "score_ms": wall(score)}
        score_kernel = bank.last_kernel()
        bank.set_timing(True)
        times["score_dev_ms"] = device(lambda: bank.score_batch_device(
            *batch, n, L, d_scores.data_ptr(), min_len=L))
        times["shuffle_dev_ms"] = device(lambda: bank.shuffle_batch_device(
            *batch, n, L, 1, d_shuf.data_ptr()))
        times["hist_dev_ms"] = device(lambda: bank.score_histogram_device(
            d_scores.data_ptr(), n, d_cnt.data_ptr(), d_lens=d_lens.data_ptr(),
            d_len_sums=d_cnt.data_ptr() + 8 * S.STAT_BINS,
            d_clamped=d_cnt.data_ptr() + 16 * S.STAT_BINS))
        for key, xs in times.items():
            row[key], row[key + "_min_max"] = spread(xs)
        row["ratio"] = round(row["estimate_ms"] / row["score_ms"], 4)
        row["kernel"], row["score_kernel"] = stats_kernel, score_kernel
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
