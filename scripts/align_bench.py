#!/usr/bin/env python3
"""Time the alignment passes (sw_align_hits_device) on the 1,024 best hits of two batches:

* dna      query100.fa x seeded uniform-ACGT 128-bp targets (the headline batch's shape),
           5/-4/-12/-4, merged gaps
* protein  a 512-aa query x seeded 1-kaa targets, BLOSUM62, -11/-1, Gotoh

For each: the batch is scored, the 1,024 best targets (score descending, ties in batch order)
are the hit list, and three things are timed with the bank's HIP events (sw_bank_set_timing:
events around the launches on the stream they run on), `--warmup` calls first, then `--reps`
calls, the median reported:

* ab_ms     passes A+B (end and start cells): a coordinates-only call
* cd_ms     passes C+D (direction store and walk): a call with CIGARs minus the coordinates-only
            call made right before it (the two alternate, so both see the same machine state)
* i32_ms    the yardstick: the int32 score kernel on the same 1,024 pairs as a batch of their
            own (SWBANK_I32=1 sends every pair through it; score_ms of that call, which
            includes the 16-bit pass in front of it)

and ratio_ab = ab_ms / i32_ms.  Two walks of the same recurrence with a few more operations per
cell should land near 2-3.  One JSON line per workload on stdout, the list in --out if given.

* readmap  the query-set chains at the read-mapping shape: 16 seeded 1-kbp references as the set,
           131,072 seeded 150-bp reads as the batch (5/-4/-12/-4, merged).  Timed the same way:
           best_ms (sw_best_queries_device over the 16 x 131,072 scores, with the bytes per
           second it reads against the HBM figure of bench.py's roofline), ab_ms / cd_ms of
           sw_align_set_hits_device on the first `--readmap-hits` reads against their best
           references, and i32_ms on the same pairs, each reference's reads as a batch of their
           own.

Needs a gfx950 GPU; there is no CPU path.
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


def workloads(args):
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    yield ("dna", f"query100.fa x {args.dna_targets} seeded 128-bp targets, 5/-4/-12/-4, merged",
           dict(), lambda b: b.set_penalties(5, -4, -12, -4), q,
           O.random_codes(1000, args.dna_targets * 128, 4).reshape(args.dna_targets, 128))
    pq = O.random_codes(99, 512, 20)
    yield ("protein", f"512-aa query x {args.protein_targets} seeded 1-kaa targets, BLOSUM62 "
           "-11/-1, Gotoh",
           dict(alphabet=S.ALPHABET_PROTEIN, gap_model=S.GAP_GOTOH),
           lambda b: b.set_matrix(O.BLOSUM62, -11, -1), pq,
           O.random_codes(3000, args.protein_targets * 1000, 20).reshape(args.protein_targets,
                                                                          1000))


def median_ms(bank, call, warmup, reps):
    for _ in range(warmup):
        call()
    bank.sync()
    bank.timing()
    out = []
    for _ in range(reps):
        call()
        bank.sync()
        out.append(bank.timing()[2])
    return out


def run(name, desc, kw, pen, q, batch, args, torch):
    dev = torch.device("cuda", args.device)
    n, L = batch.shape
    res = np.ascontiguousarray(batch).reshape(-1)
    offs = np.arange(n, dtype=np.uint64) * L
    lens = np.full(n, L, np.uint32)
    k = min(args.hits, n)
    with S.ScoreBank(device=args.device, **kw) as bank:
        pen(bank)
        bank.load_query(q)
        scores = bank.score_batch(res, offs, lens)
        hits = np.lexsort((np.arange(n), -scores.astype(np.int64)))[:k].astype(np.uint64)
        d_res = torch.from_numpy(res).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_hits = torch.from_numpy(hits.view(np.int64)).to(dev)
        stride = 2 * L + 1
        d_out = torch.zeros(k * S.ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cig = torch.zeros(k * stride, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        bank.set_timing(True)

        def coords():
            bank.align_hits_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                   d_hits.data_ptr(), k, d_out.data_ptr())

        def full():
            bank.align_hits_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                   d_hits.data_ptr(), k, d_out.data_ptr(), d_cig.data_ptr(),
                                   stride)

        for _ in range(args.warmup):
            coords()
            full()
        bank.sync()
        bank.timing()
        ab, cd = [], []
        for _ in range(args.reps):
            coords()
            bank.sync()
            a = bank.timing()[2]
            full()
            bank.sync()
            ab.append(a)
            cd.append(bank.timing()[2] - a)
        kernel = bank.last_kernel()
        rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
        assert (rec["score"] == scores[hits.astype(np.int64)]).all(), "alignment vs batch scores"
        assert (rec["flags"][rec["score"] > 0] == 0).all(), "a hit without a path"
        cells = int(len(q)) * int(L) * k
        # the yardstick: the same pairs as their own batch through the int32 score kernel
        sub = np.ascontiguousarray(batch[hits.astype(np.int64)]).reshape(-1)
        s_res = torch.from_numpy(sub).to(dev)
        s_offs = torch.from_numpy((np.arange(k, dtype=np.uint64) * L).view(np.int64)).to(dev)
        s_lens = torch.from_numpy(np.full(k, L, np.uint32).view(np.int32)).to(dev)
        s_sc = torch.zeros(k, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        os.environ["SWBANK_I32"] = "1"
        try:
            i32 = median_ms(bank, lambda: bank.score_batch_device(
                s_res.data_ptr(), s_offs.data_ptr(), s_lens.data_ptr(), k, L, s_sc.data_ptr()),
                args.warmup, args.reps)
            i32_kernel = bank.last_kernel()
        finally:
            os.environ.pop("SWBANK_I32", None)
        assert (s_sc.cpu().numpy() == scores[hits.astype(np.int64)]).all()
    m = statistics.median
    out = {"workload": name, "desc": desc, "hits": k, "query_len": int(len(q)), "target_len": int(L),
           "cells_per_walk": cells, "warmup": args.warmup, "reps": args.reps,
           "ab_ms": round(m(ab), 4), "ab_ms_min_max": [round(min(ab), 4), round(max(ab), 4)],
           "cd_ms": round(m(cd), 4), "cd_ms_min_max": [round(min(cd), 4), round(max(cd), 4)],
           "i32_ms": round(m(i32), 4), "i32_ms_min_max": [round(min(i32), 4), round(max(i32), 4)],
           "ratio_ab": round(m(ab) / m(i32), 3), "ab_gcups": round(2 * cells / m(ab) / 1e6, 2),
           "kernel": kernel, "i32_kernel": i32_kernel,
           "mean_columns": round(float(rec["n_columns"].mean()), 1)}
    if args.series:
        out["series"] = args.series
    print(json.dumps(out), flush=True)
    return out


HBM_BYTES_PER_S = 8000.0e9  # bench.py's roofline figure (HBM_PEAK_GBS)


def run_readmap(args, torch):
    dev = torch.device("cuda", args.device)
    nq, n, L, k = 16, args.readmap_reads, 150, min(args.readmap_hits, args.readmap_reads)
    refs = [O.random_codes(7000 + i, 1000, 4) for i in range(nq)]
    batch = O.random_codes(7100, n * L, 4).reshape(n, L)
    res = np.ascontiguousarray(batch).reshape(-1)
    offs = np.arange(n, dtype=np.uint64) * L
    lens = np.full(n, L, np.uint32)
    to_dev = lambda a: torch.from_numpy(a).to(dev)
    with S.ScoreBank(device=args.device) as bank:
        bank.set_penalties(5, -4, -12, -4)
        bank.load_queries(refs)
        d_res, d_offs, d_lens = to_dev(res), to_dev(offs.view(np.int64)), to_dev(lens.view(np.int32))
        d_scores = torch.zeros(nq * n, dtype=torch.int32, device=dev)
        d_bq = torch.zeros(n, dtype=torch.int32, device=dev)
        d_bs = torch.zeros(n, dtype=torch.int32, device=dev)
        stride = 2 * L + 1
        d_out = torch.zeros(k * S.ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cig = torch.zeros(k * stride, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                d_scores.data_ptr())
        score_kernel = bank.last_kernel()
        bank.sync()
        scores = d_scores.cpu().numpy().reshape(nq, n)
        bank.set_timing(True)
        best = median_ms(bank, lambda: bank.best_queries_device(
            d_scores.data_ptr(), n, nq, d_bq.data_ptr(), d_bs.data_ptr()), args.warmup, args.reps)
        best_kernel = bank.last_kernel()
        bq = d_bq.cpu().numpy().view(np.uint32)
        assert (bq == scores.argmax(0)).all() and (d_bs.cpu().numpy() == scores.max(0)).all()

        def coords():
            bank.align_set_hits_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                       k, d_out.data_ptr(), d_hit_queries=d_bq.data_ptr())

        def full():
            bank.align_set_hits_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                       k, d_out.data_ptr(), d_hit_queries=d_bq.data_ptr(),
                                       d_cigar=d_cig.data_ptr(), cigar_stride=stride)

        for _ in range(args.warmup):
            coords()
            full()
        bank.sync()
        bank.timing()
        ab, cd = [], []
        for _ in range(args.reps):
            coords()
            bank.sync()
            a = bank.timing()[2]
            full()
            bank.sync()
            ab.append(a)
            cd.append(bank.timing()[2] - a)
        kernel = bank.last_kernel()
        rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
        assert (rec["score"] == scores.max(0)[:k]).all(), "alignment vs batch scores"
        assert (rec["flags"][rec["score"] > 0] == 0).all(), "a hit without a path"
        # the yardstick: the same pairs through the int32 score kernel, each reference's reads
        # as a batch of their own against that reference alone
        i32 = [0.0] * args.reps
        os.environ["SWBANK_I32"] = "1"
        try:
            for qi in range(nq):
                mine = np.nonzero(bq[:k] == qi)[0]
                if not len(mine):
                    continue
                s_res = to_dev(np.ascontiguousarray(batch[mine]).reshape(-1))
                s_offs = to_dev((np.arange(len(mine), dtype=np.uint64) * L).view(np.int64))
                s_lens = to_dev(np.full(len(mine), L, np.uint32).view(np.int32))
                s_sc = torch.zeros(len(mine), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                bank.load_query(refs[qi])
                part = median_ms(bank, lambda: bank.score_batch_device(
                    s_res.data_ptr(), s_offs.data_ptr(), s_lens.data_ptr(), len(mine), L,
                    s_sc.data_ptr()), args.warmup, args.reps)
                i32 = [x + y for x, y in zip(i32, part)]
                i32_kernel = bank.last_kernel()
                assert (s_sc.cpu().numpy() == scores[qi, mine]).all()
        finally:
            os.environ.pop("SWBANK_I32", None)
    m = statistics.median
    cells = 1000 * L * k
    bytes_read = nq * n * 4
    out = {"workload": "readmap",
           "desc": f"{nq} seeded 1-kbp references (the set) x {n} seeded {L}-bp reads, "
                   "5/-4/-12/-4, merged",
           "reads": n, "queries": nq, "hits": k, "query_len": 1000, "target_len": L,
           "cells_per_walk": cells, "warmup": args.warmup, "reps": args.reps,
           "best_ms": round(m(best), 4),
           "best_ms_min_max": [round(min(best), 4), round(max(best), 4)],
           "best_bytes": bytes_read,
           "best_bytes_per_s": round(bytes_read / (m(best) * 1e-3), 0),
           "best_hbm_fraction": round(bytes_read / (m(best) * 1e-3) / HBM_BYTES_PER_S, 4),
           "ab_ms": round(m(ab), 4), "ab_ms_min_max": [round(min(ab), 4), round(max(ab), 4)],
           "cd_ms": round(m(cd), 4), "cd_ms_min_max": [round(min(cd), 4), round(max(cd), 4)],
           "i32_ms": round(m(i32), 4), "i32_ms_min_max": [round(min(i32), 4), round(max(i32), 4)],
           "ratio_ab": round(m(ab) / m(i32), 3), "ab_gcups": round(2 * cells / m(ab) / 1e6, 2),
           "kernel": kernel, "best_kernel": best_kernel, "score_kernel": score_kernel,
           "i32_kernel": i32_kernel, "mean_columns": round(float(rec["n_columns"].mean()), 1)}
    if args.series:
        out["series"] = args.series
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--hits", type=int, default=1024)
    ap.add_argument("--dna-targets", type=int, default=499 * 256)
    ap.add_argument("--protein-targets", type=int, default=12500)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--readmap-reads", type=int, default=131072)
    ap.add_argument("--readmap-hits", type=int, default=4096)
    ap.add_argument("--only", choices=["dna", "protein", "readmap"])
    ap.add_argument("--series", help="a label stored with every row (e.g. the commit measured)")
    ap.add_argument("--out", help="also write the rows as a JSON list to this file "
                    "(profiles/align_bench.json is such a file)")
    args = ap.parse_args()
    if S.device_count() == 0:
        raise SystemExit("align_bench: no gfx950 device (there is no CPU path)")
    import torch
    rows = [run(*w, args, torch) for w in workloads(args) if args.only in (None, w[0])]
    if args.only in (None, "readmap"):
        rows.append(run_readmap(args, torch))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
