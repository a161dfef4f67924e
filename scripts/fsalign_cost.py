#!/usr/bin/env python3
"""What an alignment of a frameshift hit costs: sw_align_fshift_hits_device against
sw_align_frame_hits_device (the yardstick: the six-frame aligner, one frame per hit) on the same
hits, the 512-aa query of scripts/fshift_cost.py against seeded random 3,000-nt targets that each
hold a 300-aa window of the query with one base inserted in its middle, on either strand,
BLOSUM62 -11/-1, Gotoh gaps, for 64 and for 1,024 hits (hit h is target h).

The frame aligner walks one frame of one strand (m L / 3 cells in pass A); the frameshift aligner
walks the three frames of both strands (2 m L cells), so its pass A alone visits six times the
cells, each at the int32 price of the score kernel.  The two calls alternate call by
call in one process, `--warmup` rounds first, then `--reps` rounds; a call's time is the sum of
the bank's own brackets (sw_bank_set_timing: device time of its launches, the end / start passes
and the path passes one bracket each), the median is reported.  One JSON line on stdout, the same
object in --out if given (profiles/fsalign_align_cost.json is such a file).  Needs a gfx950 GPU.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "smith-waterman-fpga-module_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import swbank as S  # noqa: E402
from oracle import oracle as O  # noqa: E402


def back_translate(rng, aa, table):
    out = []
    for a in aa:
        c = int(rng.choice(np.nonzero(table == a)[0]))
        out += [c >> 4, (c >> 2) & 3, c & 3]
    return np.array(out, np.uint8)


def planted(rng, q, n, L, window, table):
    """n targets of L codes: random DNA around a `window`-aa piece of q, back-translated, with one
    base inserted in its middle; every other target reverse-complemented."""
    res = O.random_codes(3001, n * L, 4).reshape(n, L).copy()
    for k in range(n):
        a = int(rng.integers(0, len(q) - window + 1))
        core = np.insert(back_translate(rng, q[a:a + window], table), 3 * (window // 2) + 1,
                         int(rng.integers(0, 4)))
        at = int(rng.integers(0, L - len(core) + 1))
        res[k, at:at + len(core)] = core
        if k % 2:
            res[k] = (res[k][::-1] ^ 2)  # T, C, A, G = 0..3: the complement flips bit 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--query-len", type=int, default=512)
    ap.add_argument("--hits", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--target-len", type=int, default=3000)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--frameshift", type=int, default=-15)
    ap.add_argument("--stride", type=int, default=64, help="CIGAR ops per hit")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    if S.device_count() == 0:
        raise SystemExit("fsalign_cost: no gfx950 device")
    import torch
    dev = torch.device("cuda", args.device)
    m, L = args.query_len, args.target_len
    rng = np.random.default_rng(512)
    q = rng.integers(0, 20, m).astype(np.uint8)
    table = O.encode_protein(S.STANDARD_CODE)
    out = {"query": m, "target_len": L, "window": args.window, "penalties": "BLOSUM62 -11/-1 Gotoh",
           "frameshift": args.frameshift, "warmup": args.warmup, "reps": args.reps, "runs": []}
    with S.ScoreBank(device=args.device, alphabet=S.ALPHABET_PROTEIN,
                     gap_model=S.GAP_GOTOH) as bank:
        bank.set_matrix(O.BLOSUM62, -11, -1)
        bank.load_query(q)
        for n in args.hits:
            res = planted(rng, q, n, L, args.window, table)
            d_res = torch.from_numpy(np.concatenate([res.reshape(-1), np.zeros(64, np.uint8)])).to(dev)
            d_offs = torch.from_numpy((np.arange(n, dtype=np.uint64) * L).view(np.int64)).to(dev)
            d_lens = torch.from_numpy(np.full(n, L, np.uint32).view(np.int32)).to(dev)
            d_six = torch.zeros(n, dtype=torch.int32, device=dev)
            d_fr = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_sc = torch.zeros(n, dtype=torch.int32, device=dev)
            recs = {k: torch.zeros(n * S.ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                    for k in ("frame", "fshift")}
            cigs = {k: torch.zeros(n * args.stride, dtype=torch.int32, device=dev) for k in recs}
            ptrs = (d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr())
            torch.cuda.synchronize()
            bank.set_timing(False)
            bank.score_frames_device(*ptrs, n, L, d_six.data_ptr(), d_frames=d_fr.data_ptr(),
                                     min_len=L)
            bank.score_frameshift_device(*ptrs, n, L, args.frameshift, d_sc.data_ptr())
            bank.sync()
            calls = {
                "frame": lambda: bank.align_frame_hits_device(
                    *ptrs, n, L, n, recs["frame"].data_ptr(), d_fr.data_ptr(), hits_per_query=n,
                    d_cigar=cigs["frame"].data_ptr(), cigar_stride=args.stride),
                "fshift": lambda: bank.align_frameshift_hits_device(
                    *ptrs, n, L, args.frameshift, n, recs["fshift"].data_ptr(), hits_per_query=n,
                    d_cigar=cigs["fshift"].data_ptr(), cigar_stride=args.stride),
            }
            bank.set_timing(True)
            ms, names = {k: [] for k in calls}, {}
            for it in range(args.warmup + args.reps):
                for k, call in calls.items():
                    bank.timing()
                    call()
                    names[k] = bank.last_kernel()
                    bank.sync()
                    _, _, t = bank.timing()
                    if it >= args.warmup:
                        ms[k].append(t)
            got = {k: recs[k].cpu().numpy().view(S.ALIGNMENT_DTYPE) for k in recs}
            # every hit has its path; the shifted hit scores what the score call said and more
            # than its longer half
            assert (got["fshift"]["flags"] & S.ALIGN_NO_PATH == 0).all()
            assert (got["frame"]["flags"] & S.ALIGN_NO_PATH == 0).all()
            assert np.array_equal(got["fshift"]["score"], d_sc.cpu().numpy())
            assert np.array_equal(got["frame"]["score"], d_six.cpu().numpy())
            assert (got["fshift"]["score"] > got["frame"]["score"]).mean() > 0.9
            med = {k: statistics.median(v) for k, v in ms.items()}
            out["runs"].append({
                "hits": n, "kernels": names, "ms_median": med, "ms_all": ms,
                "ratio_fshift_over_frame": round(med["fshift"] / med["frame"], 2),
                "mean_rows": {k: float((got[k]["q_end"] - got[k]["q_start"] + 1).mean())
                              for k in got}})
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
