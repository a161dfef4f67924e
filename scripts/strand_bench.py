#!/usr/bin/env python3
"""Time the both-strand search (sw_score_strands_device) on the headline batch: query100.fa x
1,021,952 seeded uniform-ACGT 128-bp targets (bench.py's q100xdata500), 5/-4/-12/-4, merged gaps.

Three calls are timed on one device, alternating call by call so all see the same machine state,
`--warmup` rounds first, then `--reps` rounds, the median reported.  A call's time is the span
between two events on the stream it runs on (enqueue to completion, nothing else on the device):

* forward_ms    sw_score_batch_device_range: the forward search, the yardstick's unit
* resident_ms   sw_score_strands_device with the caller's resident reverse complement (d_rc)
* scratch_ms    the same with d_rc = NULL: the bank complements into its scratch first

Then, with sw_bank_set_timing, the bank's own brackets (device time of the launches alone):

* rc_kernel_ms     the reverse-complement pass (sw_revcomp_batch_device, one bracketed launch)
* merge_kernel_ms  the strand merge: the brackets of a resident call minus two forward calls'

The yardstick is 2 x forward_ms plus those two kernels' own times; ratio_resident and
ratio_scratch are the calls' times over forward_ms, beyond_* what they take past the yardstick.
One JSON line on stdout, the same object in --out if given.

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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--targets", type=int, default=499 * 2048)
    ap.add_argument("--target-len", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", help="also write the result to this file "
                    "(profiles/strand_bench.json is such a file)")
    args = ap.parse_args()
    if S.device_count() == 0:
        raise SystemExit("strand_bench: no gfx950 device (there is no CPU path)")
    import torch
    dev = torch.device("cuda", args.device)
    n, L = args.targets, args.target_len
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    res = np.concatenate([O.random_codes(1000, n * L, 4), np.zeros(64, np.uint8)])
    offs = np.arange(n, dtype=np.uint64) * L
    lens = np.full(n, L, np.uint32)
    d_res = torch.from_numpy(res).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_rc = torch.zeros_like(d_res)
    d_fwd = torch.zeros(n, dtype=torch.int32, device=dev)
    d_sc = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    h = stream.cuda_stream
    with S.ScoreBank(device=args.device) as bank:
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(q)
        torch.cuda.synchronize()
        bank.revcomp_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n,
                                  d_rc.data_ptr(), stream=h)
        names = {}

        def forward():
            bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                    d_fwd.data_ptr(), stream=h, min_len=L)

        def strands(rc):
            bank.score_strands_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                      d_sc.data_ptr(), d_strands=d_st.data_ptr(), d_rc=rc,
                                      min_len=L, stream=h)

        calls = {"forward": forward, "resident": lambda: strands(d_rc.data_ptr()),
                 "scratch": lambda: strands(0)}

        def span(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            bank.sync()
            return a.elapsed_time(b)

        ms = {k: [] for k in calls}
        for it in range(args.warmup + args.reps):
            for k, call in calls.items():
                t = span(call)
                names[k] = bank.last_kernel()
                if it >= args.warmup:
                    ms[k].append(t)
        # the results: both strand calls agree, and merge what two forward searches give
        merged, st = d_sc.cpu().numpy().copy(), d_st.cpu().numpy().copy()
        strands(d_rc.data_ptr())
        bank.sync()
        stream.synchronize()
        assert np.array_equal(merged, d_sc.cpu().numpy()) and np.array_equal(st, d_st.cpu().numpy())
        fwd = d_fwd.cpu().numpy().copy()
        bank.score_batch_device(d_rc.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                d_fwd.data_ptr(), stream=h, min_len=L)
        bank.sync()
        stream.synchronize()
        rev = d_fwd.cpu().numpy()
        assert np.array_equal(merged, np.maximum(fwd, rev)) and np.array_equal(st, rev > fwd)
        # the bank's own brackets
        bank.set_timing(True)

        def bracket(call):
            out = []
            for it in range(args.warmup + args.reps):
                call()
                bank.sync()
                t = bank.timing()[2]
                if it >= args.warmup:
                    out.append(t)
            return out

        bank.timing()
        rc_ms = bracket(lambda: bank.revcomp_batch_device(
            d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, d_rc.data_ptr(), stream=h))
        fwd_b, res_b = [], []
        for it in range(args.warmup + args.reps):
            forward()
            bank.sync()
            f = bank.timing()[2]
            strands(d_rc.data_ptr())
            bank.sync()
            r = bank.timing()[2]
            if it >= args.warmup:
                fwd_b.append(f)
                res_b.append(r)
    m = statistics.median
    f, r, s = m(ms["forward"]), m(ms["resident"]), m(ms["scratch"])
    rc, merge = m(rc_ms), m([b - 2 * a for a, b in zip(fwd_b, res_b)])
    rnd = lambda xs: [round(min(xs), 4), round(max(xs), 4)]
    out = {"workload": f"query100x{n}x{L}",
           "desc": f"query100.fa x {n} seeded {L}-bp targets, 5/-4/-12/-4, merged; three calls "
                   "alternating on one device",
           "targets": n, "target_len": L, "query_len": int(len(q)), "warmup": args.warmup,
           "reps": args.reps,
           "forward_ms": round(f, 4), "forward_ms_min_max": rnd(ms["forward"]),
           "resident_ms": round(r, 4), "resident_ms_min_max": rnd(ms["resident"]),
           "scratch_ms": round(s, 4), "scratch_ms_min_max": rnd(ms["scratch"]),
           "rc_kernel_ms": round(rc, 4), "rc_kernel_ms_min_max": rnd(rc_ms),
           "merge_kernel_ms": round(merge, 4),
           "forward_bracket_ms": round(m(fwd_b), 4), "resident_bracket_ms": round(m(res_b), 4),
           "rc_bytes": 2 * n * L + 12 * n, "merge_bytes": 13 * n,
           "ratio_resident": round(r / f, 4), "ratio_scratch": round(s / f, 4),
           "yardstick_resident_ms": round(2 * f + merge, 4),
           "yardstick_scratch_ms": round(2 * f + merge + rc, 4),
           "beyond_resident_ms": round(r - (2 * f + merge), 4),
           "beyond_scratch_ms": round(s - (2 * f + merge + rc), 4),
           "reverse_hits": int(st.sum()), "kernels": names}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
