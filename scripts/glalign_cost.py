#!/usr/bin/env python3
"""What aligning a read end to end costs: the alignments of global-local hits
(sw_align_glocal_hits_device, SW_ENDS_TARGET, one strand) against the local alignments of the
same pairs (sw_align_set_hits_device, unchanged), on the reads of scripts/glocal_cost.py: seeded
random 150-bp reads as the batch, every fourth a noisy window of one of `--refs` random 1-kbp
references loaded as the query set, 5 / -4, -12 / -4, Gotoh gaps.  Hit h is read h against the
reference (h // 4) % refs (the planted reads' own reference), for `--hits` of 1,024 and 16,384.

The two calls alternate call by call in one process, `--warmup` rounds first, then `--reps`
rounds; a call's time is the sum of the bank's own brackets (sw_bank_set_timing: the device time
of its two launch groups); the median, the minimum and the maximum are reported.  The global-local
call walks the whole 1,000 x 150 matrix of a pair three times at most (score, start, window); the
local call walks it twice and its window is the read's.  Every new kernel instance's registers,
scratch, LDS and occupancy are read from the compiler's resource remarks.  One JSON line on stdout,
the same object in --out if given (profiles/glalign_cost.json is such a file).

Needs a gfx950 GPU for the times; --static-only prints the compiler's figures alone.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "smith-waterman-fpga-module_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import swbank as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

ENDS_NAMES = {1: "query", 2: "target", 3: "both"}


def static_figures():
    """{"<kernel> K<k>[ <ends>]": {vgprs, agprs, scratch_bytes, lds_bytes, occupancy, spills}}."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(PKG, "csrc", "swbank_kglalign.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
                        "-munsafe-fp-atomics", "-I", os.path.join(REPO, "include"), "-I",
                        os.path.join(PKG, "csrc"), "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    keys = {"VGPRs:": "vgprs", "AGPRs:": "agprs", "ScratchSize [bytes/lane]:": "scratch_bytes",
            "Occupancy [waves/SIMD]:": "occupancy", "LDS Size [bytes/block]:": "lds_bytes",
            "VGPRs Spill:": "vgpr_spills", "SGPRs Spill:": "sgpr_spills"}
    inst, cur = {}, None
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            a = re.search(r"glalign_endsILi(\d+)ELi(\d)E", line)
            b = re.search(r"glalign_pathsILi(\d+)E", line)
            cur = None
            if a:
                cur = inst.setdefault(f"ends K{a.group(1)} {ENDS_NAMES[int(a.group(2))]}", {})
            elif b:
                cur = inst.setdefault(f"paths K{b.group(1)}", {})
        for k, name in keys.items():
            if cur is not None and f" {k}" in line:
                cur[name] = int(line.split(k)[1].split()[0])
    return inst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--hits", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--refs", type=int, default=16)
    ap.add_argument("--ref-len", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    L, nq, m = args.read_len, args.refs, args.ref_len
    out = {"shape": f"reads{L} x {nq} refs of {m} bp, hit h = read h x ref (h // 4) % {nq}",
           "penalties": "5/-4 -12/-4 Gotoh", "ends": "target", "both_strands": False,
           "warmup": args.warmup, "reps": args.reps, "instances": static_figures(), "runs": {}}
    if not args.static_only:
        if S.device_count() == 0:
            raise SystemExit("glalign_cost: no gfx950 device (--static-only needs none)")
        import torch
        dev = torch.device("cuda", args.device)
        n = max(args.hits)
        res = np.concatenate([O.random_codes(2000, n * L, 4), np.zeros(64, np.uint8)])
        refs = list(O.random_codes(77, nq * m, 4).reshape(nq, m))
        for k in range(0, n, 4):  # every fourth read is a read: a noisy window of a reference
            a = (k * 37) % (m - L)
            w = refs[(k // 4) % nq][a:a + L].copy()
            w[10 + (k // 4) % (L - 20)] ^= 1
            res[k * L:(k + 1) * L] = w
        offs = np.arange(n, dtype=np.uint64) * L
        lens = np.full(n, L, np.uint32)
        hq = ((np.arange(n) // 4) % nq).astype(np.uint32)
        stride = 2 * L  # ops of a path: every run is at least one column
        d_res = torch.from_numpy(res).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_hq = torch.from_numpy(hq.view(np.int32)).to(dev)
        d_out = {k: torch.zeros(n * S.ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                 for k in ("local", "glocal")}
        d_cig = {k: torch.zeros(n * stride, dtype=torch.int32, device=dev)
                 for k in ("local", "glocal")}
        ptrs = (d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr())
        with S.ScoreBank(device=args.device, gap_model=S.GAP_GOTOH) as bank:
            bank.set_penalties(5, -4, -12, -4)
            bank.load_queries(refs)
            torch.cuda.synchronize()
            for hits in args.hits:
                calls = {
                    "local": lambda: bank.align_set_hits_device(
                        *ptrs, n, L, hits, d_out["local"].data_ptr(),
                        d_hit_queries=d_hq.data_ptr(), d_cigar=d_cig["local"].data_ptr(),
                        cigar_stride=stride),
                    "glocal": lambda: bank.align_glocal_hits_device(
                        *ptrs, n, L, S.ENDS_TARGET, hits, d_out["glocal"].data_ptr(),
                        d_hit_queries=d_hq.data_ptr(), d_cigar=d_cig["glocal"].data_ptr(),
                        cigar_stride=stride),
                }
                bank.set_timing(True)
                ms, names, launches = {k: [] for k in calls}, {}, {}
                for it in range(args.warmup + args.reps):
                    for k, call in calls.items():
                        bank.timing()
                        call()
                        names[k] = bank.last_kernel()
                        bank.sync()
                        cnt, _, t = bank.timing()
                        launches[k] = cnt
                        if it >= args.warmup:
                            ms[k].append(t)
                rec = {k: d_out[k].cpu().numpy().view(S.ALIGNMENT_DTYPE)[:hits] for k in calls}
                # a planted read (one substitution) aligns end to end in both: the same record
                planted = np.arange(0, hits, 4)
                for f in ("score", "q_start", "q_end", "t_start", "t_end", "n_columns"):
                    assert np.array_equal(rec["local"][f][planted], rec["glocal"][f][planted]), f
                assert (rec["glocal"]["score"][planted] == 5 * (L - 1) - 4).all()
                assert (rec["glocal"]["flags"][planted] == 0).all()
                stat = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                        for k, v in ms.items()}
                out["runs"][str(hits)] = {
                    "kernels": names, "launches": launches, "ms": stat, "ms_all": ms,
                    "ratio_glocal_over_local": round(stat["glocal"]["median"] /
                                                     stat["local"]["median"], 3),
                    "no_path": {k: int((rec[k]["flags"] & S.ALIGN_NO_PATH != 0).sum())
                                for k in calls},
                    "negative_share": round(float((rec["glocal"]["score"] < 0).mean()), 4)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
