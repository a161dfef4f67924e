#!/usr/bin/env python3
"""The price of the cross-frame links: the frameshift-tolerant translated search
(sw_score_fshift_device) against the six-frame search (sw_score_frames_device) on the same batch,
a 512-aa query x 12,500 seeded random 3,000-nt targets, BLOSUM62 -11/-1, Gotoh gaps.  Both calls
visit about 2 m L cells per target (three frames of L / 3 codons on two strands), so the ratio of
their times is what a cell costs more when it reads the other two frames.

The two calls alternate call by call in one process, `--warmup` rounds first, then `--reps`
rounds; a call's time is the sum of the bank's own brackets (sw_bank_set_timing: device time of its
launches), the median is reported.  The new kernel's registers, scratch, LDS and occupancy are
read from `make resources`, its VALU instructions per cell from the device assembly of
`make asm`: the VALU instructions of the longest loop-free block of the kernel for that query
(the K rows x 3 frames of one step) over 3 K cells.  One JSON line on stdout, the same object in
--out if given (profiles/fshift_cost.json is such a file).

Needs a gfx950 GPU for the times; --static-only prints the compiler's figures alone, and
--static-from takes them from such a result.
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


def rows_per_lane(m):
    return 4 if m <= 256 else 8 if m <= 512 else 16


def static_figures(m):
    """{vgprs, agprs, scratch_bytes, lds_bytes, occupancy, valu_per_cell} of the kernel variant
    that serves a query of m rows."""
    K = rows_per_lane(m)
    tag = f"fshift_scoreILi{K}E"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(PKG, "csrc", "swbank_kfshift.hip")
    base = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-munsafe-fp-atomics",
            "-I", os.path.join(REPO, "include"), "-I", os.path.join(PKG, "csrc")]
    r = subprocess.run(base + ["-c", src, "-o", os.devnull,
                               "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    out, take = {"rows_per_lane": K}, False
    keys = {"VGPRs:": "vgprs", "AGPRs:": "agprs", "ScratchSize [bytes/lane]:": "scratch_bytes",
            "Occupancy [waves/SIMD]:": "occupancy", "LDS Size [bytes/block]:": "lds_bytes"}
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            take = tag in line
        for k, name in keys.items():
            if take and k in line:
                out[name] = int(line.split(k)[1].split()[0])
    asm = subprocess.run(base + ["-S", "--cuda-device-only", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    body = re.split(rf"^\w*{tag}\w*:", asm, 1, flags=re.M)[1].split("s_endpgm", 1)[0]
    best = 0
    for block in re.split(r"^\.LBB\w+:.*$|^\s*s_cbranch\w*.*$|^\s*s_branch.*$", body, flags=re.M):
        best = max(best, len(re.findall(r"^\s*v_(?!readlane|readfirstlane)\w+", block, flags=re.M)))
    out["valu_per_step"] = best
    out["valu_per_cell"] = round(best / (3 * K), 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--query-len", type=int, default=512)
    ap.add_argument("--targets", type=int, default=12500)
    ap.add_argument("--target-len", type=int, default=3000)
    ap.add_argument("--frameshift", type=int, default=-15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--static-from", help="take the compiler's figures from this earlier result "
                    "instead of compiling (the kernel source unchanged since)")
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    m, n, L = args.query_len, args.targets, args.target_len
    out = {"shape": f"protein{m} x {n} x {L} nt", "penalties": "BLOSUM62 -11/-1 Gotoh",
           "frameshift": args.frameshift, "warmup": args.warmup, "reps": args.reps,
           "kernel": (json.load(open(args.static_from))["kernel"] if args.static_from
                      else static_figures(m))}
    assert out["kernel"]["rows_per_lane"] == rows_per_lane(m)
    if not args.static_only:
        if S.device_count() == 0:
            raise SystemExit("fshift_cost: no gfx950 device (--static-only needs none)")
        import torch
        dev = torch.device("cuda", args.device)
        rng = np.random.default_rng(512)
        q = rng.integers(0, 20, m).astype(np.uint8)
        res = np.concatenate([O.random_codes(3000, n * L, 4), np.zeros(64, np.uint8)])
        offs = np.arange(n, dtype=np.uint64) * L
        lens = np.full(n, L, np.uint32)
        d_res = torch.from_numpy(res).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_six = torch.zeros(n, dtype=torch.int32, device=dev)
        d_fr = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_sc = torch.zeros(n, dtype=torch.int32, device=dev)
        d_sd = torch.zeros(n, dtype=torch.uint8, device=dev)
        ptrs = (d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr())
        with S.ScoreBank(device=args.device, alphabet=S.ALPHABET_PROTEIN,
                         gap_model=S.GAP_GOTOH) as bank:
            bank.set_matrix(O.BLOSUM62, -11, -1)
            bank.load_query(q)
            torch.cuda.synchronize()
            calls = {
                "six_frames": lambda: bank.score_frames_device(
                    *ptrs, n, L, d_six.data_ptr(), d_frames=d_fr.data_ptr(), min_len=L),
                "fshift": lambda: bank.score_frameshift_device(
                    *ptrs, n, L, args.frameshift, d_sc.data_ptr(), d_strands=d_sd.data_ptr()),
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
            # at fs = -32767 the new call must give the six-frame scores (the scores stay far
            # below 32,767 on random targets)
            bank.score_frameshift_device(*ptrs, n, L, -32767, d_sc.data_ptr(),
                                         d_strands=d_sd.data_ptr())
            bank.sync()
            assert np.array_equal(d_sc.cpu().numpy(), d_six.cpu().numpy())
            assert np.array_equal(d_sd.cpu().numpy(), (d_fr.cpu().numpy() >= 3).astype(np.uint8))
        med = {k: statistics.median(v) for k, v in ms.items()}
        cells = 2.0 * m * (L - 2) * n
        out.update({"kernels": names, "launches": launches, "ms_median": med, "ms_all": ms,
                    "ratio_fshift_over_six_frames": round(med["fshift"] / med["six_frames"], 3),
                    "cells": cells,
                    "gcups_fshift": round(cells / med["fshift"] / 1e6, 1),
                    "gcups_six_frames": round(cells / med["six_frames"] / 1e6, 1)})
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
