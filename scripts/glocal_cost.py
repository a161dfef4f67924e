#!/usr/bin/env python3
"""What scoring a read end to end costs: the global-local search (sw_score_glocal_device,
SW_ENDS_TARGET, one strand) against the local search (sw_score_batch_device, unchanged) on the same
batch and the same query set, a reduced shape of bench.py's reads150x1k: `--reads` seeded random
150-bp reads as the batch against `--refs` random 1-kbp references as the query set, 5 / -4,
-12 / -4, Gotoh gaps.  Both calls visit refs x 1,000 x 150 cells per read, so the ratio of their
times is the price of int32 lanes without a floor beside the packed 16-bit local kernels.

The two calls alternate call by call in one process, `--warmup` rounds first, then `--reps`
rounds; a call's time is the sum of the bank's own brackets (sw_bank_set_timing: device time of its
launches), the median is reported.  The new kernel's registers, scratch, LDS and occupancy are
read from the compiler's resource remarks for every instance, its VALU instructions per cell from
the device assembly: the VALU instructions of the whole body of the step loop of the instance
that serves the references (the K cells, the DPP moves, the boundary and loop bookkeeping; the
one-time capture of the end column apart) over K cells, and the issue ceiling they imply at
1,024 SIMDs x 2.4 GHz (nominal) / 4 clocks per wave64 instruction x 64 lanes.  One JSON line on
stdout, the same object in --out if given (profiles/glocal_cost.json is such a file).

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

LANE_OPS = 1024 * 2.4e9 / 4 * 64  # wave64 VALU lane-operations per second, nominal clock
ENDS_NAMES = {1: "query", 2: "target", 3: "both"}


def rows_per_lane(m):
    return 4 if m <= 256 else 8 if m <= 512 else 16


def static_figures(m, ends):
    """{instances: {"K<k> <ends>": {vgprs, agprs, scratch_bytes, lds_bytes, occupancy, spills}},
    rows_per_lane, valu_per_step, valu_per_cell, tcups_ceiling} -- the last four of the instance
    that serves queries of m rows under `ends`."""
    K = rows_per_lane(m)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(PKG, "csrc", "swbank_kglocal.hip")
    base = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-munsafe-fp-atomics",
            "-I", os.path.join(REPO, "include"), "-I", os.path.join(PKG, "csrc")]
    r = subprocess.run(base + ["-c", src, "-o", os.devnull,
                               "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    keys = {"VGPRs:": "vgprs", "AGPRs:": "agprs", "ScratchSize [bytes/lane]:": "scratch_bytes",
            "Occupancy [waves/SIMD]:": "occupancy", "LDS Size [bytes/block]:": "lds_bytes",
            "VGPRs Spill:": "vgpr_spills", "SGPRs Spill:": "sgpr_spills"}
    inst, cur = {}, None
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            mm = re.search(r"glocal_scoreILi(\d+)ELi(\d)E", line)
            cur = inst.setdefault(f"K{mm.group(1)} {ENDS_NAMES[int(mm.group(2))]}", {}) if mm else None
        for k, name in keys.items():
            if cur is not None and f" {k}" in line:
                cur[name] = int(line.split(k)[1].split()[0])
    out = {"instances": inst, "rows_per_lane": K}
    tag = f"glocal_scoreILi{K}ELi{ends}E"
    asm = subprocess.run(base + ["-S", "--cuda-device-only", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    body = re.split(rf"^\w*{tag}\w*:", asm, 1, flags=re.M)[1].split("s_endpgm", 1)[0]
    out.update(step_figures(body.splitlines(), K))
    return out


def step_figures(lines, K):
    """The VALU instructions of one walk step, counted over the whole body of the step loop: the
    innermost loop (a label and the closest `s_branch` back to it) that holds the K cells, the
    longest loop-free block.  The block that follows the cells under their own EXEC branch, if
    any, is the capture of the end column (TARGET, BOTH): a lane runs it at one step only, so it
    is reported apart and not counted into the step."""
    def valu(a, b):
        return sum(1 for s in lines[a:b] if re.match(r"\s*v_(?!readlane|readfirstlane)\w+", s))

    labels = {re.match(r"(\.LBB\w+):", s).group(1): i for i, s in enumerate(lines)
              if re.match(r"\.LBB\w+:", s)}
    loops = []  # (head, back) of every backward branch
    for i, s in enumerate(lines):
        mm = re.match(r"\s*s_c?branch\w*\s+(\.LBB\w+)", s)
        if mm and labels.get(mm.group(1), i) < i:
            loops.append((labels[mm.group(1)], i))
    inner = [(h, b) for h, b in loops
             if not any((h2, b2) != (h, b) and h <= h2 and b2 <= b for h2, b2 in loops)]
    head, back = max(inner, key=lambda hb: valu(*hb))  # the step loop: the one with the cells
    cuts = [i for i in range(head, back + 1)
            if re.match(r"\.LBB\w+:|\s*s_cbranch\w*|\s*s_branch", lines[i])]
    cells = max(zip(cuts, cuts[1:]), key=lambda ab: valu(*ab))
    capture = 0
    mm = re.match(r"\s*s_cbranch_execz\s+(\.LBB\w+)", lines[cells[1]])
    if mm and cells[1] < labels[mm.group(1)] <= back:
        capture = valu(cells[1], labels[mm.group(1)])
    step = valu(head, back) - capture
    return {"valu_cells_block": valu(*cells), "valu_end_column_capture": capture,
            "valu_per_step": step, "valu_per_cell": round(step / K, 2),
            "tcups_ceiling": round(LANE_OPS / (step / K) / 1e12, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reads", type=int, default=16384)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--refs", type=int, default=16)
    ap.add_argument("--ref-len", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--static-from", help="take the compiler's figures from this earlier result "
                    "instead of compiling (the kernel source unchanged since)")
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    n, L, nq, m = args.reads, args.read_len, args.refs, args.ref_len
    out = {"shape": f"reads{L} x {n} x {nq} refs of {m} bp", "penalties": "5/-4 -12/-4 Gotoh",
           "ends": "target", "both_strands": False, "warmup": args.warmup, "reps": args.reps,
           "kernel": (json.load(open(args.static_from))["kernel"] if args.static_from
                      else static_figures(m, S.ENDS_TARGET))}
    assert out["kernel"]["rows_per_lane"] == rows_per_lane(m)
    if not args.static_only:
        if S.device_count() == 0:
            raise SystemExit("glocal_cost: no gfx950 device (--static-only needs none)")
        import torch
        dev = torch.device("cuda", args.device)
        res = np.concatenate([O.random_codes(2000, n * L, 4), np.zeros(64, np.uint8)])
        refs = list(O.random_codes(77, nq * m, 4).reshape(nq, m))
        for k in range(0, n, 4):  # every fourth read is a read: a noisy window of a reference
            a = (k * 37) % (m - L)
            w = refs[(k // 4) % nq][a:a + L].copy()
            w[10 + (k // 4) % (L - 20)] ^= 1  # (away from the ends: no local trim pays)
            res[k * L:(k + 1) * L] = w
        offs = np.arange(n, dtype=np.uint64) * L
        lens = np.full(n, L, np.uint32)
        d_res = torch.from_numpy(res).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_loc = torch.zeros(nq * n, dtype=torch.int32, device=dev)
        d_gl = torch.zeros(nq * n, dtype=torch.int32, device=dev)
        d_ep = torch.zeros(nq * n, dtype=torch.int32, device=dev)
        ptrs = (d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr())
        with S.ScoreBank(device=args.device, gap_model=S.GAP_GOTOH) as bank:
            bank.set_penalties(5, -4, -12, -4)
            bank.load_queries(refs)
            torch.cuda.synchronize()
            calls = {
                "local": lambda: bank.score_batch_device(*ptrs, n, L, d_loc.data_ptr(), min_len=L),
                "glocal": lambda: bank.score_glocal_device(
                    *ptrs, n, L, S.ENDS_TARGET, d_gl.data_ptr(), d_end_pos=d_ep.data_ptr()),
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
        loc = d_loc.cpu().numpy().reshape(nq, n)
        gl = d_gl.cpu().numpy().reshape(nq, n)
        # a read end to end never beats its best piece; a planted read (one substitution) scores
        # 5 x 149 - 4 in both searches against its reference
        assert (gl <= loc).all()
        planted = [(k, (k // 4) % nq) for k in range(0, n, 4)]
        assert all(gl[i][k] == loc[i][k] == 5 * (L - 1) - 4 for k, i in planted[:512])
        med = {k: statistics.median(v) for k, v in ms.items()}
        cells = float(nq) * m * L * n
        out.update({"kernels": names, "launches": launches, "ms_median": med, "ms_all": ms,
                    "ratio_glocal_over_local": round(med["glocal"] / med["local"], 3),
                    "cells": cells,
                    "negative_share": round(float((gl < 0).mean()), 4),
                    "gcups_glocal": round(cells / med["glocal"] / 1e6, 1),
                    "gcups_local": round(cells / med["local"] / 1e6, 1)})
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
