#!/usr/bin/env python3
"""What the next best alignments of a pair cost: sw_align_disjoint_hits_device with rounds = 1 and
rounds = 4 against the local alignments of the same pairs (sw_align_set_hits_device, unchanged),
on two shapes:

  protein  1,024 hits of one seeded 512-aa query, BLOSUM62 at -11 / -1, against 1-kaa targets that
           each hold two diverged copies of a 200-aa window of the query;
  reads    1,024 seeded 150-bp reads as the batch, every fourth a noisy window of one of 16 random
           1-kbp references loaded as the query set (the reads of scripts/glalign_cost.py), 5 / -4
           at -12 / -4; hit h is read h against reference (h // 4) % 16.

The method is that of scripts/glalign_cost.py: the calls alternate call by call in one process,
`--warmup` rounds first, then `--reps` rounds; a call's time is the sum of the bank's own brackets
(sw_bank_set_timing); the median, the minimum and the maximum are reported.  The new call walks the
whole matrix of a pair once per round and keeps a direction byte per cell; the local call walks it
twice (end, start) and then the window.  Every kernel instance's registers, scratch, LDS and
occupancy are read from the compiler's resource remarks.  One JSON line on stdout, the same object
in --out if given (profiles/disjoint_cost.json is such a file).

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


def static_figures():
    """{"K<k> first|later": {vgprs, agprs, scratch_bytes, lds_bytes, occupancy, spills}}."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(PKG, "csrc", "swbank_klalign.hip")
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
            a = re.search(r"lalign_roundILi(\d+)ELb(\d)E", line)
            cur = inst.setdefault(f"K{a.group(1)} {'first' if a.group(2) == '1' else 'later'}",
                                  {}) if a else None
        for k, name in keys.items():
            if cur is not None and f" {k}" in line:
                cur[name] = int(line.split(k)[1].split()[0])
    return inst


def protein_shape(n):
    """(queries, residues, offsets, lens, hit queries, max_len, stride)."""
    m, L, w = 512, 1000, 200
    q = O.random_codes(91, m, 20)
    res = O.random_codes(3000, n * L, 20)
    rng = np.random.default_rng(92)
    for k in range(n):
        a = (k * 29) % (m - w)
        for c, at in enumerate((50 + k % 100, 600 + k % 150)):
            x = q[a:a + w].copy()
            x[rng.integers(0, w, 10 + 20 * c)] = rng.integers(0, 20, 10 + 20 * c)
            res[k * L + at:k * L + at + w] = x
    return [q], res, L, np.zeros(n, np.uint32), 2 * m


def reads_shape(n):
    L, nq, m = 150, 16, 1000
    res = O.random_codes(2000, n * L, 4)
    refs = list(O.random_codes(77, nq * m, 4).reshape(nq, m))
    for k in range(0, n, 4):  # every fourth read is a read: a noisy window of a reference
        a = (k * 37) % (m - L)
        x = refs[(k // 4) % nq][a:a + L].copy()
        x[10 + (k // 4) % (L - 20)] ^= 1
        res[k * L:(k + 1) * L] = x
    return refs, res, L, ((np.arange(n) // 4) % nq).astype(np.uint32), 2 * L


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--hits", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    n = args.hits
    out = {"hits": n, "warmup": args.warmup, "reps": args.reps, "instances": static_figures(),
           "runs": {}}
    if not args.static_only:
        if S.device_count() == 0:
            raise SystemExit("disjoint_cost: no gfx950 device (--static-only needs none)")
        import torch
        dev = torch.device("cuda", args.device)
        for shape, make, protein in (("protein", protein_shape, True), ("reads", reads_shape, False)):
            qs, res, L, hq, stride = make(n)
            res = np.concatenate([res, np.zeros(64, np.uint8)])
            d_res = torch.from_numpy(res).to(dev)
            d_offs = torch.from_numpy((np.arange(n, dtype=np.uint64) * L).view(np.int64)).to(dev)
            d_lens = torch.from_numpy(np.full(n, L, np.uint32).view(np.int32)).to(dev)
            d_hq = torch.from_numpy(hq.view(np.int32)).to(dev)
            names_ = ("local", "disjoint1", "disjoint4")
            rounds = {"local": 1, "disjoint1": 1, "disjoint4": 4}
            d_out = {k: torch.zeros(n * rounds[k] * S.ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8,
                                    device=dev) for k in names_}
            d_cig = {k: torch.zeros(n * rounds[k] * stride, dtype=torch.int32, device=dev)
                     for k in names_}
            ptrs = (d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr())
            alphabet = S.ALPHABET_PROTEIN if protein else S.ALPHABET_DNA
            with S.ScoreBank(device=args.device, alphabet=alphabet, gap_model=S.GAP_GOTOH) as bank:
                if protein:
                    bank.set_matrix(O.BLOSUM62, -11, -1)
                else:
                    bank.set_penalties(5, -4, -12, -4)
                bank.load_queries(qs)
                torch.cuda.synchronize()

                def disjoint(k):
                    return lambda: bank.align_disjoint_hits_device(
                        *ptrs, n, L, rounds[k], n, d_out[k].data_ptr(),
                        d_hit_queries=d_hq.data_ptr(), d_cigar=d_cig[k].data_ptr(),
                        cigar_stride=stride)
                calls = {
                    "local": lambda: bank.align_set_hits_device(
                        *ptrs, n, L, n, d_out["local"].data_ptr(), d_hit_queries=d_hq.data_ptr(),
                        d_cigar=d_cig["local"].data_ptr(), cigar_stride=stride),
                    "disjoint1": disjoint("disjoint1"), "disjoint4": disjoint("disjoint4")}
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
                rec = {k: d_out[k].cpu().numpy().view(S.ALIGNMENT_DTYPE) for k in calls}
                # round 0 scores and ends where the local call does; rounds = 4 begins as rounds = 1
                r4 = rec["disjoint4"].reshape(n, 4)
                for f in ("score", "q_end", "t_end"):
                    assert np.array_equal(rec["local"][f], rec["disjoint1"][f]), f
                    assert np.array_equal(r4[f][:, 0], rec["disjoint1"][f]), f
                assert (np.diff(r4["score"].astype(np.int64), axis=1) <= 0).all()
                stat = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                        for k, v in ms.items()}
                out["runs"][shape] = {
                    "kernels": names, "launches": launches, "ms": stat, "ms_all": ms,
                    "ratio_disjoint1_over_local": round(stat["disjoint1"]["median"] /
                                                        stat["local"]["median"], 3),
                    "ratio_disjoint4_over_local": round(stat["disjoint4"]["median"] /
                                                        stat["local"]["median"], 3),
                    "ratio_disjoint4_over_disjoint1": round(stat["disjoint4"]["median"] /
                                                            stat["disjoint1"]["median"], 3),
                    "alignments_per_hit_of_4": round(float((r4["score"] > 0).sum(axis=1).mean()), 3),
                    "no_path": {k: int((rec[k]["flags"] & S.ALIGN_NO_PATH != 0).sum())
                                for k in calls}}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
