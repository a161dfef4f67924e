#!/usr/bin/env python3
"""What the statistics of the frameshift-tolerant search cost, and what the shuffle of long targets
gains, on the §3.16 workload: a 512-aa query x 12,500 seeded random 3,000-nt targets, BLOSUM62
-11/-1, Gotoh gaps, frameshift -15.

* passes     device time (the bank's own brackets, sw_bank_set_timing) of one round's three passes
             through the public calls: sw_shuffle_batch_device, sw_score_fshift_device on the
             shuffled batch, sw_score_histogram_device
* estimate   one sw_estimate_fshift_statistics_device call of 1 round: wall time (it returns after
             synchronising and fitting) and the sum of its brackets
* shuffle    sw_shuffle_batch_device of this build against the library given with --parent-lib
             (the parent commit's, built by scripts/build_variant.sh from its tree), the two
             alternating call by call on the same device buffers, on three batches: the workload's,
             the workload's with one 70,000-nt target added, and the 128-bp headline batch of
             scripts/stats_bench.py; the two libraries' outputs are compared byte for byte.
             `headline_ok`: this build's median is not above the parent's by more than the parent's
             own min-to-max spread.

Every figure: `--warmup` rounds first, then the median and [min, max] of `--reps`.  One JSON line on
stdout, the same object in --out if given (profiles/fshift_stats_cost.json is such a file).  Needs
a gfx950 GPU; there is no CPU path.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "smith-waterman-fpga-module_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import swbank as S  # noqa: E402
from oracle import oracle as O  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min_max": [round(min(xs), 4), round(max(xs), 4)]}


class Shuffler:
    """sw_shuffle_batch_device of one library file through its C ABI, timed by its own bank."""

    def __init__(self, path, device):
        P, u64, u32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
        L = self.L = ctypes.CDLL(path)
        L.sw_config_default.argtypes = [P]
        L.sw_bank_create.argtypes = [ctypes.POINTER(P), P]
        L.sw_bank_destroy.argtypes = [P]
        L.sw_bank_destroy.restype = None
        L.sw_bank_set_timing.argtypes = [P, ctypes.c_int32]
        L.sw_bank_sync.argtypes = [P]
        L.sw_bank_timing.argtypes = [P, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_double)]
        L.sw_shuffle_batch_device.argtypes = [P, P, P, P, sz, u32, u64, P, P]
        L.sw_last_error.argtypes = [P]
        L.sw_last_error.restype = ctypes.c_char_p
        cfg = S._Config()
        self.ok(L.sw_config_default(ctypes.byref(cfg)))
        cfg.device = device
        self.h = P()
        self.ok(L.sw_bank_create(ctypes.byref(self.h), ctypes.byref(cfg)))
        self.ok(L.sw_bank_set_timing(self.h, 1))

    def ok(self, st):
        if st != 0:
            raise SystemExit(f"fshift_stats_cost: status {st}")

    def shuffle_ms(self, ptrs, n, max_len, seed, d_out):
        L, n_l, pm, sm = self.L, ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
        self.ok(L.sw_shuffle_batch_device(self.h, *ptrs, n, max_len, seed, d_out, None))
        self.ok(L.sw_bank_sync(self.h))
        self.ok(L.sw_bank_timing(self.h, ctypes.byref(n_l), ctypes.byref(pm), ctypes.byref(sm)))
        return float(sm.value)

    def close(self):
        self.L.sw_bank_destroy(self.h)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--query-len", type=int, default=512)
    ap.add_argument("--targets", type=int, default=12500)
    ap.add_argument("--target-len", type=int, default=3000)
    ap.add_argument("--long-target", type=int, default=70000)
    ap.add_argument("--headline-targets", type=int, default=499 * 2048)
    ap.add_argument("--frameshift", type=int, default=-15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", help="the parent commit's libswbank.so for the shuffle A/B")
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    if S.device_count() == 0:
        raise SystemExit("fshift_stats_cost: no gfx950 device (there is no CPU path)")
    import torch
    dev = torch.device("cuda", args.device)
    m, n, L, fs = args.query_len, args.targets, args.target_len, args.frameshift
    rounds = args.warmup + args.reps

    def on_dev(a):
        a = np.ascontiguousarray(a)
        a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
        return torch.from_numpy(a).to(dev)

    def batch(n_t, length, extra=0):
        lens = np.full(n_t + (1 if extra else 0), length, np.uint32)
        if extra:
            lens[-1] = extra
        offs = np.zeros(len(lens), np.uint64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        total = int(lens.sum())
        res = np.concatenate([O.random_codes(3000, total, 4), np.zeros(64, np.uint8)])
        t = (on_dev(res), on_dev(offs), on_dev(lens))
        return t, tuple(x.data_ptr() for x in t), len(lens), int(lens.max()), total + 64

    out = {"shape": f"protein{m} x {n} x {L} nt", "penalties": "BLOSUM62 -11/-1 Gotoh",
           "frameshift": fs, "warmup": args.warmup, "reps": args.reps}
    keep, ptrs, _, _, nbytes = batch(n, L)
    d_shuf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    d_sc = torch.zeros(n, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(2 * S.STAT_BINS + 1, dtype=torch.int64, device=dev)
    q = np.random.default_rng(512).integers(0, 20, m).astype(np.uint8)
    with S.ScoreBank(device=args.device, alphabet=S.ALPHABET_PROTEIN, gap_model=S.GAP_GOTOH) as bank:
        bank.set_matrix(O.BLOSUM62, -11, -1)
        bank.load_query(q)
        torch.cuda.synchronize()
        bank.set_timing(True)

        def device(call):
            xs = []
            for it in range(rounds):
                bank.timing()
                call()
                bank.sync()
                xs.append(bank.timing()[2])
            return xs[args.warmup:]

        passes = {
            "shuffle_ms": device(lambda: bank.shuffle_batch_device(*ptrs, n, L, 1, d_shuf.data_ptr())),
            "score_ms": device(lambda: bank.score_frameshift_device(
                d_shuf.data_ptr(), ptrs[1], ptrs[2], n, L, fs, d_sc.data_ptr())),
            "histogram_ms": device(lambda: bank.score_histogram_device(
                d_sc.data_ptr(), n, d_cnt.data_ptr(), d_lens=ptrs[2],
                d_len_sums=d_cnt.data_ptr() + 8 * S.STAT_BINS,
                d_clamped=d_cnt.data_ptr() + 16 * S.STAT_BINS)),
        }
        out["passes"] = {k: spread(v) for k, v in passes.items()}
        wall, brackets = [], []
        for it in range(rounds):
            bank.timing()
            t0 = time.perf_counter()
            (st,) = bank.estimate_frameshift_statistics_device(*ptrs, n, L, fs, seed=1, rounds=1)
            wall.append((time.perf_counter() - t0) * 1e3)
            brackets.append(bank.timing()[2])
        out["estimate"] = {"kernel": bank.last_kernel(), "wall_ms": spread(wall[args.warmup:]),
                           "brackets_ms": spread(brackets[args.warmup:]),
                           "lambda": round(st.lambda_, 6), "K": round(st.K, 6),
                           "n_samples": int(st.n_samples), "flags": int(st.flags)}
    del keep, d_shuf

    if args.parent_lib:
        libs = {"new": Shuffler(S.LIB_PATH, args.device), "parent": Shuffler(args.parent_lib, args.device)}
        cases = {"workload": (n, L, 0), "workload_plus_long": (n, L, args.long_target),
                 "headline_128bp": (args.headline_targets, 128, 0)}
        out["shuffle"] = {}
        for name, (n_t, length, extra) in cases.items():
            keep, ptrs, cnt, max_len, nbytes = batch(n_t, length, extra)
            outs = {k: torch.zeros(nbytes, dtype=torch.uint8, device=dev) for k in libs}
            torch.cuda.synchronize()
            ms = {k: [] for k in libs}
            for it in range(rounds):  # the two alternate call by call
                for k, lib in libs.items():
                    ms[k].append(lib.shuffle_ms(ptrs, cnt, max_len, 1, outs[k].data_ptr()))
            same = bool(torch.equal(outs["new"], outs["parent"]))
            row = {k: spread(v[args.warmup:]) for k, v in ms.items()}
            row.update({"n": cnt, "max_len": max_len, "same_bytes": same,
                        "speedup": round(row["parent"]["median"] / row["new"]["median"], 2)})
            out["shuffle"][name] = row
            del keep, outs
        hp = out["shuffle"]["headline_128bp"]
        out["headline_ok"] = bool(hp["new"]["median"] - hp["parent"]["median"] <=
                                  hp["parent"]["min_max"][1] - hp["parent"]["min_max"][0])
        for lib in libs.values():
            lib.close()
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(out, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
