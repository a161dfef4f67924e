"""The reference of the frameshift search's statistics (a helper, not a test module; include/swbank.h
"statistics of frameshift hits"): nothing new is restated, the definition is a chain of references
the suite already has --

    stat_cases.shuffle -> fshift_cases.c_search_set -> stat_cases.histogram -> stat_cases.fit

-- and the inputs the CPU and GPU tests share, each computed once per process: BLOSUM62 at -11 / -1,
200 DNA targets of 0 .. 400 bases with N codes inside (frame_cases.search_case), a single query of
17 residues and a set of 5, 40, 130 and 300 (the score kernel's 4 and 8 rows per lane)."""
import functools

import numpy as np

from oracle import oracle as O

import frame_cases as F
import fshift_cases as FS
import stat_cases as SC

FS_VALUES = (-15, -32767)
SEEDS = (1, 2)
ROUNDS = 2
SET_LENS = (5, 40, 130, 300)


@functools.lru_cache(maxsize=None)
def batch():
    """(residues, offsets, lengths) of the 200 targets, packed back to back."""
    _, seqs, _ = F.search_case()
    res, offs, lens = O.pack_residues(seqs)
    assert len(lens) == 200 and lens.min() == 0 and lens.max() <= 400 and (res == 4).any()
    return res, offs, lens


@functools.lru_cache(maxsize=None)
def queries(which):
    """which: "one" (17 residues) or "set" (SET_LENS)."""
    rng = np.random.default_rng(163)
    one = rng.integers(0, 20, 17).astype(np.uint8)
    qset = [rng.integers(0, 20, m).astype(np.uint8) for m in SET_LENS]
    return [one] if which == "one" else qset


def targets_of(res, offs, lens):
    return [res[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


def shuffled_scores(qs, res, offs, lens, seed, fs, first=0):
    """scores[nq, n] of the queries against the reference shuffle (batch positions first, ...)."""
    shuf = SC.shuffle(res, offs, lens, seed, first=first)
    return FS.c_search_set(qs, targets_of(shuf, offs, lens), O.BLOSUM62, *F.PEN, fs)[0]


@functools.lru_cache(maxsize=None)
def round_scores(which, seed, fs):
    """One round of the shared batch: scores[nq, n] under the shuffle seed `seed`."""
    return shuffled_scores(queries(which), *batch(), seed, fs)


def pool(score_rounds, lens, nq):
    """(counts[nq, BINS], sums[nq, BINS], clamped[nq]) of several rounds of scores[nq, n]."""
    counts = np.zeros((nq, SC.BINS), np.uint64)
    sums = np.zeros((nq, SC.BINS), np.uint64)
    clamped = np.zeros(nq, np.uint64)
    for sc in score_rounds:
        for i in range(nq):
            c, s, x = SC.histogram(sc[i], lens)
            counts[i] += c
            sums[i] += s
            clamped[i] += np.uint64(x)
    return counts, sums, clamped


@functools.lru_cache(maxsize=None)
def reference(which, seed, fs, rounds=ROUNDS):
    """The pooled histograms of `rounds` rounds (shuffle seeds seed, seed + 1, ...) of the shared
    batch: (counts, sums, clamped)."""
    _, _, lens = batch()
    return pool([round_scores(which, seed + r, fs) for r in range(rounds)], lens,
                len(queries(which)))


def fitted(which, seed, fs, rounds=ROUNDS):
    """Per query (lambda, K, n_samples, min_score, max_score, n_clamped) of the reference."""
    counts, sums, clamped = reference(which, seed, fs, rounds)
    out = []
    for i, q in enumerate(queries(which)):
        lam, K, degenerate = SC.fit(counts[i], sums[i], len(q))
        occ = np.nonzero(counts[i])[0]
        assert not degenerate
        out.append((lam, K, int(counts[i].sum()), int(occ[0]), int(occ[-1]), int(clamped[i])))
    return out
