"""CPU references of the hit statistics (include/swbank.h "hit significance"): the seeded
shuffle, the score / length histogram and the maximum-likelihood fit, in numpy; and the inputs
the CPU and GPU tests share, each computed once.

The shuffle is vectorised over the targets of a batch, one step per j; the fit is a bisection
of the likelihood equation over the occupied bins."""
import functools
import os

import numpy as np

from oracle import oracle as O

BINS = 4096
G = np.uint64(0x9E3779B97F4A7C15)
REF = (5, -4, -12, -4)   # the reference's penalties
GOLDEN_STATS = os.path.join(O.GOLDEN, "statistics500.tsv")


def mix(z):
    """The finaliser of oracle.splitmix64_bytes on a uint64 array."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def shuffle(res, offs, lens, seed, sattolo=False, first=0):
    """The shuffled copy of every target of the batch (positions first, first + 1, ...) inside a
    copy of `res`: bytes outside the targets are kept.  sattolo: r drawn from [0, j) instead of
    [0, j] (the variant the tests must tell apart)."""
    res = np.ascontiguousarray(res, np.uint8)
    offs = np.asarray(offs, np.uint64).astype(np.int64)
    lens = np.asarray(lens, np.uint32).astype(np.int64)
    out = res.copy()
    n = len(lens)
    if n == 0:
        return out
    with np.errstate(over="ignore"):
        key = mix(np.uint64(seed % (1 << 64)) +
                  G * (np.arange(n, dtype=np.uint64) + np.uint64(first + 1)))
    order = np.argsort(-lens, kind="stable")  # longest first: the active ones are a prefix
    so, sk, sl = offs[order], key[order], lens[order]
    for j in range(int(sl[0]) - 1, 0, -1):
        a = int(np.searchsorted(-sl, -j, side="left"))  # targets with len > j
        with np.errstate(over="ignore"):
            h = mix(sk[:a] + G * np.uint64(j + 1))
        r = (((h >> np.uint64(32)) * np.uint64(j if sattolo else j + 1)) >> np.uint64(32))
        pj, pr = so[:a] + j, so[:a] + r.astype(np.int64)
        vj, vr = out[pj], out[pr]
        out[pj], out[pr] = vr, vj
    return out


def histogram(scores, lens=None):
    """(counts, len_sums, clamped) of one row of scores, as sw_score_histogram_device adds them."""
    s = np.asarray(scores, np.int64)
    keep = np.ones(len(s), bool) if lens is None else np.asarray(lens) > 0
    b = np.clip(s[keep], 0, BINS - 1)
    counts = np.bincount(b, minlength=BINS).astype(np.uint64)
    if lens is None:
        sums = np.zeros(BINS, np.uint64)
    else:
        ln = np.asarray(lens, np.uint64)[keep]
        sums = np.zeros(BINS, np.uint64)
        np.add.at(sums, b, ln)
    return counts, sums, int((b != s[keep]).sum())


def fit(counts, len_sums, query_len, weights=True):
    """(lambda, K, degenerate) of one histogram row.  weights=False drops the length weights
    (every target weighs 1: the variant the tests must tell apart)."""
    c = np.asarray(counts, np.float64)
    occ = np.nonzero(np.asarray(counts))[0]
    if len(occ) < 2 or query_len == 0:
        return 0.0, 0.0, True
    s = occ.astype(np.float64)
    cs = c[occ]
    A = query_len * (np.asarray(len_sums, np.float64)[occ] if weights else cs)
    N = cs.sum()
    mean = (s * cs).sum() / N
    s0 = s[0]

    def f(lam):
        w = A * np.exp(-lam * (s - s0))
        return 1.0 / lam - mean + (s * w).sum() / w.sum()

    hi = 1.0
    while f(hi) > 0:
        hi *= 2.0
    lo = hi / 2.0
    while f(lo) < 0:
        lo /= 2.0
    for _ in range(200):
        if hi - lo <= 1e-14 * lo:
            break
        mid = 0.5 * (lo + hi)
        if f(mid) > 0:
            lo = mid
        else:
            hi = mid
    lam = 0.5 * (lo + hi)
    K = N * np.exp(lam * s0) / (A * np.exp(-lam * (s - s0))).sum()
    return float(lam), float(K), False


# ---- shared inputs ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    """query100 x data500 of the reference: (query codes, packed residues, offsets, lengths)."""
    recs = O.read_fasta(O.golden_fasta("data500.fa"))
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    res, offs, lens = O.pack_residues([O.encode_dna(s) for _, s in recs])
    return q, res, offs, lens


@functools.lru_cache(maxsize=None)
def golden_hist(seed, rounds=1):
    """The pooled histogram of the oracle's scores of `rounds` reference shuffles (seeds seed,
    seed + 1, ...) of data500 against query100: (counts, len_sums)."""
    q, res, offs, lens = golden()
    counts, sums = np.zeros(BINS, np.uint64), np.zeros(BINS, np.uint64)
    for r in range(rounds):
        sc = O.score_batch(q, shuffle(res, offs, lens, seed + r), offs, lens, O.dna_matrix(),
                           REF[2], REF[3], O.GAP_MERGED)
        c, s, _ = histogram(sc, lens)
        counts += c
        sums += s
    return counts, sums


@functools.lru_cache(maxsize=None)
def ragged():
    """A ragged DNA batch of 400 targets of 64 .. 150 codes and a query of 90:
    (query, residues, offsets, lengths)."""
    rng = np.random.default_rng(31)
    lens = rng.integers(64, 151, 400)
    seqs = [O.random_codes(700 + i, int(l), 4) for i, l in enumerate(lens)]
    res, offs, ln = O.pack_residues(seqs)
    return O.random_codes(699, 90, 4), res, offs, ln


@functools.lru_cache(maxsize=None)
def ragged_hist(seed=5, rounds=4):
    q, res, offs, lens = ragged()
    counts, sums = np.zeros(BINS, np.uint64), np.zeros(BINS, np.uint64)
    for r in range(rounds):
        sc = O.score_batch(q, shuffle(res, offs, lens, seed + r), offs, lens, O.dna_matrix(),
                           REF[2], REF[3], O.GAP_MERGED)
        c, s, _ = histogram(sc, lens)
        counts += c
        sums += s
    return counts, sums


def golden_stats():
    """tests/golden/statistics500.tsv: (Lambda, K, db_size, query_len, [(name, target_len,
    score, bits text, E text)])."""
    rows = [ln.rstrip("\n").split("\t") for ln in open(GOLDEN_STATS) if not ln.startswith("#")]
    head = dict(zip(rows[0], rows[1]))
    hits = [(r[0], int(r[1]), int(r[2]), r[3], r[4]) for r in rows[3:]]
    return (float(head["lambda"]), float(head["K"]), int(head["db_size"]),
            int(head["query_len"]), hits)
