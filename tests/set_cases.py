"""Inputs and references of the query-set tests (a helper, not a test module): the pair lists of
sw_align_set_hits[_device] and the score matrices of sw_best_queries[_device].

The references are never the code under test: align_check.brute_ends_batch (score and
coordinates; it asserts the oracle's score for every pair), align_cases.ref_paths (the ops),
align_check.check_alignment, the oracle's score_batch, and numpy's max / argmax down a column
(argmax returns the first occurrence: the lowest query).  Everything is computed once per
process and shared.  A builder that selects among its inputs asserts how many remain."""
import numpy as np

from oracle import oracle as O

import align_cases as AL
import align_check as AC

GAP_MERGED, GAP_GOTOH = 0, 1
MODELS = [GAP_MERGED, GAP_GOTOH]
REF, ALT = AL.REF, AL.ALT
HIT_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
QUERY_NONE = np.uint32(0xFFFFFFFF)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ALIGN_EMPTY, ALIGN_NO_PATH, ALIGN_NO_HIT = 1, 2, 4
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------
# 1. pair lists
# The lane and strip edges of align_cases.QLENS, and a second query of 300 rows: queries 8 and 10
# have one length, so a target paired with both tells them apart by their letters alone.
SET_QLENS = [1, 4, 63, 64, 65, 255, 256, 257, 300, 513, 300]
TWINS = (8, 10)
PAIRS_PER_QUERY = 6
LONG_QUERY = 4100          # test 4: its windows need 17 strips
WAVES_SHARED = 64          # the wave count at which hits 0 and 64 share a wave (see set_case)


class SetCase:
    """queries, seqs (the batch), hit_queries / hits (the pair list, hit h = query
    hit_queries[h] against target hits[h])."""

    def __init__(self, queries, seqs, hit_queries, hits, alpha=4):
        self.queries, self.seqs = queries, seqs
        self.hit_queries = np.asarray(hit_queries, np.uint32)
        self.hits = np.asarray(hits, np.uint64)
        self.alpha = alpha

    def __len__(self):
        return len(self.hits)

    def head(self, n):
        return SetCase(self.queries, self.seqs, self.hit_queries[:n], self.hits[:n], self.alpha)


def _scramble(rng, pairs, lens):
    """A random order in which consecutive pairs differ in query (and so in query length, but for
    the twins), pair 0 is one of the 513-row query and pair WAVES_SHARED one of the 1-row query."""
    for _ in range(64):
        left = [pairs[int(k)] for k in rng.permutation(len(pairs))]
        fixed = {0: next(p for p in left if p[0] == 9 and lens[p[1]] >= 63),
                 WAVES_SHARED: next(p for p in left if p[0] == 0)}
        for p in fixed.values():
            left.remove(p)
        out = []
        while len(out) < len(pairs):
            k = len(out)
            if k in fixed:
                out.append(fixed[k])
                continue
            ahead = fixed[k + 1][0] if k + 1 in fixed else None
            ok = [p for p in left if (not out or p[0] != out[-1][0]) and p[0] != ahead]
            if not ok:
                break
            out.append(ok[0])
            left.remove(ok[0])
        if len(out) == len(pairs):
            return out
    raise ValueError("set case: no order with differing neighbours")


def set_case():
    """The boundary set: SET_QLENS queries, 24 targets with the lengths of align_cases.TLENS,
    target k's home query is k % 11 and every odd target is planted from its home query.  Every
    query is paired with its home targets and with others up to PAIRS_PER_QUERY; the list is
    scrambled, then: hit 0 is a pair of the 513-row query and hit WAVES_SHARED one of the 1-row
    query (with WAVES_SHARED waves one wave aligns the one, then the other), two pairs are
    repeated, and one odd target is paired with both 300-row queries."""
    def make():
        rng = np.random.default_rng(2024)
        nqs = len(SET_QLENS)
        queries = [rng.integers(0, 4, L).astype(np.uint8) for L in SET_QLENS]
        lens = [int(x) for x in rng.choice(AL.TLENS, 24)]
        lens[:len(AL.TLENS)] = AL.TLENS
        lens[19] = 200  # (the twins' target: odd, its home is query 8)
        home = [k % nqs for k in range(24)]
        seqs = [rng.integers(0, 4, L).astype(np.uint8) if k % 2 == 0
                else AL.planted(rng, queries[home[k]], L) for k, L in enumerate(lens)]
        pairs = []
        for qi in range(nqs):
            mine = [k for k in range(24) if home[k] == qi]
            rest = [int(k) for k in rng.permutation(24) if home[int(k)] != qi]
            for t in (mine + rest)[:PAIRS_PER_QUERY]:
                pairs.append((qi, t))
        assert all(sum(1 for q, _ in pairs if q == qi) >= PAIRS_PER_QUERY for qi in range(nqs))
        pairs = _scramble(rng, pairs, lens)
        twin_t = next(k for k in range(1, 24, 2) if home[k] == TWINS[0] and lens[k] >= 63)
        tail = [pairs[3], pairs[17], (TWINS[0], twin_t), (TWINS[1], twin_t)]  # two repeats
        if tail[0][0] == pairs[-1][0]:
            tail[0], tail[1] = tail[1], tail[0]
        pairs += tail
        assert pairs[0][0] == 9 and pairs[WAVES_SHARED][0] == 0 and len(pairs) == 70
        assert all(pairs[k][0] != pairs[k - 1][0] for k in range(1, len(pairs))), pairs
        assert len({len(queries[pairs[k][0]]) for k in range(len(pairs))}) == len(set(SET_QLENS))
        return SetCase(queries, seqs, [q for q, _ in pairs], [t for _, t in pairs])
    return _cached("set", make)


def long_case():
    """Test 4's set: set_case's queries and a LONG_QUERY-row one; the batch gains a target
    planted over the whole of it (a window of about 4100 x 4100 cells).  The pairs: the first 30 of
    set_case, the long query against two short targets, and against the long target."""
    def make():
        c = set_case()
        rng = np.random.default_rng(4100)
        ql = rng.integers(0, 4, LONG_QUERY).astype(np.uint8)
        t = ql.copy()
        for pos in rng.integers(8, LONG_QUERY - 8, 60):
            t[pos] = (t[pos] + 1) & 3
        t = np.concatenate([t[:1500], rng.integers(0, 4, 3).astype(np.uint8), t[1500:3000],
                            t[3004:]])
        short = AL.planted(rng, ql, 200)
        seqs = c.seqs + [short, t]
        nq = len(c.queries)
        hq = list(c.hit_queries[:30]) + [nq, nq, nq]
        hits = list(c.hits[:30]) + [3, len(c.seqs), len(c.seqs) + 1]
        return SetCase(c.queries + [ql], seqs, hq, hits)
    return _cached("long", make)


def protein_set_case():
    """300, 37 and 257 aa against targets with the lengths of align_cases.protein_case, target k
    planted from query k % 3 and paired with it; every third target is also paired with the next
    query."""
    def make():
        rng = np.random.default_rng(35)
        queries = [rng.integers(0, 20, L).astype(np.uint8) for L in (300, 37, 257)]
        lens = [400, 1, 37, 256, 257, 399, 128, 300] * 2
        seqs = [AL.planted(rng, queries[k % 3], L, 20) for k, L in enumerate(lens)]
        pairs = [(k % 3, k) for k in range(16)] + [((k + 1) % 3, k) for k in range(0, 16, 3)]
        pairs = [pairs[int(k)] for k in rng.permutation(len(pairs))]
        return SetCase(queries, seqs, [q for q, _ in pairs], [t for _, t in pairs], 20)
    return _cached("protein", make)


def pair_refs(case, sub, go, ge, model, key):
    """[(brute record, Ref | None)] per hit of the case (a slot that names no pair: None)."""
    def make():
        per = {}
        for h, (qi, t) in enumerate(zip(case.hit_queries, case.hits)):
            if qi != QUERY_NONE and t != HIT_NONE:
                per.setdefault(int(qi), set()).add(int(t))
        done = {}
        for qi, ts in per.items():
            ts = sorted(ts, key=lambda t: len(case.seqs[t]))
            q = case.queries[qi]
            for at in range(0, len(ts), 12):
                part = ts[at:at + 12]
                targets = [case.seqs[t] for t in part]
                brute = AC.brute_ends_batch(O, q, targets, sub, go, ge, model)
                refs = AL.ref_paths(q, targets, brute, sub, go, ge, model)
                for t, b, r in zip(part, brute, refs):
                    done[(qi, t)] = (b, r)
        return [done.get((int(qi), int(t))) for qi, t in zip(case.hit_queries, case.hits)]
    return _cached(("refs", key, go, ge, model), make)


def check_records(case, alns, refs, want_path=True, no_path=()):
    """Every record against its reference: index, score and coordinates (brute force), the ops,
    columns and identities (the reference traceback).  `no_path`: hits that must hold
    SW_ALIGN_NO_PATH with exact coordinates although want_path."""
    assert len(alns) == len(case) == len(refs)
    for h, (a, ref) in enumerate(zip(alns, refs)):
        (s, qs, qe, ts, te), path = ref
        assert a.index == int(case.hits[h]) and a.id == a.index, (h, a)
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == (s, qs, qe, ts, te), (h, a)
        if s == 0:
            assert a.flags == ALIGN_EMPTY and not a.ops, (h, a)
        elif not want_path or h in no_path:
            assert a.flags == ALIGN_NO_PATH and not a.ops, (h, a)
            assert (a.n_columns, a.n_identities) == (0, 0), (h, a)
        else:
            assert a.flags == 0 and tuple(a.ops) == tuple(path.ops), (h, a, path)
            assert (a.n_columns, a.n_identities) == (path.n_columns, path.n_identities), (h, a)


def sentinel_ok(a):
    """The record of a slot that names no pair."""
    return (a.index == int(HIT_NONE) and a.id == int(HIT_NONE) and a.score == 0 and
            a.flags == ALIGN_EMPTY | ALIGN_NO_HIT and not a.ops and
            (a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns, a.n_identities) == (0,) * 6)


def readmap_case():
    """Read mapping in small: 4 references of 300-1000 bp (the set), 192 reads of 64-150 bp planted
    from them and 64 random reads (the batch), shuffled; the oracle's 4 x 256 score matrix; a
    threshold between the random and the planted reads' best scores."""
    def make():
        rng = np.random.default_rng(66)
        refs = [rng.integers(0, 4, L).astype(np.uint8) for L in (300, 520, 777, 1000)]
        reads, planted = [], []
        for k in range(256):
            L = int(rng.integers(64, 151))
            if k < 192:
                reads.append(AL.planted(rng, refs[k % 4], L))
            else:
                reads.append(rng.integers(0, 4, L).astype(np.uint8))
            planted.append(k < 192)
        order = rng.permutation(256)
        reads = [reads[int(k)] for k in order]
        planted = np.array([planted[int(k)] for k in order])
        res, offs, lens = O.pack_residues(reads)
        scores = np.stack([O.score_batch(r, res, offs, lens, O.dna_matrix(), -12, -4, GAP_MERGED)
                           for r in refs]).astype(np.int32)
        best = scores.max(0)
        min_score = int(best[~planted].max()) + 1
        assert int((best < min_score).sum()) >= 32 and int((best >= min_score).sum()) >= 32
        assert min_score <= int(best[planted].max())
        return refs, reads, scores, min_score
    return _cached("readmap", make)


# ---------------------------------------------------------------------------------------
# 2. the best query of every target
BQ_NQ = [1, 2, 3, 16, 17, 257, 4097]
BQ_N = [1, 63, 64, 65, 255, 257, 8191, 8193]
BQ_THIN = [(65536, 1), (65536, 5), (2, 70001)]
BQ_SHAPES = [(nq, n) for nq in BQ_NQ for n in BQ_N] + BQ_THIN
# What column c holds (pattern (c + shift) % 8), over a background of few values (ties abound):
BQ_PATTERNS = ("random", "all-equal", "max-last-row", "max-first-row", "tie-first-last",
               "int32-min", "int32-max", "extremes")
BQ_KEEP = 1 << 22  # matrices up to this many scores stay cached


def bq_scores(nq, n, shift=0):
    """The nq x n int32 matrix of a shape: the background is uniform in [-3, 12], and column c
    follows BQ_PATTERNS[(c + shift) % 8] (every 8 columns of the first 64 and of the last 8)."""
    def make():
        rng = np.random.default_rng([nq, n, shift])
        s = rng.integers(-3, 13, (nq, n), dtype=np.int32)
        cols = [c for c in range(n) if c < 64 or c >= n - 8]
        for c in cols:
            p = BQ_PATTERNS[(c + shift) % 8]
            if p == "all-equal":
                s[:, c] = 7
            elif p == "max-last-row":
                s[:, c] = np.minimum(s[:, c], 11)
                s[nq - 1, c] = 12
            elif p == "max-first-row":
                s[:, c] = np.minimum(s[:, c], 11)
                s[0, c] = 12
            elif p == "tie-first-last":
                s[:, c] = np.minimum(s[:, c], 11)
                s[0, c] = s[nq - 1, c] = 12
            elif p == "int32-min":
                s[:, c] = INT32_MIN
            elif p == "int32-max":
                s[:, c] = np.where(s[:, c] > 8, INT32_MAX, s[:, c])
                s[nq // 2, c] = INT32_MAX
            elif p == "extremes":
                s[:, c] = np.where(s[:, c] > 4, INT32_MAX, INT32_MIN)
        return s
    if nq * n > BQ_KEEP:
        return make()
    return _cached(("bq", nq, n, shift), make)


def bq_shifts(n):
    """Every pattern occurs in a matrix of >= 8 columns; a thinner one is drawn once per shift."""
    return range(1) if n >= 8 else range(0, 8, n)


def thresholded(best, min_score):
    """ref_best's pair under a threshold: QUERY_NONE / INT32_MIN where the maximum is below it."""
    bq, bs = best
    if min_score is None:
        return bq, bs
    below = bs < min_score
    return (np.where(below, QUERY_NONE, bq).astype(np.uint32),
            np.where(below, INT32_MIN, bs).astype(np.int32))


def ref_best(scores, min_score=None):
    """(best_query uint32, best_score int32): numpy's column maximum and its first occurrence."""
    s = np.asarray(scores, np.int32)
    return thresholded((s.argmax(0).astype(np.uint32), s.max(0)), min_score)


def bq_thresholds(scores, shift=0):
    """[None, INT32_MIN, m - 1, m, m + 1] for m the maximum of a background column (so the
    columns holding m exactly and those just below it both occur)."""
    nq, n = scores.shape
    c = next((c for c in range(n) if BQ_PATTERNS[(c + shift) % 8] == "random"), 0)
    m = int(scores[:, c].max())
    m = min(max(m, INT32_MIN + 1), INT32_MAX - 1)
    return [None, INT32_MIN, m - 1, m, m + 1]
