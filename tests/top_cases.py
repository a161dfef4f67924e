"""Inputs and the reference of the top-hits tests (a helper, not a test module; no GPU import).

sw_top_hits[_device] returns, per row of a score matrix, the k best batch positions: score
descending, then position ascending, among the scores >= min_score (include/swbank.h).  That is
the head of a stable descending sort of the row, which is what ``ref_top`` computes with numpy.
``mutant_top`` is the same with the highest positions first among equal scores: the answer of a
selection that cuts a run of equal scores at the wrong end (or in no order at all), which is how
a tie rule is most easily got wrong.

A group is one score matrix [nq, n] with the (k, min_score) pairs run on it; ``GROUPS`` names
them by family, ``group(name)`` builds (and caches) one, ``cases()`` yields every
(name, scores, k, min_score).  Families:

  sizes      n at and around the wave (64), the workgroup's 16-byte groups (256), its scores
             (2048 x 4 = 8192: 2047..2049 stay in one workgroup, 100,003 and up take several)
             and the headline batch; k at and around the same edges and n itself.  Scores are
             uniform in [30, 80): a DNA batch's band, thousands of ties at the cut.
  allequal   the answer is the first k positions: every digit of the cut lies in the position
             half of the key.
  hightie    the cut lies in a run of equal scores that crosses position 65,536.
  digits     the cut's deciding digit in each byte of the score; the int32 extremes; any int32.
  monotone   the best at the far or the near end of every workgroup's share.
  threshold  min_score above, at, just above the k-th value, and below the minimum.
  rows       several rows with an odd stride (row starts 4-byte aligned only).
"""
import functools

import numpy as np

TOP_MAX_K = 4096
HIT_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
INT32_MIN = -(1 << 31)
INT32_MAX = (1 << 31) - 1

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 100_003, 1_021_952, (1 << 20) + 1)


def stable_order(row):
    """Positions of a row by score descending, then position ascending."""
    return np.argsort(-np.asarray(row).astype(np.int64), kind="stable")


def mutant_order(row):
    """... by score descending, then position DESCENDING (the wrong end of every tie)."""
    row = np.asarray(row)
    return len(row) - 1 - np.argsort(-row[::-1].astype(np.int64), kind="stable")


def key64(row):
    """The kernels' key: (score ^ 0x80000000) << 32 | (2^32 - 1 - position)."""
    row = np.asarray(row, np.int32)
    hi = (row.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    return hi << np.uint64(32) | (np.uint64(0xFFFFFFFF) - np.arange(len(row), dtype=np.uint64))


def _top(scores, k, min_score, order_of, orders):
    scores = np.asarray(scores, np.int32)
    rows = scores.reshape(1, -1) if scores.ndim == 1 else scores
    nq, n = rows.shape
    hits = np.full((nq, k), HIT_NONE, np.uint64)
    hsc = np.full((nq, k), INT32_MIN, np.int32)
    cnt = np.zeros(nq, np.uint32)
    for i in range(nq):
        order = orders[i] if orders is not None else order_of(rows[i])
        head = order[:min(k, n)]
        if min_score is not None:
            head = head[rows[i][head] >= min_score]
        cnt[i] = len(head)
        hits[i, :len(head)] = head
        hsc[i, :len(head)] = rows[i][head]
    return hits, hsc, cnt


def ref_top(scores, k, min_score=None, orders=None):
    """(hits [nq, k] uint64, hit_scores [nq, k] int32, counts [nq] uint32) of scores [nq, n] (or
    [n]): the first min(k, n) entries of the stable descending sort of each row that reach
    min_score; the slots past the count hold HIT_NONE / INT32_MIN.  `orders`: the rows'
    stable_order, when the caller has them already."""
    return _top(scores, k, min_score, stable_order, orders)


def mutant_top(scores, k, min_score=None, orders=None):
    """ref_top with the highest positions first among equal scores."""
    return _top(scores, k, min_score, mutant_order, orders)


def band(rng, n):
    return rng.integers(30, 80, n).astype(np.int32)


def _ks(n):
    ks = []
    for k in (1, 2, 63, 64, 65, 4096, n - 1, n, n + 5):
        if 1 <= k <= TOP_MAX_K and k not in ks:
            ks.append(k)
    return ks


def _sizes(n):
    return band(np.random.default_rng([1, n]), n)[None, :], [(k, None) for k in _ks(n)]


def _allequal(n):
    return np.full((1, n), 47, np.int32), [(k, None) for k in (1, 255, 256, 257, 4096)]


def _hightie():
    s = np.zeros((1, 70_000), np.int32)
    s[0, 65_500:65_601] = 5
    return s, [(50, None)]


def _digit(b):
    rng = np.random.default_rng([2, b])
    d = rng.integers(0, 256, 5000).astype(np.int64)
    v = (0x01020304 + (d << (8 * b))) & 0xFFFFFFFF
    return v.astype(np.uint32).view(np.int32)[None, :], [(100, None)]


def _extremes():
    rng = np.random.default_rng(3)
    vals = np.array([INT32_MIN, INT32_MAX, -1, 0, 1], np.int64)
    return vals[rng.integers(0, 5, 5000)].astype(np.int32)[None, :], [(100, None), (4096, None)]


def _anyint():
    rng = np.random.default_rng(4)
    s = rng.integers(INT32_MIN, INT32_MAX + 1, 5000, dtype=np.int64).astype(np.int32)
    return s[None, :], [(100, None)]


def _monotone(sign):
    return (sign * (np.arange(20_000, dtype=np.int64) * 3 - 30_000)).astype(np.int32)[None, :], \
        [(100, None)]


def _threshold():
    s = band(np.random.default_rng(5), 5000)
    kth = int(np.sort(s)[::-1][299])  # (about 100 targets per score: the third value from the top)
    return s[None, :], [(300, int(s.max()) + 1), (300, kth), (300, kth + 1), (300, int(s.min()) - 1)]


def _rows(nq, n, k):
    rng = np.random.default_rng([6, nq, n])
    s = np.empty((nq, n), np.int32)
    for i in range(nq):
        if i % 3 == 0:
            s[i] = 47 + i
        elif i % 3 == 1:
            s[i] = band(rng, n)
        else:
            s[i] = rng.integers(INT32_MIN, INT32_MAX + 1, n, dtype=np.int64).astype(np.int32)
    return s, [(k, None), (k, 50)]


GROUPS = {}
for _n in SIZES:
    GROUPS[f"sizes-{_n}"] = functools.partial(_sizes, _n)
for _n in (257, 100_003):
    GROUPS[f"allequal-{_n}"] = functools.partial(_allequal, _n)
GROUPS["hightie"] = _hightie
for _b in range(4):
    GROUPS[f"digits-byte{_b}"] = functools.partial(_digit, _b)
GROUPS["digits-extremes"] = _extremes
GROUPS["digits-anyint32"] = _anyint
GROUPS["monotone-up"] = functools.partial(_monotone, 1)
GROUPS["monotone-down"] = functools.partial(_monotone, -1)
GROUPS["threshold"] = _threshold
GROUPS["rows-3x2049"] = functools.partial(_rows, 3, 2049, 65)
GROUPS["rows-16x4099"] = functools.partial(_rows, 16, 4099, 200)

# families in which some case cuts a run of equal scores
TIE_FAMILIES = ("sizes", "allequal", "hightie", "digits", "threshold", "rows")


@functools.lru_cache(maxsize=None)
def group(name):
    """(scores [nq, n] int32, [(k, min_score)], [stable_order of each row]) of a group; shared
    by the tests and left unchanged."""
    scores, runs = GROUPS[name]()
    scores.setflags(write=False)
    return scores, runs, [stable_order(r) for r in scores]


def family(name):
    return name.split("-")[0]


def cases(names=None):
    """(case name, scores [nq, n], k, min_score) of every case (of the groups `names`)."""
    for g in names or GROUPS:
        scores, runs, _ = group(g)
        for k, ms in runs:
            yield f"{g}/k{k}" + ("" if ms is None else f"/min{ms}"), scores, k, ms


def golden_scores(path):
    """(names, scores) of the ssearch36 -R lines of tests/golden/score500_R_lines.txt."""
    rows = [ln.split() for ln in open(path) if ln.strip()]
    return [r[0] for r in rows], np.array([int(r[5]) for r in rows], np.int32)


GOLDEN_TOP12 = [("db211", 78), ("db428", 72), ("db454", 70), ("db263", 69), ("db278", 69),
                ("db419", 69), ("db123", 67), ("db465", 67), ("db169", 65), ("db15", 64),
                ("db339", 64), ("db125", 63)]
