"""CPU: the block-framed skewed rows of the merged pair kernel, restated in plain
Python and checked against the oracle.  tests/test_skew_model.py stays as the record of the rows
before them (one frame per anti-diagonal over all 32 rows of a wave).

Cell (i, j), i the query row and j the tile column, is held in frame f = (i mod 8) + j:
H^ = H + c(f), T~ = G + c(f), c(k) = e (k - 1).  Rows with i mod 8 != 0 are the old rows,

    A  = H^(i-1, j-1) + s + 2e      T~ = max(A - o, T~up, T~left)      H^ = max(T~, A, c(f))

and a block's first row (i mod 8 = 0), whose upper neighbours sit 7 frames on, takes the table
word s + 2e - 8e and T~up - 8e.  Rows u, u + 8, u + 16, u + 24 of a column share frame u + j, so
a wave folds them with two max, no move between them, into accumulator u // 2 (four
accumulators: one + e move per accumulator and column, none from a column to the next, since
class 2a of column j + 1 has the frame of class 2a + 1 of column j).

The model follows the kernel, not only the algebra: the query padded to whole 32-row waves with
the table's pad score, column -1 and row -1 as the frames' floors with T~ = -2048 (row -1's
becomes -2048 - 8e by the shift of row 0: exact, and below every A - o), the accumulators
starting at their frames' floors,
the last accumulator's second half of a column (move, class 7) run at the start of the next
column as the generated rows place it, the tile-end merge of the accumulators into the last
frame and the unshift by its floor; the plain and balanced kernels run a target's last 8-column
chunk whole, the trimmed one stops at the last code.  The form with one accumulator (8 moves per
column) is checked too.  Every formed value is rounded as f16 rounds it.

Range.  The frames reach 7 + cols instead of rows + cols, so every value stays under the bound
launch() keeps using (that of the old rows).  prepare()'s skew_neg is the lowest value that must
be exact: A - o of a block's first row in frame 0, min(s, pad) - e - o, the old figure.  One
value can lie below it, by at most e: the shifted T~up of a row whose own A - o sits at that
minimum.  It is a T~ far below every floor (floors are >= -2e), it only ever enters max and
further -8e shifts, so if it rounds (below -2048, in steps of 2) whatever derives from it stays
below -2047 and never reaches an H^; test_shifted_up_below_the_range_is_harmless keeps a case."""
import numpy as np
import pytest

from oracle import oracle as O
import seam_cases as SC
from test_skew_model import _cases, _edge_pair, bound, cols_run, f16, most_negative

R = 32
NEG = -2048
NACC = 4  # the kernel's accumulator count (SWK_SKEW_ACC)


def block_score(q, t, sub, go, ge, nacc=NACC, trim=False, pad=4, shift=True):
    """(score, lowest A - o / best, lowest shifted T~up, highest value formed) of one pair by the
    block-framed rows.  shift=False leaves the -8e of T~up out (the mutant of the last test)."""
    o, e = -go, -ge
    m = len(q)
    t = list(t) + [pad] * (cols_run(len(t), trim) - len(t))
    n = len(t)
    rows = (m + R - 1) // R * R
    smax = max(0, int(sub.max()))
    spad = -min(2048 - 2 * e, smax * max(m, 1))
    srow = [[int(sub[a][b]) for b in range(sub.shape[1])] for a in q] + \
        [[spad] * sub.shape[1]] * (rows - m)

    def c(k):
        return e * (k - 1)

    h = [c(i % 8 - 1) for i in range(rows)]  # column -1: H = 0 in every row's frame
    tt = [NEG] * rows
    W = rows // R
    if nacc == 4:   # accumulator a starts column 0 in frame 2a; the last one a move earlier
        acc = [[c(0), c(2), c(4), c(5)] for _ in range(W)]
    else:           # one accumulator: -6e at each column's start, from frame 7 + (j - 1) to j
        acc = [[c(6)] for _ in range(W)]
    lo, lo_up, hi = 0, 0, 0

    def fold(w, a, u):  # rows of class u of wave w into accumulator a
        b = w * R + u
        acc[w][a] = max(acc[w][a], h[b], h[b + 8], h[b + 16], h[b + 24])

    def move(w, a, d):
        nonlocal lo, hi
        acc[w][a] = f16(acc[w][a] + d)
        lo, hi = min(lo, acc[w][a]), max(hi, acc[w][a])

    for j in range(n):
        tj = t[j]
        for w in range(W):  # what a column's first block does before it overwrites the rows
            if nacc == 4:
                move(w, 3, e)
                fold(w, 3, 7)
            else:
                move(w, 0, -6 * e)
        diag, up = c(j + 6), NEG  # row -1: H = 0 in frame 7 + (j - 1), T~ never wins
        for i in range(rows):
            first = i % 8 == 0
            a = f16(diag + srow[i][tj] + (2 * e - 8 * e if first else 2 * e))
            ao = f16(a - o)
            if first and shift:
                up = f16(up - 8 * e)
                lo_up = min(lo_up, up) if i > 0 else lo_up
            tn = max(ao, up, tt[i])
            hn = max(tn, a, c(i % 8 + j))
            lo = min(lo, ao)
            hi = max(hi, hn, tn)
            diag, h[i] = h[i], hn
            up = tt[i] = tn
        for w in range(W):  # the folds of the column's last block
            if nacc == 4:
                for a in range(4):
                    fold(w, a, 2 * a)
                    if a < 3:
                        move(w, a, e)
                        fold(w, a, 2 * a + 1)
            else:
                for u in range(8):
                    fold(w, 0, u)
                    if u < 7:
                        move(w, 0, e)
            hi = max(hi, max(acc[w]))
    score = 0
    for w in range(W):  # the tile's end: every accumulator into frame 7 + (n - 1), then out
        if nacc == 4:
            move(w, 3, e)
            fold(w, 3, 7)
            bb = acc[w][3]
            for a in range(3):
                v = f16(acc[w][a] + (6 - 2 * a) * e)
                hi = max(hi, v)
                bb = max(bb, v)
        else:
            bb = acc[w][0]
        score = max(score, f16(bb - c(7 + n - 1)))
    return score, lo, lo_up, hi


def _oracle(q, t, sub, go, ge):
    return int(O.score_batch(np.asarray(q, np.uint8), np.asarray(t, np.uint8),
                             np.zeros(1, np.uint64), np.array([len(t)], np.uint32), sub, go,
                             ge)[0])


@pytest.mark.parametrize("nacc", [NACC, 1])
def test_block_rows_match_the_oracle(nacc):
    cases = _cases()
    assert len(cases) == 400
    worst_hi = 0
    for q, t, (ma, mi, go, ge) in cases:
        sub = O.dna_matrix(ma, mi)
        want = _oracle(q, t, sub, go, ge)
        for trim in (False, True):
            got, lo, lo_up, hi = block_score(q.tolist(), t.tolist(), sub, go, ge, nacc, trim)
            assert got == want, (len(q), len(t), (ma, mi, go, ge), trim, got, want)
            top = bound(sub, len(q), len(t), -ge)
            neg = most_negative(sub, len(q), -go, -ge)
            assert top <= 2048 and neg >= -2048  # (every case is one launch() would take)
            assert hi <= top and lo >= neg and lo_up >= neg + ge, (lo, lo_up, hi, top, neg)
            # the frames need less range than the bound grants: 8 rows of offsets, not all
            rows = (len(q) + R - 1) // R * R
            assert hi <= top + ge * (rows - 8)
        worst_hi = max(worst_hi, hi)
    assert worst_hi > 900  # (the cases reach the upper part of the range)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9])
def test_short_targets(n):
    """Targets of one chunk or less: most cells are folded in the first columns or by the
    tile-end pass."""
    sub = O.dna_matrix(5, -4)
    for seed in range(8):
        q = O.random_codes(seed, 33, 4)
        t = q[5:5 + n].copy() if seed % 2 else O.random_codes(100 + seed, n, 4)
        want = _oracle(q, t, sub, -12, -4)
        for nacc in (NACC, 1):
            for trim in (False, True):
                assert block_score(q.tolist(), t.tolist(), sub, -12, -4, nacc, trim)[0] == want


@pytest.mark.parametrize("m,L", [(100, 249), (100, 250), (100, 251), (100, 252), (100, 256),
                                 (128, 209), (128, 210), (128, 212), (128, 216), (33, 393)])
def test_at_the_bound(m, L):
    """The longest targets launch() still takes (its bound is unchanged): near-maximal odd and
    even scores ending in the last wave, every value exact and well inside the range."""
    sub = O.dna_matrix(5, -4)
    top = bound(sub, m, L, 4)
    assert top <= 2048 < bound(sub, m, cols_run(L) + 1, 4)
    for hit in (m, m - 1, m - 2, m - 5):
        q, t = _edge_pair(m, L, hit)
        want = _oracle(q, t, sub, -12, -4)
        assert want >= 5 * hit
        for nacc in (NACC, 1):
            got, lo, lo_up, hi = block_score(q.tolist(), t.tolist(), sub, -12, -4, nacc)
            neg = most_negative(sub, m, 12, 4)
            assert got == want and hi <= top and lo >= neg and lo_up >= neg - 4, (got, want, hi)


def test_every_row_and_column_class_holds_the_best():
    """A 12-row exact copy ending at (r, c) for all 64 (r mod 8, c mod 8), r over block and wave
    boundary rows: the best is made in every accumulator, every fold and both column halves."""
    sub = O.dna_matrix(5, -4)
    q = O.random_codes(5, 128, 4)
    seen, turn = set(), [0] * 8
    for r in range(11, 128):
        c = 16 + turn[r % 8] % 16  # (every column class in turn for this row class)
        turn[r % 8] += 1
        t = (q[:c + 1][::-1].copy() + 1) % 4  # (no accidental long match elsewhere)
        t[c - 11:c + 1] = q[r - 11:r + 1]
        t = np.concatenate([t, (q[r + 1:r + 9] + 2) % 4]) if r + 9 <= 128 else t
        want = _oracle(q, t, sub, -12, -4)
        assert want >= 60
        for trim in (False, True):
            assert block_score(q.tolist(), t.tolist(), sub, -12, -4, NACC, trim)[0] == want
        seen.add((r % 8, c % 8))
    assert len(seen) == 64


def test_shifted_up_below_the_range_is_harmless():
    """Where the shifted T~up can leave the range at all: a huge open (1 / -1 / -2028 / -3, still
    inside prepare()'s f16 range o + 2e + S - smin <= 2048) and 17 rows, so that skew_neg =
    -17 - 3 - 2028 = -2048 is still taken.  In column 0 the pad rows 17-23 above block-first row
    24 hold nothing better than their own A - o, and T~up - 8e falls below -2048, past the exact range.
    It never reaches an H^: every score is the oracle's."""
    pens = (1, -1, -2028, -3)
    sub = O.dna_matrix(*pens[:2])
    m = 17
    assert most_negative(sub, m, 2028, 3) == -2048
    assert 2028 + 2 * 3 + int(sub.max()) - int(sub.min()) <= 2048
    q = O.random_codes(3, m, 4)
    rng = np.random.default_rng(9)
    below = 0
    for L in (1, 8, 16, 30, 40, 150):
        for k in range(4):
            t = rng.integers(0, 4, L).astype(np.uint8)
            if k % 2 and L >= 16:
                t[4:16] = q[2:14]
            assert bound(sub, m, L, 3) <= 2048
            got, lo, lo_up, _ = block_score(q.tolist(), t.tolist(), sub, *pens[2:])
            assert lo >= -2048 and lo_up >= -2048 - 3 - 1  # (-2051 held as -2052)
            assert got == _oracle(q, t, sub, *pens[2:])
            below += lo_up < -2048
    assert below >= 12


def test_leaving_the_boundary_shift_out_shows():
    """The rows with T~up taken unshifted at a block's first row (8e too high: a gap that
    crosses into a block looks 8e cheaper) against the oracle, on deletion targets whose
    vertical gap run straddles rows 7|8 ... 95|96 (tests/seam_cases.py, 8 per cut): measured, the
    mutant changes 48 of 48 scores (100 %, 8 of 8 at every cut) at 5/-4/-12/-4 and at 2/-3/-16/-8
    (e = 8) alike; asserted >= 90 %: a margin of 4 targets of 48, so rows that lost the shift at
    one of the six cuts (8 targets unchanged) already fail."""
    cuts = [8, 16, 24, 32, 64, 96]
    for pens in ((5, -4, -12, -4), (2, -3, -16, -8)):
        sub = O.dna_matrix(*pens[:2])
        rng = np.random.default_rng(77)
        for attempt in range(64):
            q = rng.integers(0, 4, 128).astype(np.uint8)
            try:
                tg, meta = SC.straddle_targets(q, 4, cuts, [], None, rng, per=8)
                break
            except ValueError:
                continue
        while bound(sub, 128, max(len(t) for t in tg), -pens[3]) > 2048:
            tg = [t[:-8] for t in tg]  # (e = 8: the longest target launch() takes)
        changed = 0
        for t in tg:
            want = _oracle(q, t, sub, *pens[2:])
            assert block_score(q.tolist(), t.tolist(), sub, *pens[2:])[0] == want
            changed += block_score(q.tolist(), t.tolist(), sub, *pens[2:], shift=False)[0] != want
        assert len(tg) == 48 and changed >= 0.9 * len(tg), (pens, changed, len(tg))
