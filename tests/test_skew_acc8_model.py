"""CPU: the skewed rows' running best with eight renamed accumulators, restated in
plain Python and checked against the oracle.  tests/test_skew_block_model.py stays as the record
of the four accumulators (which the trimmed kernel keeps) and of one.

The rows are those of test_skew_block_model.py: cell (i, j) in frame f = (i mod 8) + j.  The
best has one accumulator per frame, named by the frame mod 8: class u = i mod 8 of column j folds
into b[(u + j) mod 8], and an accumulator stays with its frame from column to column.  Frame j
leaves after column j; its accumulator takes frame j + 8, class 7 of column j + 1: one + 8e move
per column.  As the generated rows place it, column j's first block

    moves  b[(j + 7) mod 8]   (frame j - 1 left with column j - 1; the move makes it frame j + 7)
    folds class 7 of column j - 1 into b[(j + 6) mod 8]   (before it overwrites those rows)

and its last block folds classes 0-6.  After the 8 columns of a chunk the names are back where
they were, so the unrolled chunk needs no copies and a head / tail hand-off at a chunk boundary
carries the eight as they are.  The kernels with eight accumulators run a target's last chunk
whole, so the tile end always meets the same rotation: b[7] still in the frame that left with
the last column (its move belongs to the next column), b[0..6] in the 7 frames after it, class 7
of the last column not folded yet.  The merge goes up one e at a time from b[7] into the last
frame, 7 + (n - 1), and out by its floor.

The model follows the kernel: pad rows to whole 32-row waves, column -1 and row -1 as floors,
the accumulators starting at their frames' floors (b[7] a move before, frame -1), every formed
value rounded as f16 rounds it.

Range.  A moved accumulator holds a best H in the column's highest frame, as a cell of class 7
of that column could, so it stays under the bound launch() uses; the tile-end merge ends in the
frame the four-accumulator merge ends in."""
import numpy as np
import pytest

from oracle import oracle as O
from test_skew_model import _cases, _edge_pair, bound, cols_run, f16, most_negative

R = 32
NEG = -2048


def acc8_score(q, t, sub, go, ge, pad=4, move=True, rot=0):
    """(score, lowest A - o / accumulator, highest value formed) of one pair.  move=False leaves
    the + 8e move out, rot=1 names the last block's accumulators one frame on (the mutants)."""
    o, e = -go, -ge
    m = len(q)
    t = list(t) + [pad] * (cols_run(len(t)) - len(t))
    n = len(t)
    assert n % 8 == 0
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
    acc = [[c(k) for k in range(7)] + [c(-1)] for _ in range(W)]
    lo, hi = 0, 0

    def fold(w, a, u):  # rows of class u of wave w into accumulator a
        b = w * R + u
        acc[w][a] = max(acc[w][a], h[b], h[b + 8], h[b + 16], h[b + 24])

    for j in range(n):
        tj = t[j]
        for w in range(W):  # the column's first block, before it overwrites the rows
            if move:
                a = (j + 7) % 8
                acc[w][a] = f16(acc[w][a] + 8 * e)
                lo, hi = min(lo, acc[w][a]), max(hi, acc[w][a])
            fold(w, (j + 6) % 8, 7)
        diag, up = c(j + 6), NEG
        for i in range(rows):
            first = i % 8 == 0
            a = f16(diag + srow[i][tj] + (2 * e - 8 * e if first else 2 * e))
            ao = f16(a - o)
            if first:
                up = f16(up - 8 * e)
            tn = max(ao, up, tt[i])
            hn = max(tn, a, c(i % 8 + j))
            lo = min(lo, ao)
            hi = max(hi, hn, tn)
            diag, h[i] = h[i], hn
            up = tt[i] = tn
        for w in range(W):  # the folds of the column's last block
            for u in range(7):
                fold(w, (u + j + rot) % 8, u)
            hi = max(hi, max(acc[w]))
    score = 0
    for w in range(W):  # the tile's end, after a whole chunk: names 0-6 in frames n .. n + 6
        bb = acc[w][7]
        for k in range(6):
            bb = max(f16(bb + e), acc[w][k])
            hi = max(hi, bb)
        fold(w, 6, 7)
        bb = max(f16(bb + e), acc[w][6])
        hi = max(hi, bb)
        score = max(score, f16(bb - c(7 + n - 1)))
    return score, lo, hi


def _oracle(q, t, sub, go, ge):
    return int(O.score_batch(np.asarray(q, np.uint8), np.asarray(t, np.uint8),
                             np.zeros(1, np.uint64), np.array([len(t)], np.uint32), sub, go,
                             ge)[0])


def test_eight_accumulators_match_the_oracle():
    cases = _cases()
    assert len(cases) == 400
    worst_hi, chunks = 0, set()
    for q, t, (ma, mi, go, ge) in cases:
        sub = O.dna_matrix(ma, mi)
        want = _oracle(q, t, sub, go, ge)
        got, lo, hi = acc8_score(q.tolist(), t.tolist(), sub, go, ge)
        assert got == want, (len(q), len(t), (ma, mi, go, ge), got, want)
        top = bound(sub, len(q), len(t), -ge)
        neg = most_negative(sub, len(q), -go, -ge)
        assert top <= 2048 and neg >= -2048  # (every case is one launch() would take)
        assert hi <= top and lo >= neg, (lo, hi, top, neg)
        worst_hi = max(worst_hi, hi)
        chunks.add(min(cols_run(len(t)) // 8, 3))
    assert worst_hi > 900  # (the cases reach the upper part of the range)
    assert chunks == {1, 2, 3}  # (one chunk, and the rotation across one and more boundaries)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 15, 16, 17])
def test_short_targets_and_chunk_boundaries(n):
    """Targets of one chunk or just past a chunk boundary: most cells are folded in the first
    columns, by the pad columns of the whole last chunk or by the tile-end merge."""
    sub = O.dna_matrix(5, -4)
    for seed in range(8):
        q = O.random_codes(seed, 33, 4)
        t = q[5:5 + n].copy() if seed % 2 else O.random_codes(100 + seed, n, 4)
        want = _oracle(q, t, sub, -12, -4)
        assert acc8_score(q.tolist(), t.tolist(), sub, -12, -4)[0] == want


@pytest.mark.parametrize("m,L", [(100, 249), (100, 250), (100, 251), (100, 252), (100, 256),
                                 (128, 209), (128, 210), (128, 212), (128, 216), (33, 393)])
def test_at_the_bound(m, L):
    """The longest targets launch() still takes (its bound is unchanged): near-maximal odd and
    even scores ending in the last wave; the moved accumulators and the merge stay exact."""
    sub = O.dna_matrix(5, -4)
    top = bound(sub, m, L, 4)
    assert top <= 2048 < bound(sub, m, cols_run(L) + 1, 4)
    for hit in (m, m - 1, m - 2, m - 5):
        q, t = _edge_pair(m, L, hit)
        want = _oracle(q, t, sub, -12, -4)
        assert want >= 5 * hit
        got, lo, hi = acc8_score(q.tolist(), t.tolist(), sub, -12, -4)
        assert got == want and hi <= top and lo >= most_negative(sub, m, 12, 4), (got, want, hi)


def _placements(tail):
    """(r, c, q, t): a 12-row exact copy of q ending at row r, column c, for all 64 (r mod 8,
    c mod 8), followed by `tail` columns that match nothing nearby."""
    q = O.random_codes(5, 128, 4)
    turn = [0] * 8
    for r in range(11, 128):
        c = 16 + turn[r % 8] % 16  # (every column class in turn for this row class)
        turn[r % 8] += 1
        t = (q[:c + 1][::-1].copy() + 1) % 4  # (no accidental long match elsewhere)
        t[c - 11:c + 1] = q[r - 11:r + 1]
        ext = (np.resize(q[r + 1:r + 9], tail) + 2) % 4 if r + 9 <= 128 else \
            (np.resize(q[:8], tail) + 2) % 4
        yield r, c, q, np.concatenate([t, ext]).astype(np.uint8)


def test_every_row_and_column_class_holds_the_best():
    """The best made in every accumulator name, every fold and at every rotation; with the hit
    in the last columns run (the tile-end merge takes it from a low frame or from class 7's late
    fold) and with whole chunks after it (it crosses moves)."""
    sub = O.dna_matrix(5, -4)
    for tail in (0, 8, 24):
        seen = set()
        for r, c, q, t in _placements(tail):
            want = _oracle(q, t, sub, -12, -4)
            assert want >= 60
            assert acc8_score(q.tolist(), t.tolist(), sub, -12, -4)[0] == want, (r, c, tail)
            seen.add((r % 8, c % 8))
        assert len(seen) == 64


def test_leaving_the_move_out_shows():
    """Family: the 12-row copies of _placements with 24 unrelated columns after the hit.  The
    hit's cell sits in frame (r mod 8) + c <= c + 7, which has left the column at least 9
    columns before the tile's end, so its accumulator has been moved at least once: without the
    + 8e the best reads 8e low per move, and nothing later reaches it (the tail scores at most
    a few matches).  Every score of the family must change."""
    sub = O.dna_matrix(5, -4)
    fam = list(_placements(24))
    changed = 0
    for r, c, q, t in fam:
        want = _oracle(q, t, sub, -12, -4)
        got = acc8_score(q.tolist(), t.tolist(), sub, -12, -4, move=False)[0]
        assert got <= want
        changed += got != want
    print(f"move left out: {changed} of {len(fam)} scores change")
    assert len(fam) == 117 and changed == len(fam)


def test_a_rotation_off_by_one_shows():
    """Family: the same copies ending in the target's last column (no tail), by row class.  With
    the last block's names one frame on, classes 0-6 fold into the accumulator of the next frame
    and read e low; class 7, folded by the next first block (or the tile end), is not touched.
    So every hit ending in a row of classes 0-6 must change, by exactly e, and none of class 7."""
    sub = O.dna_matrix(5, -4)
    n_low, n7 = 0, 0
    for r, c, q, t in _placements(0):
        want = _oracle(q, t, sub, -12, -4)
        got = acc8_score(q.tolist(), t.tolist(), sub, -12, -4, rot=1)[0]
        if r % 8 == 7:
            assert got == want, (r, c)
            n7 += 1
        else:
            assert got == want - 4, (r, c, got, want)
            n_low += 1
    assert n7 >= 14 and n_low >= 100
