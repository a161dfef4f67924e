"""CPU: the skewed rows of the merged pair kernel, restated in plain Python and
checked against the oracle's merged recurrence.

Cell (i, j) of a tile is held in the frame of its anti-diagonal k = i + j: H^ = H + c_k and
T~ = G + c_k with c_k = e (k - 1), so the gap extension is paid by the frame and a row is

    A  = H^(i-1, j-1) + s + 2e
    T~ = max(A - o, T~(i-1, j), T~(i, j-1))
    H^ = max(T~, A, c_k)

The model below follows the kernel, not only the algebra: the query padded to whole 32-row waves
with the table's pad score, column -1 and row -1 as the frames' floors with T~ = -2048, one
running best per wave that moves with the frame (pairs H^(i-1, j) new / H^(i, j-1) old, step 2e,
(3 - R) e from a column's last pair to the next column's first), the fold of the last column's
odd rows and the unshift by the last frame's floor; and, as the plain and balanced kernels do,
it runs a target's last 8-column chunk whole, the columns past the target holding N (only the
trimmed kernel stops at a tile's last code), so the frames, the best and the unshift go on up
to 7 columns further.  Every value is rounded as f16 rounds it (exact up to 2048 on this scale)
and checked against the bound launch() uses to choose these rows, which counts the columns run.
Past that bound the rounding shows: test_past_the_bound_rounds keeps the case that the bound
with the bare target length would have let through."""
import numpy as np
import pytest

from oracle import oracle as O

R = 32
NEG = -2048


def f16(v):
    """v as the kernel holds it: an f16 multiple of 2^-11, exact for |v| <= 2048."""
    return v if -2048 <= v <= 2048 else int(float(np.float16(v / 2048.0)) * 2048.0)


def cols_run(L, trim=False):
    """Columns a tile of L-bp targets runs: whole 8-column chunks unless trimmed."""
    return L if trim else (L + 7) // 8 * 8


def bound(sub, m, L, e, trim=False):
    """launch()'s bound on the largest value a skewed column holds (it takes trim = False)."""
    smax = max(0, int(sub.max()))
    rows = (m + R - 1) // R * R
    return smax * min(m, L) + smax + e * (rows + cols_run(L, trim))


def most_negative(sub, m, o, e):
    """prepare()'s skew_neg: A - o in the first frame, A = c_{-2} + min(s, pad) + 2e."""
    smax = max(0, int(sub.max()))
    spad = -min(2048 - 2 * e, smax * max(m, 1))
    return -3 * e + min(int(sub.min()), spad) + 2 * e - o


def skew_score(q, t, sub, go, ge, trim=False, pad=4):
    """(score, lowest, highest value formed) of one pair by the skewed rows."""
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

    h = [c(r - 1) for r in range(rows)]  # column -1: H = 0 in every row's frame
    tt = [NEG] * rows
    best = [h[w * R + R - 2] for w in range(rows // R)]
    lo, hi = 0, 0
    for j in range(n):
        tj = t[j]
        diag, up = c(j - 2), NEG  # row -1: H = 0 in column j - 1's frame
        for i in range(rows):
            a = f16(diag + srow[i][tj] + 2 * e)
            ao = f16(a - o)
            tn = max(ao, up, tt[i])
            w, r = divmod(i, R)
            if r % 2 == 0:
                best[w] = f16(best[w] + ((3 - R) * e if r == 0 else 2 * e))
            else:  # both in frame i + j - 1: row i - 1 of this column, row i of the last one
                best[w] = max(best[w], h[i - 1], h[i])
            hn = max(tn, a, c(i + j))
            lo = min(lo, ao, best[w])
            hi = max(hi, hn, tn, best[w])
            diag, h[i] = h[i], hn
            up = tt[i] = tn
    score = 0
    for w in range(rows // R):
        bb = best[w]
        for r in range(1, R, 2):  # the last column's odd rows
            bb = max(f16(bb + ((3 - R) * e if r == 1 else 2 * e)), h[w * R + r])
            lo, hi = min(lo, bb), max(hi, bb)
        score = max(score, f16(bb - c(w * R + R - 1 + n - 1)))
    return score, lo, hi


PENS = [(5, -4, -12, -4)] * 5 + [(5, -4, -20, -1), (2, -3, -16, -8), (1, -1, -2, -2)]


def _cases():
    rng = np.random.default_rng(20260)
    out = []
    for it in range(400):
        m = int(rng.choice([2, 3, 7, 8, 16, 31, 32, 33, 64, 100, 127, 128],
                           p=[.12, .1, .1, .1, .12, .1, .1, .06, .08, .04, .04, .04]))
        n = int(rng.integers(1, 151))
        q = rng.integers(0, 4, m).astype(np.uint8)
        q[rng.random(m) < .05] = 4
        kind = it % 4
        if kind == 0:
            t = rng.integers(0, 4, n).astype(np.uint8)
        else:  # homologous: the query repeated, point changes and N, often a deletion
            t = np.resize(q, n).copy()
            x = rng.random(n) < .1
            t[x] = rng.integers(0, 5, int(x.sum()))
            if kind == 2 and n > 10:
                a = int(rng.integers(1, n - 5))
                t = np.delete(t, slice(a, a + int(rng.integers(1, 5))))
            if kind == 3 and n > 10:  # an insertion
                a = int(rng.integers(1, n - 1))
                t = np.insert(t, a, rng.integers(0, 4, int(rng.integers(1, 4))))[:150]
        if it % 50 == 49:
            t[:] = 4  # all N
        pen = PENS[it % len(PENS)]
        while bound(O.dna_matrix(*pen[:2]), m, len(t), -pen[3]) > 2048:
            t = t[:-1]  # (e = 8: the longest target launch() would still take)
        out.append((q, t.astype(np.uint8), pen))
    return out


def test_skewed_rows_match_the_oracle():
    cases = _cases()
    assert len(cases) == 400
    worst_lo, worst_hi = 0, 0
    for q, t, (ma, mi, go, ge) in cases:
        sub = O.dna_matrix(ma, mi)
        want = int(O.score_batch(q, t, np.zeros(1, np.uint64), np.array([len(t)], np.uint32),
                                 sub, go, ge)[0])
        got, lo, hi = skew_score(q.tolist(), t.tolist(), sub, go, ge)
        assert got == want, (len(q), len(t), (ma, mi, go, ge), got, want)
        top = bound(sub, len(q), len(t), -ge)
        assert top <= 2048, (len(q), len(t), top)  # (every case is one launch() would take)
        assert hi <= top and lo >= most_negative(sub, len(q), -go, -ge) >= -2048, (lo, hi, top)
        worst_lo, worst_hi = min(worst_lo, lo), max(worst_hi, hi)
    assert worst_hi > 1200  # (the cases reach the upper part of the range)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9])
def test_short_targets_fold_the_last_column(n):
    """Targets of one chunk or less: most cells are folded by the tile-end pass or against the
    virtual column -1."""
    sub = O.dna_matrix(5, -4)
    for seed in range(8):
        q = O.random_codes(seed, 33, 4)
        t = q[5:5 + n].copy() if seed % 2 else O.random_codes(100 + seed, n, 4)
        want = int(O.score_batch(q, t, np.zeros(1, np.uint64), np.array([n], np.uint32), sub,
                                 -12, -4)[0])
        assert skew_score(q.tolist(), t.tolist(), sub, -12, -4)[0] == want


def _edge_pair(m, L, hit):
    """A query of m rows and an L-bp target whose last `hit` bases repeat the query's last
    `hit`: the best ends in the last wave's last rows at the last real column."""
    q = O.random_codes(m, m, 4)
    t = O.random_codes(L, L, 4)
    t[L - hit:] = q[m - hit:]
    return q, t


@pytest.mark.parametrize("m,L", [(100, 249), (100, 250), (100, 251), (100, 252), (100, 256),
                                 (128, 209), (128, 210), (128, 212), (128, 216), (33, 393)])
def test_at_the_bound(m, L):
    """The longest targets launch() still takes, lengths that leave 4-7 pad columns: odd and
    even near-maximal scores ending in the last wave, every value exact."""
    sub = O.dna_matrix(5, -4)
    top = bound(sub, m, L, 4)
    assert top <= 2048 < bound(sub, m, cols_run(L) + 1, 4)  # (the last chunk under the bound)
    for hit in (m, m - 1, m - 2, m - 5):
        q, t = _edge_pair(m, L, hit)
        want = int(O.score_batch(q, t, np.zeros(1, np.uint64), np.array([L], np.uint32), sub,
                                 -12, -4)[0])
        assert want >= 5 * hit
        got, lo, hi = skew_score(q.tolist(), t.tolist(), sub, -12, -4)
        assert got == want and hi <= top and lo >= most_negative(sub, m, 12, 4), (got, want, hi)


def test_past_the_bound_rounds():
    """100 rows x 257 bp: 505 + 4 (128 + 257) = 2045 would pass with the bare length, but the
    plain and balanced kernels run 264 columns, the best reaches 2051 in the tile-end fold and
    rounds: a 99-match hit scores 496.  The bound with the columns run refuses the batch; the
    trimmed kernel, which stops at column 256, stays exact and inside its own count."""
    sub = O.dna_matrix(5, -4)
    m, L = 100, 257
    assert bound(sub, m, L, 4, trim=True) <= 2048 < bound(sub, m, L, 4)
    q, t = _edge_pair(m, L, 99)
    want = int(O.score_batch(q, t, np.zeros(1, np.uint64), np.array([L], np.uint32), sub, -12,
                             -4)[0])
    assert want == 495
    got, _, hi = skew_score(q.tolist(), t.tolist(), sub, -12, -4)
    assert hi > 2048 and got != want  # (what the kernel would return: 496)
    got, _, hi = skew_score(q.tolist(), t.tolist(), sub, -12, -4, trim=True)
    assert got == want and hi <= bound(sub, m, L, 4, trim=True)
