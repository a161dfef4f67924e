"""The inputs of the best-query tests (tests/set_cases.py), checked on the CPU: the matrices hold
what they are meant to hold, and they tell the reference (numpy's column maximum, its first
occurrence, a threshold of "maximum < min_score") from the two likely wrong selections: one that
keeps the highest query on a tie, and one that compares with <= against the threshold."""
import numpy as np
import pytest

import set_cases as SC

SMALL = [(nq, n) for nq, n in SC.BQ_SHAPES if nq * n <= 1 << 18]


def _highest_on_tie(scores, min_score=None):
    s = np.asarray(scores, np.int32)
    bs = s.max(0)
    bq = (s.shape[0] - 1 - s[::-1].argmax(0)).astype(np.uint32)
    if min_score is not None:
        bq = np.where(bs < min_score, SC.QUERY_NONE, bq).astype(np.uint32)
        bs = np.where(bs < min_score, SC.INT32_MIN, bs).astype(np.int32)
    return bq, bs


def _le_threshold(scores, min_score=None):
    s = np.asarray(scores, np.int32)
    bs = s.max(0)
    bq = s.argmax(0).astype(np.uint32)
    if min_score is not None and min_score != SC.INT32_MIN:
        bq = np.where(bs <= min_score, SC.QUERY_NONE, bq).astype(np.uint32)
        bs = np.where(bs <= min_score, SC.INT32_MIN, bs).astype(np.int32)
    return bq, bs


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_shapes():
    assert len(SC.BQ_SHAPES) == 7 * 8 + 3 == len(set(SC.BQ_SHAPES))
    assert {n % 4 for _, n in SC.BQ_SHAPES} == {0, 1, 3}  # rows start at other 4-byte phases
    assert (65536, 1) in SC.BQ_SHAPES and (2, 70001) in SC.BQ_SHAPES
    assert len(SMALL) >= 40


@pytest.mark.parametrize("nq,n", SMALL)
def test_patterns_hold(nq, n):
    seen = set()
    for shift in SC.bq_shifts(n):
        s = SC.bq_scores(nq, n, shift)
        assert s.shape == (nq, n) and s.dtype == np.int32
        bq, bs = SC.ref_best(s)
        for c in range(min(n, 64)):
            p = SC.BQ_PATTERNS[(c + shift) % 8]
            seen.add(p)
            col = s[:, c]
            if p == "all-equal":
                assert (col == 7).all() and bq[c] == 0
            elif p == "max-last-row":
                assert bq[c] == nq - 1 and bs[c] == 12 and (col[:-1] < 12).all()
            elif p == "max-first-row":
                assert bq[c] == 0 and bs[c] == 12 and (nq == 1 or (col[1:] < 12).all())
            elif p == "tie-first-last":
                assert bq[c] == 0 and col[0] == col[-1] == 12
            elif p == "int32-min":
                assert (col == SC.INT32_MIN).all() and bq[c] == 0 and bs[c] == SC.INT32_MIN
            elif p == "int32-max":
                assert bs[c] == SC.INT32_MAX and col[bq[c]] == SC.INT32_MAX
                assert (col[:bq[c]] < SC.INT32_MAX).all()
    assert seen == set(SC.BQ_PATTERNS) or (n < 8 and len(seen) == min(8, n * len(SC.bq_shifts(n))))


def test_cases_tell_the_selections_apart():
    ties = thresholds = 0
    for nq, n in SMALL:
        for shift in SC.bq_shifts(n):
            s = SC.bq_scores(nq, n, shift)
            for ms in SC.bq_thresholds(s, shift):
                want = SC.ref_best(s, ms)
                # the threshold's two outputs agree, and INT32_MIN is no threshold
                assert np.array_equal(want[0] == SC.QUERY_NONE, s.max(0) < (
                    SC.INT32_MIN if ms is None else ms))
                ties += not _same(want, _highest_on_tie(s, ms))
                thresholds += not _same(want, _le_threshold(s, ms))
            assert _same(SC.ref_best(s, SC.INT32_MIN), SC.ref_best(s, None))
    # every shape with more than one query has tied columns; the threshold at a column's maximum
    # separates < from <= wherever a column holds exactly it
    assert ties >= sum(1 for nq, _ in SMALL if nq > 1)
    assert thresholds >= len(SMALL) // 2


def test_thresholds_straddle_a_maximum():
    s = SC.bq_scores(17, 257)
    none, lowest, below, at, above = SC.bq_thresholds(s)
    assert none is None and lowest == SC.INT32_MIN and (below + 1, above - 1) == (at, at)
    best = s.max(0)
    assert (best == at).any() and (best < at).any() and (best > at).any()
