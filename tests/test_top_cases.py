"""The top-hits test inputs are what they claim to be (CPU only): they can tell a wrong tie cut
from the right one, the reference is the descending order of the kernels' 64-bit key, and the
ssearch36 scores of the golden library have the 12 best hits the GPU tests expect."""
import os

import numpy as np
import pytest

from oracle import oracle as O

import top_cases as TC


def _cut_splits_a_tie(scores, k, min_score, orders):
    """Whether some row's selection ends inside a run of equal scores."""
    for row, order in zip(scores, orders):
        head = order[:min(k, len(row))]
        if min_score is not None:
            head = head[row[head] >= min_score]
        if len(head) and int((row == row[head[-1]]).sum()) > int((row[head] == row[head[-1]]).sum()):
            return True
    return False


def test_the_cases_tell_a_wrong_tie_cut_from_the_right_one():
    seen = {f: 0 for f in TC.TIE_FAMILIES}
    for g in TC.GROUPS:
        scores, runs, orders = TC.group(g)
        for k, ms in runs:
            same = all((a == b).all() for a, b in zip(TC.ref_top(scores, k, ms, orders),
                                                      TC.mutant_top(scores, k, ms)))
            split = _cut_splits_a_tie(scores, k, ms, orders)
            assert not (split and same), (g, k, ms)  # (ties inside the head differ in order too)
            if split and TC.family(g) in seen:
                seen[TC.family(g)] += 1
    assert all(seen.values()), seen
    # the families built around one tie: every case of theirs splits it
    for g in ("allequal-257", "allequal-100003", "hightie", "rows-3x2049", "rows-16x4099"):
        scores, runs, orders = TC.group(g)
        for k, ms in runs:
            if k < scores.shape[1]:
                assert _cut_splits_a_tie(scores, k, ms, orders), (g, k, ms)
    # the sizes family: about n / 50 = 2,000 targets share the 4,096th score of 100,003, and the
    # cut falls inside that run
    scores, _, orders = TC.group("sizes-100003")
    row = scores[0]
    assert 1500 < int((row == row[orders[0][4095]]).sum()) < 2500
    assert row[orders[0][4095]] == row[orders[0][4096]]


def test_the_reference_is_the_descending_order_of_the_64_bit_key():
    for g in TC.GROUPS:
        scores, _, orders = TC.group(g)
        for row, order in zip(scores, orders):
            key = TC.key64(row)
            assert len(np.unique(key)) == len(key)
            assert (np.argsort(key)[::-1] == order).all(), g


def test_reference_shape_sentinels_and_threshold():
    scores, runs, orders = TC.group("threshold")
    (k, above), (_, at), (_, over), (_, below) = runs
    hits, hsc, cnt = TC.ref_top(scores, k, above, orders)
    assert cnt.tolist() == [0] and (hits == TC.HIT_NONE).all() and (hsc == TC.INT32_MIN).all()
    assert TC.ref_top(scores, k, at, orders)[2].tolist() == [k]
    inside = int(TC.ref_top(scores, k, over, orders)[2][0])
    assert 0 < inside < k
    assert TC.ref_top(scores, k, below, orders)[2].tolist() == [k]
    hits, hsc, cnt = TC.ref_top(np.array([3, 9, 9], np.int32), 5)
    assert hits.tolist() == [[1, 2, 0] + [int(TC.HIT_NONE)] * 2] and cnt.tolist() == [3]
    assert hsc.tolist() == [[9, 9, 3, TC.INT32_MIN, TC.INT32_MIN]]
    assert TC.mutant_top(np.array([3, 9, 9], np.int32), 2)[0].tolist() == [[2, 1]]


def test_every_case_is_callable():
    names = [c[0] for c in TC.cases()]
    assert len(names) == len(set(names)) > 100
    for name, scores, k, ms in TC.cases():
        assert scores.dtype == np.int32 and scores.ndim == 2 and 1 <= k <= TC.TOP_MAX_K, name
    assert {n for n in TC.SIZES} == {int(g.split("-")[1]) for g in TC.GROUPS if g.startswith("sizes")}


def test_golden_best_scores_list():
    """The 12 best of the ssearch36 scores of query100 x data500; the first two are the "The best
    scores are:" list of the reference's alignments500.txt (tests/golden/alignments500.tsv), the
    runs of 69, 67 and 64 are in library order."""
    names, scores = TC.golden_scores(os.path.join(O.GOLDEN, "score500_R_lines.txt"))
    hits, hsc, cnt = TC.ref_top(scores, 12)
    assert cnt.tolist() == [12]
    assert [(names[int(h)], int(s)) for h, s in zip(hits[0], hsc[0])] == TC.GOLDEN_TOP12
    rows = [ln.split("\t") for ln in open(os.path.join(O.GOLDEN, "alignments500.tsv"))][1:]
    assert [(r[0], int(r[1])) for r in rows] == TC.GOLDEN_TOP12[:2]
    for a, b in zip(hits[0], hits[0][1:]):
        assert scores[a] > scores[b] or a < b
    assert (TC.mutant_top(scores, 12)[0] != hits).any()
