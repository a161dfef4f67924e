"""The reference pipeline of the frameshift search's statistics (tests/fshift_stats_cases.py) on the
CPU: it does not depend on how the batch is sliced, at fs = -32767 its scores are the merged
six-frame scores of the same shuffles, and the shared inputs give a fit that is not degenerate --
asserted here, for the reference alone, so that no GPU test can pass on a degenerate fit.  And,
without a device, the two new entries are exported and refuse a NULL bank."""
import ctypes
import subprocess

import numpy as np
import pytest

import swbank as S

import fshift_cases as FS
import fshift_stats_cases as FSS
import stat_cases as SC


def test_reference_is_invariant_under_slicing():
    res, offs, lens = FSS.batch()
    qs = FSS.queries("one")
    whole = FSS.round_scores("one", 1, -15)
    cuts = (0, 1, 63, 64, 137, len(lens))
    parts = [FSS.shuffled_scores(qs, res, offs[a:b], lens[a:b], 1, -15, first=a)
             for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    got = FSS.pool(parts[:1], lens[:1], 1)
    for a, b, p in list(zip(cuts[:-1], cuts[1:], parts))[1:]:
        got = tuple(x + y for x, y in zip(got, FSS.pool([p], lens[a:b], 1)))
    want = FSS.pool([whole], lens, 1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # the key is the batch position: the same slice at another position is another shuffle
    assert not np.array_equal(FSS.shuffled_scores(qs, res, offs[64:137], lens[64:137], 1, -15),
                              parts[3])


@pytest.mark.parametrize("which", ["one", "set"])
def test_anchor_equals_six_frames_of_the_same_shuffles(which):
    res, offs, lens = FSS.batch()
    shuf = SC.shuffle(res, offs, lens, 2)
    seqs = FSS.targets_of(shuf, offs, lens)
    got = FSS.round_scores(which, 2, -32767)
    for i, q in enumerate(FSS.queries(which)):
        want, _ = FS.six_frames(q, seqs)
        assert np.array_equal(got[i], want), i
    # a shift that can win lowers no score of the same shuffles, and among shuffled targets it
    # raises some only where the query is long enough to pay for it
    assert (FSS.round_scores(which, 2, -15) >= got).all()
    if which == "set":
        assert (FSS.round_scores(which, 2, -15) > got).any()


@pytest.mark.parametrize("fs", FSS.FS_VALUES)
@pytest.mark.parametrize("which", ["one", "set"])
def test_shared_inputs_give_a_real_fit(which, fs):
    _, _, lens = FSS.batch()
    for seed in FSS.SEEDS:
        counts, sums, clamped = FSS.reference(which, seed, fs)
        assert not clamped.any()
        for i, q in enumerate(FSS.queries(which)):
            assert np.count_nonzero(counts[i]) >= 2, (seed, i)
            assert int(counts[i].sum()) == FSS.ROUNDS * int((lens > 0).sum())
            assert int(sums[i].sum()) == FSS.ROUNDS * int(lens.sum())
            lam, K, degenerate = SC.fit(counts[i], sums[i], len(q))
            assert not degenerate and lam > 0 and K > 0
    # two seeds share one round (seed + 1 of the first is seed of the second) and differ
    a, b = FSS.reference(which, 1, fs), FSS.reference(which, 2, fs)
    assert not np.array_equal(a[0], b[0])


def test_entries_are_exported_and_refuse_a_null_bank():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"sw_estimate_fshift_statistics", "sw_estimate_fshift_statistics_device"} <= syms
    L = S.lib()
    st = S.Statistics()
    res, offs, lens = FSS.batch()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.sw_estimate_fshift_statistics(None, p(res), res.size, p(offs), p(lens), len(lens),
                                           None, -15, 1, 1, ctypes.byref(st)) == S.ERR_ARG
    assert L.sw_estimate_fshift_statistics_device(None, p(res), p(offs), p(lens), len(lens), 400,
                                                  None, -15, 1, 1, ctypes.byref(st),
                                                  None) == S.ERR_ARG
    assert (st.lambda_, st.K, st.n_samples) == (0.0, 0.0, 0)
