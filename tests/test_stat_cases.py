"""Hit statistics on the host (no GPU): sw_hit_significance against the figures ssearch36
printed for the reference's own search (tests/golden/statistics500.tsv), sw_fit_statistics
against the numpy fit of tests/stat_cases.py on histograms of oracle scores of reference
shuffles, the reference's Lambda and K inside the spread of the single-round estimates, and the
inputs' power to tell the shuffle and the fit from their near misses.

Tolerances: the solver stops at a relative change of 1e-13, so lambda agrees to 1e-9 with room;
dK/K <= s_max dlambda with s_max <= 4095, so K agrees to 1e-6."""
import ctypes

import numpy as np
import pytest

import swbank as S

import stat_cases as SC

LAMBDA_RTOL, K_RTOL = 1e-9, 1e-6


def _close(st, lam, K):
    assert not st.degenerate
    assert abs(st.lambda_ - lam) <= LAMBDA_RTOL * lam, (st.lambda_, lam)
    assert abs(st.K - K) <= K_RTOL * K, (st.K, K)


# ---- sw_hit_significance against the reference ------------------------------------------------
def test_hit_significance_reproduces_the_printed_bits_and_evalues():
    lam, K, db, qlen, hits = SC.golden_stats()
    st = S.make_statistics(lam, K, qlen)
    bits, ev = S.hit_significance(st, [h[2] for h in hits], [h[1] for h in hits], db)
    assert [h[0] for h in hits] == ["db211", "db428"]
    assert ["%.1f" % b for b in bits] == [h[3] for h in hits] == ["23.7", "22.1"]
    assert ["%.2g" % e for e in ev] == [h[4] for h in hits] == ["0.62", "1.9"]


def test_hit_significance_formulas_and_errors():
    st = S.make_statistics(0.25, 0.05, 77)
    sc = np.array([0, 1, 50, 4095, -3], np.int32)
    tl = np.array([1, 128, 300, 65536, 9], np.uint32)
    bits, ev = S.hit_significance(st, sc, tl, 12345)
    want_bits = (0.25 * sc - np.log(0.05)) / np.log(2.0)
    want_ev = 12345 * 0.05 * 77 * tl.astype(np.float64) * np.exp(-0.25 * sc.astype(np.float64))
    assert np.allclose(bits, want_bits, rtol=1e-13, atol=0)
    assert np.allclose(ev, want_ev, rtol=1e-13, atol=0)
    L = S.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(5)
    # either output alone; neither is an error; so are NULL inputs and degenerate statistics
    assert L.sw_hit_significance(ctypes.byref(st), p(sc), p(tl), 5, 9, p(out), None) == S.OK
    assert L.sw_hit_significance(ctypes.byref(st), p(sc), p(tl), 5, 9, None, p(out)) == S.OK
    assert L.sw_hit_significance(ctypes.byref(st), p(sc), p(tl), 5, 9, None, None) == S.ERR_ARG
    assert L.sw_hit_significance(None, p(sc), p(tl), 5, 9, p(out), None) == S.ERR_ARG
    assert L.sw_hit_significance(ctypes.byref(st), None, p(tl), 5, 9, p(out), None) == S.ERR_ARG
    assert L.sw_hit_significance(ctypes.byref(st), p(sc), None, 5, 9, p(out), None) == S.ERR_ARG
    for bad in (S.make_statistics(0.0, 0.1, 10), S.make_statistics(0.2, 0.0, 10),
                S.Statistics(lambda_=0.2, K=0.1, query_len=10, flags=S.STAT_DEGENERATE)):
        with pytest.raises(S.SwbankError) as e:
            S.hit_significance(bad, sc, tl, 9)
        assert e.value.status == S.ERR_ARG


# ---- sw_fit_statistics against stat_cases.fit --------------------------------------------------
@pytest.mark.parametrize("seed", range(1, 41))
def test_fit_single_rounds(seed):
    counts, sums = SC.golden_hist(seed)
    qlen = len(SC.golden()[0])
    st = S.fit_statistics(counts, sums, qlen)
    _close(st, *SC.fit(counts, sums, qlen)[:2])
    occ = np.nonzero(counts)[0]
    assert (st.n_samples, st.min_score, st.max_score) == (int(counts.sum()), occ[0], occ[-1])
    assert st.query_len == qlen and st.flags == 0 and st.n_clamped == 0


def test_fit_pooled_rounds():
    counts, sums = SC.golden_hist(100, 8)
    qlen = len(SC.golden()[0])
    lam, K, _ = SC.fit(counts, sums, qlen)
    _close(S.fit_statistics(counts, sums, qlen), lam, K)
    # the figures of the pooled estimate (4 digits)
    assert (round(lam, 4), round(K, 4)) == (0.1788, 0.0977)
    assert int(counts.sum()) == 8 * len(SC.golden()[3])


def test_fit_ragged_batch():
    counts, sums = SC.ragged_hist()
    qlen = len(SC.ragged()[0])
    _close(S.fit_statistics(counts, sums, qlen), *SC.fit(counts, sums, qlen)[:2])


def test_fit_two_bins_one_bin_and_empty():
    z = np.zeros(SC.BINS, np.uint64)
    two_c, two_s = z.copy(), z.copy()
    two_c[[10, 4095]] = 7, 2
    two_s[[10, 4095]] = 7 * 100, 2 * 300
    _close(S.fit_statistics(two_c, two_s, 50), *SC.fit(two_c, two_s, 50)[:2])
    adj_c, adj_s = z.copy(), z.copy()  # adjacent bins at the low end, a large lambda
    adj_c[[0, 1]] = 1000, 1
    adj_s[[0, 1]] = 1000 * 64, 64
    _close(S.fit_statistics(adj_c, adj_s, 33), *SC.fit(adj_c, adj_s, 33)[:2])
    one_c, one_s = z.copy(), z.copy()
    one_c[17], one_s[17] = 5, 640
    for c, s, n, lo, hi in ((one_c, one_s, 5, 17, 17), (z, z, 0, 0, 0)):
        st = S.fit_statistics(c, s, 50)
        assert st.degenerate and st.flags == S.STAT_DEGENERATE
        assert (st.lambda_, st.K, st.n_samples, st.min_score, st.max_score) == (0.0, 0.0, n, lo, hi)
        assert SC.fit(c, s, 50)[2]
    assert S.fit_statistics(two_c, two_s, 0).degenerate  # an empty query
    L = S.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = S.Statistics()
    assert L.sw_fit_statistics(None, p(two_s), 5, ctypes.byref(st)) == S.ERR_ARG
    assert L.sw_fit_statistics(p(two_c), None, 5, ctypes.byref(st)) == S.ERR_ARG
    assert L.sw_fit_statistics(p(two_c), p(two_s), 5, None) == S.ERR_ARG
    with pytest.raises(ValueError):
        S.fit_statistics(two_c[:100], two_s[:100], 5)


# ---- the reference's Lambda and K against the model ----------------------------------------------
def test_reference_lambda_and_K_lie_inside_the_single_round_spread():
    """A condition on the model, not a tolerance: ssearch36 fitted one shuffle of the same 499
    sequences, so its Lambda and K must be values the 40 single-round estimates reach."""
    lam, K, _, qlen, _ = SC.golden_stats()
    est = [SC.fit(*SC.golden_hist(seed), qlen)[:2] for seed in range(1, 41)]
    lams, Ks = [e[0] for e in est], [e[1] for e in est]
    assert min(lams) <= lam <= max(lams), (min(lams), lam, max(lams))
    assert min(Ks) <= K <= max(Ks), (min(Ks), K, max(Ks))


# ---- the inputs discriminate ---------------------------------------------------------------------
def test_inputs_tell_the_shuffle_from_sattolo_and_the_fit_from_an_unweighted_one():
    _, res, offs, lens = SC.golden()
    a = SC.shuffle(res, offs, lens, 1)
    b = SC.shuffle(res, offs, lens, 1, sattolo=True)
    differ = sum(not np.array_equal(a[o:o + l], b[o:o + l])
                 for o, l in zip(offs.astype(np.int64), lens.astype(np.int64)))
    assert differ == len(lens)  # every target of the batch tells them apart
    # a permutation of each target, nothing outside the targets touched, seeds differ
    for o, l in zip(offs.astype(np.int64)[:50], lens.astype(np.int64)[:50]):
        assert np.array_equal(np.sort(a[o:o + l]), np.sort(res[o:o + l]))
    assert not np.array_equal(a, SC.shuffle(res, offs, lens, 2))
    assert np.array_equal(a, SC.shuffle(res, offs, lens, 1))
    # slicing: a target's shuffle depends on its batch position alone
    k0 = 100
    part = SC.shuffle(res, offs[k0:], lens[k0:], 1, first=k0)
    o0 = int(offs[k0])
    assert np.array_equal(part[o0:], a[o0:])
    # the ragged batch: dropping the length weights moves K far outside the tolerance
    counts, sums = SC.ragged_hist()
    qlen = len(SC.ragged()[0])
    lam, K, _ = SC.fit(counts, sums, qlen)
    lam_u, K_u, _ = SC.fit(counts, sums, qlen, weights=False)
    assert abs(lam_u - lam) > 1e3 * LAMBDA_RTOL * lam or abs(K_u - K) > 1e3 * K_RTOL * K
    st = S.fit_statistics(counts, sums, qlen)
    assert abs(st.K - K_u) > 1e3 * K_RTOL * K
