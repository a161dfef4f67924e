"""Statistics of the frameshift-tolerant translated search on the GPU (include/swbank.h
"statistics of frameshift hits") against the reference pipeline of
tests/fshift_stats_cases.py (stat_cases.shuffle -> fshift_cases.c_search_set ->
stat_cases.histogram -> stat_cases.fit; its shared inputs are checked for a real fit by
tests/test_fshift_stats_cases.py): the public chain shuffle -> score_frameshift -> histogram and the
estimate's counters exactly, lambda and K within the tolerances of tests/test_gpu_stats.py (lambda
relative 1e-9, K relative 1e-6: the histograms are equal, so only the solver's stop separates the
two fits), slices, the host form, a two-child bank, what the call must leave alone, timing, the
chain into top hits and significance on one stream, and the refusals in the header's order."""
import ctypes

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fshift_stats_cases as FSS
import stat_cases as SC

pytestmark = pytest.mark.gpu

FILL = 0x3C
LAMBDA_RTOL, K_RTOL, SIG_RTOL = 1e-9, 1e-6, 1e-10


def _torch():
    import torch
    return torch


def _to_dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _filled(nbytes):
    torch = _torch()
    return torch.full((max(nbytes, 1),), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def _zeros64(n):
    torch = _torch()
    return torch.zeros((max(n, 1),), dtype=torch.int64, device=torch.device("cuda", 0))


class Batch:
    """A packed DNA batch on the device."""

    def __init__(self, res, offs, lens):
        self.res, self.offs, self.lens = res, offs, lens
        self.n, self.max_len = len(lens), int(lens.max())
        self.d_res, self.d_offs, self.d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)

    def ptrs(self):
        return self.d_res.data_ptr(), self.d_offs.data_ptr(), self.d_lens.data_ptr()


def _bank(which=None, **kw):
    bank = S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH, **kw)
    bank.set_matrix(O.BLOSUM62, *F.PEN)
    if which:
        qs = FSS.queries(which)
        bank.load_query(qs[0]) if len(qs) == 1 else bank.load_queries(qs)
    return bank


def _live():
    f = S.lib().swbank_live_buffers
    f.restype = ctypes.c_long
    f.argtypes = []
    return int(f())


def _fields(st):
    return (st.lambda_, st.K, st.n_samples, st.n_clamped, st.query_len, st.flags, st.min_score,
            st.max_score)


def _check_against_reference(stats, which, seed, fs):
    want = FSS.fitted(which, seed, fs)
    assert len(stats) == len(want)
    for st, q, (lam, K, ns, lo, hi, clamped) in zip(stats, FSS.queries(which), want):
        assert (st.n_samples, st.min_score, st.max_score, st.n_clamped) == (ns, lo, hi, clamped)
        assert (st.query_len, st.flags) == (len(q), 0)
        assert abs(st.lambda_ - lam) <= LAMBDA_RTOL * lam, (st.lambda_, lam)
        assert abs(st.K - K) <= K_RTOL * K, (st.K, K)


# ---- 1. the public chain and the estimate against the reference ------------------------------------
def _chain_hist(bank, bt, nq, seed, fs, rounds):
    """The pooled histogram through the three public device calls."""
    torch = _torch()
    d_c, d_s, d_x = _zeros64(nq * SC.BINS), _zeros64(nq * SC.BINS), _zeros64(nq)
    d_shuf = _filled(len(bt.res))
    d_scores = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32,
                          device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    for r in range(rounds):
        bank.shuffle_batch_device(*bt.ptrs(), bt.n, bt.max_len, seed + r, d_shuf.data_ptr())
        bank.score_frameshift_device(d_shuf.data_ptr(), bt.d_offs.data_ptr(),
                                     bt.d_lens.data_ptr(), bt.n, bt.max_len, fs,
                                     d_scores.data_ptr())
        bank.score_histogram_device(d_scores.data_ptr(), bt.n, d_c.data_ptr(), nq=nq,
                                    d_lens=bt.d_lens.data_ptr(), d_len_sums=d_s.data_ptr(),
                                    d_clamped=d_x.data_ptr())
    bank.sync()
    return (d_c.cpu().numpy().view(np.uint64).reshape(nq, -1),
            d_s.cpu().numpy().view(np.uint64).reshape(nq, -1), d_x.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("fs", FSS.FS_VALUES)
@pytest.mark.parametrize("which", ["one", "set"])
def test_chain_and_estimate_match_the_reference(which, fs):
    bt = Batch(*FSS.batch())
    nq = len(FSS.queries(which))
    with _bank(which) as bank:
        for seed in FSS.SEEDS:
            want = FSS.reference(which, seed, fs)
            got = _chain_hist(bank, bt, nq, seed, fs, FSS.ROUNDS)
            for g, w, what in zip(got, want, ("counts", "length sums", "clamped")):
                assert np.array_equal(g, w), (seed, what)
            stats = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, fs,
                                                               seed=seed, rounds=FSS.ROUNDS)
            assert bank.last_kernel() == \
                f"fshift-stats rounds={FSS.ROUNDS} nq={nq} n={bt.n} slices=1"
            _check_against_reference(stats, which, seed, fs)
            # the fit is a function of the counters alone: the library's fit of the chain's
            # counters is the estimate's, bit for bit
            for i, st in enumerate(stats):
                fit = S.fit_statistics(got[0][i], got[1][i], st.query_len)
                assert (fit.lambda_, fit.K, fit.n_samples) == (st.lambda_, st.K, st.n_samples)


# ---- 2. slices -------------------------------------------------------------------------------------
def test_slices_return_the_same_structs(monkeypatch):
    """2,200 targets of at most 600 bases.  A slice takes 4 nq + 632 bytes per target (nq scores,
    the bases at a stride of 624 and an offset), so with a set of 96 short queries 1 MiB holds
    1,032 targets: three slices."""
    rng = np.random.default_rng(167)
    lens = rng.integers(0, 601, 2200).astype(np.uint32)
    lens[:2] = (600, 0)
    offs = np.zeros(len(lens), np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    res = rng.integers(0, 5, int(lens.sum()) + 1).astype(np.uint8)
    bt = Batch(res, offs, lens)
    qs = [rng.integers(0, 20, int(m)).astype(np.uint8) for m in rng.integers(3, 9, 96)]
    with _bank() as bank:
        bank.load_queries(qs)
        whole = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, -15,
                                                           seed=1, rounds=2)
        assert bank.last_kernel() == f"fshift-stats rounds=2 nq=96 n={bt.n} slices=1"
        monkeypatch.setenv("SWBANK_STAT_MB", "1")
        sliced = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, -15,
                                                            seed=1, rounds=2)
        slices = int(bank.last_kernel().rsplit("=", 1)[1])
        assert slices >= 3
        assert bank.last_kernel().startswith(f"fshift-stats rounds=2 nq=96 n={bt.n} ")
    assert len(whole) == len(sliced) == 96
    for a, b in zip(whole, sliced):
        assert bytes(a) == bytes(b)
    assert all(st.n_samples == 2 * int((lens > 0).sum()) for st in whole)
    assert not any(st.degenerate or st.clamped for st in whole)


# ---- 3. the host form, a two-child bank, what the call leaves alone, timing, leaks ----------------
def test_host_form_two_children_side_effects_and_timing():
    torch = _torch()
    res, offs, lens = FSS.batch()
    bt = Batch(res, offs, lens)
    fs, seed, nq = -15, 1, len(FSS.SET_LENS)
    base = _live()
    with _bank("set") as bank:
        # a search's own results, made before the estimate, are not touched by it
        d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=torch.device("cuda", 0))
        d_sd = _filled(nq * bt.n)
        torch.cuda.synchronize()
        bank.score_frameshift_device(*bt.ptrs(), bt.n, bt.max_len, fs, d_sc.data_ptr(),
                                     d_strands=d_sd.data_ptr())
        bank.sync()
        sc, sd = d_sc.cpu().numpy(), d_sd.cpu().numpy()
        dev = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, fs,
                                                         seed=seed, rounds=FSS.ROUNDS)
        _check_against_reference(dev, "set", seed, fs)
        assert np.array_equal(d_sd.cpu().numpy(), sd) and np.array_equal(d_sc.cpu().numpy(), sc)
        assert np.array_equal(bt.d_res.cpu().numpy(), res)
        with pytest.raises(S.SwbankError) as ei:  # no best hit is tracked
            bank.best()
        assert ei.value.status == S.ERR_STATE
        # the host form, from a packed batch and from a list of targets
        host = bank.estimate_frameshift_statistics((res, offs, lens), fs, seed=seed,
                                                   rounds=FSS.ROUNDS)
        assert bank.last_kernel() == f"fshift-stats rounds={FSS.ROUNDS} nq={nq} n={bt.n} slices=1"
        listed = bank.estimate_frameshift_statistics(FSS.targets_of(res, offs, lens), fs,
                                                     seed=seed, rounds=FSS.ROUNDS)
        for a, b, c in zip(dev, host, listed):
            assert bytes(a) == bytes(b) == bytes(c)
        # one timing bracket per pass: shuffle, score and histogram of every round
        bank.set_timing(True)
        bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, fs, seed=seed,
                                                   rounds=FSS.ROUNDS)
        launches, _, ms = bank.timing()
        assert launches == 3 * FSS.ROUNDS and ms > 0
        # a caller's stream
        stream = torch.cuda.Stream()
        again = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, fs,
                                                           seed=seed, rounds=FSS.ROUNDS,
                                                           stream=stream.cuda_stream)
        assert [bytes(a) for a in again] == [bytes(a) for a in dev]
    with _bank("set", devices=[0, 0]) as bank:  # a multi-device bank runs the call on its root
        two = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, fs,
                                                         seed=seed, rounds=FSS.ROUNDS)
        assert bank.last_kernel() == f"fshift-stats rounds={FSS.ROUNDS} nq={nq} n={bt.n} slices=1"
        two_host = bank.estimate_frameshift_statistics((res, offs, lens), fs, seed=seed,
                                                       rounds=FSS.ROUNDS)
    for a, b, c in zip(dev, two, two_host):
        assert bytes(a) == bytes(b) == bytes(c)
    assert _live() == base  # the live-buffer count returns to its baseline


# ---- 4. score -> top hits -> significance on one stream ----------------------------------------------
def test_chain_into_top_hits_and_significance_on_one_stream():
    torch = _torch()
    res, offs, lens = FSS.batch()
    bt = Batch(res, offs, lens)
    nq, k, fs, dev = len(FSS.SET_LENS), 8, -15, torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    with _bank("set") as bank:
        stats = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, fs,
                                                           seed=1, rounds=FSS.ROUNDS)
        d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        d_hits, d_hsc = _filled(nq * k * 8), _filled(nq * k * 4)
        d_bits, d_ev = _filled(nq * k * 8), _filled(nq * k * 8)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_frameshift_device(*bt.ptrs(), bt.n, bt.max_len, fs, d_sc.data_ptr(), stream=h)
        bank.top_hits_device(d_sc.data_ptr(), bt.n, k, d_hits.data_ptr(), nq=nq,
                             d_hit_scores=d_hsc.data_ptr(), stream=h)
        bank.hit_significance_device(stats, d_hsc.data_ptr(), d_hits.data_ptr(),
                                     bt.d_lens.data_ptr(), k, bt.n, d_bits=d_bits.data_ptr(),
                                     d_evalues=d_ev.data_ptr(), stream=h)
        assert bank.last_kernel() == f"significance nq={nq} k={k}"
        bank.sync()
        stream.synchronize()
    pos = d_hits.cpu().numpy().view(np.uint64).reshape(nq, k).astype(np.int64)
    hsc = d_hsc.cpu().numpy().view(np.int32).reshape(nq, k)
    bits = d_bits.cpu().numpy().view(np.float64).reshape(nq, k)
    ev = d_ev.cpu().numpy().view(np.float64).reshape(nq, k)
    scores = d_sc.cpu().numpy().reshape(nq, bt.n)
    for i in range(nq):
        assert np.array_equal(hsc[i], scores[i][pos[i]]) and (np.diff(hsc[i]) <= 0).all()
        hb, he = S.hit_significance(stats[i], hsc[i], lens[pos[i]], bt.n)  # lengths in nucleotides
        assert np.allclose(bits[i], hb, rtol=SIG_RTOL, atol=0), i
        assert np.allclose(ev[i], he, rtol=SIG_RTOL, atol=0), i
        assert (np.diff(bits[i]) <= 0).all() and (ev[i] > 0).all()


# ---- 5. refusals -----------------------------------------------------------------------------------
def test_refusals_in_the_headers_order():
    res, offs, lens = FSS.batch()
    bt = Batch(res[:int(offs[8])], offs[:8], lens[:8])
    host = (bt.res, bt.offs, bt.lens)
    (q,) = FSS.queries("one")
    r, o, l = bt.ptrs()

    def status(fn, *a, **kw):
        with pytest.raises(S.SwbankError) as ei:
            fn(*a, **kw)
        return ei.value.status

    def both(bank, fs=-15, table=None, rounds=1):
        return {status(bank.estimate_frameshift_statistics_device, r, o, l, bt.n, bt.max_len, fs,
                       rounds=rounds, codon_table=table),
                status(bank.estimate_frameshift_statistics, host, fs, rounds=rounds,
                       codon_table=table)}

    bad_tab = F.standard_table()
    bad_tab[63] = 24
    rng = np.random.default_rng(173)
    long_q = rng.integers(0, 20, S.FSHIFT_MAX_QUERY + 1).astype(np.uint8)
    with S.ScoreBank() as bank:  # a DNA bank, whatever else is wrong
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(np.arange(20, dtype=np.uint8) % 4)
        assert both(bank, fs=1, table=bad_tab, rounds=0) == {S.ERR_UNSUPPORTED}
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_MERGED) as bank:  # merged gaps
        bank.set_matrix(O.BLOSUM62, *F.PEN)
        bank.load_query(q)
        assert both(bank, fs=1, table=bad_tab, rounds=0) == {S.ERR_UNSUPPORTED}
    with _bank() as bank:
        assert both(bank, fs=1) == {S.ERR_ARG}            # the range before the table,
        assert both(bank, table=bad_tab) == {S.ERR_ARG}   # the table before the state,
        assert both(bank, rounds=0) == {S.ERR_STATE}      # the state (no query) before the rest
        bank.load_query(long_q)
        assert both(bank, rounds=0) == {S.ERR_UNSUPPORTED}  # 1,025 rows, before the arguments
        bank.load_queries([q, long_q])
        assert both(bank) == {S.ERR_UNSUPPORTED}            # any query of the set
        bank.load_query(q)
        assert both(bank, fs=-32768) == {S.ERR_ARG}
        assert both(bank, rounds=0) == {S.ERR_ARG}
        for a in ((0, o, l, bt.n), (r, 0, l, bt.n), (r, o, 0, bt.n), (r, o, l, 0),
                  (r, o, l, 1 << 32)):
            assert status(bank.estimate_frameshift_statistics_device, *a, bt.max_len, -15) == \
                S.ERR_ARG
        L = S.lib()
        assert L.sw_estimate_fshift_statistics_device(bank._h, r, o, l, bt.n, bt.max_len, None, -15,
                                                      1, 1, None, None) == S.ERR_ARG  # no out
        st1 = S.Statistics()
        assert L.sw_estimate_fshift_statistics_device(None, r, o, l, bt.n, bt.max_len, None, -15,
                                                      1, 1, ctypes.byref(st1), None) == S.ERR_ARG
        bad = bt.res.copy()
        bad[int(bt.offs[5]) + 1] = 5  # a host code of 5 or more
        assert status(bank.estimate_frameshift_statistics, (bad, bt.offs, bt.lens), -15) == S.ERR_ARG
        outside = bt.lens.copy()
        outside[7] += len(bt.res)  # a target outside the buffer
        assert status(bank.estimate_frameshift_statistics, (bt.res, bt.offs, outside), -15) == \
            S.ERR_ARG
        # the ends of the range are fine, and a refusal leaves the bank usable
        for fs in (0, -32767):
            (st,) = bank.estimate_frameshift_statistics(host, fs, seed=3)
            assert st.n_samples == int((bt.lens > 0).sum()) and st.query_len == len(q)
