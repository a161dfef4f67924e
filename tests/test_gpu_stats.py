"""Hit statistics on the GPU (include/swbank.h "hit significance"): the seeded shuffle byte for
byte against tests/stat_cases.py, the score / length histogram against numpy.bincount, the
estimate (shuffle -> score -> histogram -> fit) against the oracle's scores of reference
shuffles, bits and E-values of a top-hits list against the figures ssearch36 printed, the CLI,
and the argument and state errors.  Every test runs with plain and with poisoned device
buffers; the CPU references are computed once (stat_cases) and shared.

Tolerances (as tests/test_stat_cases.py): lambda relative 1e-9, K relative 1e-6 -- the
histograms are compared exactly, so only the solver's stop at 1e-13 and dK/K <= s_max dlambda
separate the two fits; bits and E against numpy in double at relative 1e-10, three orders above
the rounding of exp at these arguments."""
import ctypes
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import stat_cases as SC

pytestmark = pytest.mark.gpu

FILL = 0x3C
LAMBDA_RTOL, K_RTOL, SIG_RTOL = 1e-9, 1e-6, 1e-10
# the shuffle's tiers: a lane's LDS row holds 260 bytes, a wave's LDS 64 x 260
LENS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4099]
TIER_LENS = [260, 261, 16640, 16641]


@pytest.fixture(params=["plain", "poisoned"], autouse=True)
def buffers(request):
    if request.param == "poisoned":
        request.getfixturevalue("poisoned_buffers")


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


def _close(st, lam, K):
    assert not st.degenerate
    assert abs(st.lambda_ - lam) <= LAMBDA_RTOL * lam, (st.lambda_, lam)
    assert abs(st.K - K) <= K_RTOL * K, (st.K, K)


# ---- 1. the shuffle -------------------------------------------------------------------------------
def _gapped_batch(n, alpha, lens_pool):
    """n targets whose lengths walk through lens_pool, at odd byte offsets with gaps between
    them: (residues, offsets, lengths, the mask of the targets' bytes)."""
    rng = np.random.default_rng([n, alpha])
    lens = np.array([lens_pool[(7 * k + 3) % len(lens_pool)] for k in range(n)], np.uint32)
    gaps = 2 * rng.integers(0, 4, n) + 1 + (lens.astype(np.int64) % 2)  # every start is odd
    offs = np.zeros(n, np.int64)
    pos = 0
    for k in range(n):
        pos += int(gaps[k])
        pos += (pos + 1) % 2
        offs[k] = pos
        pos += int(lens[k])
    res = rng.integers(0, alpha, pos + 5).astype(np.uint8)
    mask = np.zeros(len(res), bool)
    for k in range(n):
        mask[offs[k]:offs[k] + int(lens[k])] = True
    assert (offs % 2 == 1).all()
    return res, offs.astype(np.uint64), lens, mask


@pytest.mark.parametrize("alpha", [5, 24], ids=["dna", "protein"])
@pytest.mark.parametrize("n", [1, 63, 65, 8193])
def test_shuffle_matches_the_reference_byte_for_byte(n, alpha):
    torch = _torch()
    pool = LENS + TIER_LENS if n == 65 else LENS
    res, offs, lens, mask = _gapped_batch(n, alpha, pool)
    d_res, d_offs, d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)
    seeds = (11, 0xFFFFFFFFFFFFFFF5)
    outs = []
    with S.ScoreBank() as bank:  # neither penalties nor a query: the call needs none
        for seed in seeds + seeds[:1]:
            d_out = _filled(len(res))
            torch.cuda.synchronize()
            bank.shuffle_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n,
                                      int(lens.max()), seed, d_out.data_ptr())
            assert bank.last_kernel() == f"shuffle n={n}"
            bank.sync()
            outs.append(d_out.cpu().numpy())
    for seed, got in zip(seeds, outs):
        want = np.where(mask, SC.shuffle(res, offs, lens, seed), FILL).astype(np.uint8)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (seed, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(outs[0], outs[2])          # the same seed twice
    if lens.max() > 3:
        assert not np.array_equal(outs[0], outs[1])  # two seeds
    assert np.array_equal(d_res.cpu().numpy(), res)  # the input is left alone


# ---- 2. the histogram -----------------------------------------------------------------------------
SPECIAL = np.array([-5, 0, 4094, 4095, 4096, np.iinfo(np.int32).max, np.iinfo(np.int32).min],
                   np.int64)


def _hist_case(nq, n):
    rng = np.random.default_rng([nq, n])
    scores = rng.integers(18, 70, (nq, n))
    where = rng.random((nq, n)) < 0.02
    scores[where] = SPECIAL[rng.integers(0, len(SPECIAL), int(where.sum()))]
    scores[nq - 1, :] = 33  # an all-equal row
    if n >= len(SPECIAL):   # every special value at least once, in row 0
        scores[0, rng.permutation(n)[:len(SPECIAL)]] = SPECIAL
    lens = rng.integers(0, 300, n).astype(np.uint32)  # zero lengths among them
    lens[::5] = 0xFFFFFFF0  # a workgroup's sum of these leaves 32 bits
    return scores.astype(np.int32), lens


def _want_hist(scores, lens):
    rows = [SC.histogram(r, lens) for r in scores]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows], np.uint64))


@pytest.mark.parametrize("nq", [1, 3, 17])
def test_histogram_matches_bincount(nq):
    torch = _torch()
    with S.ScoreBank() as bank:
        for n in (1, 63, 64, 65, 8191, 8193, 70001):
            scores, lens = _hist_case(nq, n)
            pad = (nq + n) % 4  # rows at every 4-byte phase (n odd moves them row by row too)
            t = _to_dev(np.concatenate([np.full(pad, 0x3C3C3C3C, np.int32), scores.reshape(-1)]))
            d_scores, d_lens = t.data_ptr() + 4 * pad, _to_dev(lens)
            want_c, want_s, want_x = _want_hist(scores, lens)
            d_c, d_s, d_x = _zeros64(nq * SC.BINS), _zeros64(nq * SC.BINS), _zeros64(nq)
            torch.cuda.synchronize()
            for rep in (1, 2):  # the call accumulates
                bank.score_histogram_device(d_scores, n, d_c.data_ptr(), nq=nq,
                                            d_lens=d_lens.data_ptr(), d_len_sums=d_s.data_ptr(),
                                            d_clamped=d_x.data_ptr())
                assert bank.last_kernel() == f"stat-hist nq={nq} n={n}"
                bank.sync()
                got = [x.cpu().numpy().view(np.uint64) for x in (d_c, d_s, d_x)]
                assert np.array_equal(got[0].reshape(nq, -1), rep * want_c), (n, rep)
                assert np.array_equal(got[1].reshape(nq, -1), rep * want_s), (n, rep)
                assert np.array_equal(got[2], rep * want_x), (n, rep)
            # without lengths nothing is skipped and nothing summed; without d_clamped
            plain_c, _, plain_x = _want_hist(scores, None)
            for with_clamped in (True, False):
                d_c, d_x = _zeros64(nq * SC.BINS), _zeros64(nq)
                torch.cuda.synchronize()
                bank.score_histogram_device(d_scores, n, d_c.data_ptr(), nq=nq,
                                            d_clamped=d_x.data_ptr() if with_clamped else 0)
                bank.sync()
                assert np.array_equal(d_c.cpu().numpy().view(np.uint64).reshape(nq, -1), plain_c)
                assert np.array_equal(d_x.cpu().numpy().view(np.uint64),
                                      plain_x if with_clamped else np.zeros(nq, np.uint64))
            # lengths without sums: the zero lengths are still skipped
            d_c = _zeros64(nq * SC.BINS)
            torch.cuda.synchronize()
            bank.score_histogram_device(d_scores, n, d_c.data_ptr(), nq=nq,
                                        d_lens=d_lens.data_ptr())
            bank.sync()
            assert np.array_equal(d_c.cpu().numpy().view(np.uint64).reshape(nq, -1), want_c)


# ---- 3. the estimate ------------------------------------------------------------------------------
class Batch:
    """A host batch on the device."""

    def __init__(self, res, offs, lens):
        self.res, self.offs, self.lens = res, offs, lens
        self.n, self.max_len, self.min_len = len(lens), int(lens.max()), int(lens.min())
        self.d_res, self.d_offs, self.d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)

    def ptrs(self):
        return self.d_res.data_ptr(), self.d_offs.data_ptr(), self.d_lens.data_ptr()


def _chain_hist(bank, bt, seed, nq=1, rounds=1):
    """The pooled histogram through the three device calls: shuffle, score, histogram."""
    torch = _torch()
    d_c, d_s, d_x = _zeros64(nq * SC.BINS), _zeros64(nq * SC.BINS), _zeros64(nq)
    d_shuf = _filled(len(bt.res))
    d_scores = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32,
                          device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    for r in range(rounds):
        bank.shuffle_batch_device(*bt.ptrs(), bt.n, bt.max_len, seed + r, d_shuf.data_ptr())
        bank.score_batch_device(d_shuf.data_ptr(), bt.d_offs.data_ptr(), bt.d_lens.data_ptr(),
                                bt.n, bt.max_len, d_scores.data_ptr())
        bank.score_histogram_device(d_scores.data_ptr(), bt.n, d_c.data_ptr(), nq=nq,
                                    d_lens=bt.d_lens.data_ptr(), d_len_sums=d_s.data_ptr(),
                                    d_clamped=d_x.data_ptr())
    bank.sync()
    return (d_c.cpu().numpy().view(np.uint64).reshape(nq, -1),
            d_s.cpu().numpy().view(np.uint64).reshape(nq, -1), d_x.cpu().numpy().view(np.uint64))


def test_estimate_golden_seeds():
    q, res, offs, lens = SC.golden()
    bt = Batch(res, offs, lens)
    with S.ScoreBank() as bank:
        bank.set_penalties(*SC.REF)
        bank.load_query(q)
        for seed in range(1, 41):
            want_c, want_s = SC.golden_hist(seed)
            got_c, got_s, got_x = _chain_hist(bank, bt, seed)
            assert np.array_equal(got_c[0], want_c) and np.array_equal(got_s[0], want_s), seed
            assert got_x[0] == 0
            (st,) = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=seed,
                                                    min_len=bt.min_len)
            assert bank.last_kernel() == f"stats rounds=1 nq=1 n={bt.n} slices=1"
            _close(st, *SC.fit(want_c, want_s, len(q))[:2])
            occ = np.nonzero(want_c)[0]
            assert (st.n_samples, st.n_clamped, st.query_len, st.flags, st.min_score,
                    st.max_score) == (bt.n, 0, len(q), 0, occ[0], occ[-1])
        # rounds pool their counts; the host entry uploads the batch and does the same
        want_c, want_s = SC.golden_hist(100, 8)
        lam, K, _ = SC.fit(want_c, want_s, len(q))
        (st,) = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=100, rounds=8)
        assert bank.last_kernel() == f"stats rounds=8 nq=1 n={bt.n} slices=1"
        _close(st, lam, K)
        assert st.n_samples == 8 * bt.n
        (host,) = bank.estimate_statistics(res, offs, lens, seed=100, rounds=8)
        assert (host.lambda_, host.K, host.n_samples) == (st.lambda_, st.K, st.n_samples)


def _set_queries():
    q = SC.golden()[0]
    return [q, q[20:90].copy(), np.random.default_rng(12).integers(0, 4, 130).astype(np.uint8)]


def _set_hists(seed):
    """The CPU histograms of a query set of 3 against one reference shuffle of data500."""
    _, res, offs, lens = SC.golden()
    shuf = SC.shuffle(res, offs, lens, seed)
    return [SC.histogram(O.score_batch(q, shuf, offs, lens, O.dna_matrix(), SC.REF[2], SC.REF[3],
                                       O.GAP_MERGED), lens)[:2] for q in _set_queries()]


def test_estimate_query_set():
    _, res, offs, lens = SC.golden()
    bt = Batch(res, offs, lens)
    queries = _set_queries()
    want = _set_hists(7)
    with S.ScoreBank() as bank:
        bank.set_penalties(*SC.REF)
        bank.load_queries(queries)
        got_c, got_s, _ = _chain_hist(bank, bt, 7, nq=3)
        stats = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=7)
        assert bank.last_kernel() == f"stats rounds=1 nq=3 n={bt.n} slices=1"
        assert len(stats) == 3
        for i, (q, (wc, ws)) in enumerate(zip(queries, want)):
            assert np.array_equal(got_c[i], wc) and np.array_equal(got_s[i], ws), i
            _close(stats[i], *SC.fit(wc, ws, len(q))[:2])
            assert stats[i].query_len == len(q) and stats[i].n_samples == bt.n


@pytest.fixture(scope="module")
def big_ragged():
    """24,000 targets of 64 .. 150 codes: 4.5 MB of estimate scratch, 5 slices at 1 MiB."""
    rng = np.random.default_rng(77)
    lens = rng.integers(64, 151, 24000).astype(np.uint32)
    offs = np.zeros(len(lens), np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    res = O.random_codes(78, int(lens.sum()), 4)
    return res, offs, lens


def test_estimate_slices_give_identical_counters(big_ragged, monkeypatch):
    bt = Batch(*big_ragged)
    q = O.random_codes(79, 100, 4)
    with S.ScoreBank() as bank:
        bank.set_penalties(*SC.REF)
        bank.load_query(q)
        c, s, _ = _chain_hist(bank, bt, 3, rounds=2)
        want = S.fit_statistics(c[0], s[0], len(q))
        (whole,) = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=3, rounds=2,
                                                   min_len=bt.min_len)
        assert bank.last_kernel() == f"stats rounds=2 nq=1 n={bt.n} slices=1"
        monkeypatch.setenv("SWBANK_STAT_MB", "1")
        (sliced,) = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=3, rounds=2,
                                                    min_len=bt.min_len)
        slices = int(bank.last_kernel().rsplit("=", 1)[1])
        assert slices >= 3 and bank.last_kernel().startswith(f"stats rounds=2 nq=1 n={bt.n} ")
    # the fit is a function of the counters alone: identical counters, identical doubles
    for st in (whole, sliced):
        assert (st.lambda_, st.K, st.n_samples, st.min_score, st.max_score, st.flags) == \
            (want.lambda_, want.K, 2 * bt.n, want.min_score, want.max_score, 0)


def test_estimate_protein_gotoh_device_and_host():
    rng = np.random.default_rng(5)
    seqs = [O.random_codes(900 + i, int(l), 20) for i, l in enumerate(rng.integers(200, 301, 64))]
    res, offs, lens = O.pack_residues(seqs)
    q = O.random_codes(899, 180, 20)
    counts, sums = np.zeros(SC.BINS, np.uint64), np.zeros(SC.BINS, np.uint64)
    for r in range(3):
        sc = O.score_batch(q, SC.shuffle(res, offs, lens, 21 + r), offs, lens, O.BLOSUM62, -11, -1,
                           O.GAP_GOTOH)
        c, s, _ = SC.histogram(sc, lens)
        counts += c
        sums += s
    lam, K, _ = SC.fit(counts, sums, len(q))
    bt = Batch(res, offs, lens)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=S.GAP_GOTOH) as bank:
        bank.set_matrix(O.BLOSUM62, -11, -1)
        bank.load_query(q)
        (dev,) = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=21, rounds=3)
        (host,) = bank.estimate_statistics(res, offs, lens, seed=21, rounds=3)
    for st in (dev, host):
        _close(st, lam, K)
        assert st.n_samples == 3 * 64 and st.query_len == len(q)
    assert (dev.lambda_, dev.K) == (host.lambda_, host.K)


def test_estimate_multi_device_bank():
    q, res, offs, lens = SC.golden()
    bt = Batch(res, offs, lens)
    want_c, want_s = SC.golden_hist(3)
    with S.ScoreBank(devices=[0, 0]) as bank:
        bank.set_penalties(*SC.REF)
        bank.load_query(q)
        (st,) = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=3)
        assert bank.last_kernel() == f"stats rounds=1 nq=1 n={bt.n} slices=1"
        _close(st, *SC.fit(want_c, want_s, len(q))[:2])
        (host,) = bank.estimate_statistics(res, offs, lens, seed=3)
        assert (host.lambda_, host.K, host.n_samples) == (st.lambda_, st.K, bt.n)


def test_estimate_clamped_and_degenerate():
    """Targets of 1200 equal codes score 6000 against themselves, past the histogram's last bin:
    they are clamped and counted; one bin is a degenerate fit with status OK."""
    seqs = [np.zeros(1200, np.uint8) + 2] * 3 + [np.zeros(0, np.uint8)]
    res, offs, lens = S.pack_targets(seqs)
    bt = Batch(res, offs, lens)
    with S.ScoreBank() as bank:
        bank.set_penalties(*SC.REF)
        bank.load_query(np.zeros(1200, np.uint8) + 2)  # shuffles of a one-letter target are itself
        (st,) = bank.estimate_statistics_device(*bt.ptrs(), bt.n, bt.max_len, seed=1, rounds=2)
    assert st.degenerate and st.clamped and st.flags == S.STAT_DEGENERATE | S.STAT_CLAMPED
    assert (st.n_samples, st.n_clamped, st.min_score, st.max_score) == (6, 6, 4095, 4095)
    assert (st.lambda_, st.K, st.query_len) == (0.0, 0.0, 1200)


# ---- 4. significance of hits ------------------------------------------------------------------
def _want_sig(st, scores, tlens, db):
    s = np.asarray(scores, np.float64)
    bits = (st.lambda_ * s - np.log(st.K)) / np.log(2.0)
    ev = db * st.K * st.query_len * np.asarray(tlens, np.float64) * np.exp(-st.lambda_ * s)
    return bits, ev


def test_chain_top_hits_significance_golden():
    """score -> top hits -> significance on one stream, with the Lambda and K ssearch36 printed:
    db211 and db428 with the bits and E of the reference's report; a thresholded row's sentinel
    tail gets -inf / +inf."""
    torch = _torch()
    lam, K, db, qlen, hits = SC.golden_stats()
    q, res, offs, lens = SC.golden()
    names = [n for n, _ in O.read_fasta(O.golden_fasta("data500.fa"))]
    bt = Batch(res, offs, lens)
    st = S.make_statistics(lam, K, len(q))
    assert len(q) == qlen
    k, dev = 12, torch.device("cuda", 0)
    d_scores = torch.full((bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    with S.ScoreBank() as bank:
        bank.set_penalties(*SC.REF)
        bank.load_query(q)
        for min_score, outs in ((None, "be"), (68, "be"), (68, "b"), (68, "e")):
            d_hits, d_hsc = _filled(k * 8), _filled(k * 4)
            d_bits, d_ev = _filled(k * 8), _filled(k * 8)
            torch.cuda.synchronize()
            h = stream.cuda_stream
            bank.score_batch_device(*bt.ptrs(), bt.n, bt.max_len, d_scores.data_ptr(), stream=h)
            bank.top_hits_device(d_scores.data_ptr(), bt.n, k, d_hits.data_ptr(),
                                 min_score=min_score, d_hit_scores=d_hsc.data_ptr(), stream=h)
            bank.hit_significance_device(st, d_hsc.data_ptr(), d_hits.data_ptr(),
                                         bt.d_lens.data_ptr(), k, db,
                                         d_bits=d_bits.data_ptr() if "b" in outs else 0,
                                         d_evalues=d_ev.data_ptr() if "e" in outs else 0, stream=h)
            assert bank.last_kernel() == f"significance nq=1 k={k}"
            bank.sync()
            stream.synchronize()
            pos = d_hits.cpu().numpy().view(np.uint64)
            hsc = d_hsc.cpu().numpy().view(np.int32)
            bits, ev = d_bits.cpu().numpy().view(np.float64), d_ev.cpu().numpy().view(np.float64)
            cnt = int((pos != S.HIT_NONE).sum())
            assert cnt == (k if min_score is None else int((hsc >= 68).sum())) and 2 <= cnt
            if min_score is not None:
                assert cnt < k  # a sentinel tail
            wb, we = _want_sig(st, hsc[:cnt], lens[pos[:cnt].astype(np.int64)], db)
            if "b" in outs:
                assert np.allclose(bits[:cnt], wb, rtol=SIG_RTOL, atol=0)
                assert (bits[cnt:] == -np.inf).all()
                assert ["%.1f" % x for x in bits[:2]] == [hits[0][3], hits[1][3]]
            else:
                assert (d_bits.cpu().numpy() == FILL).all()
            if "e" in outs:
                assert np.allclose(ev[:cnt], we, rtol=SIG_RTOL, atol=0)
                assert (ev[cnt:] == np.inf).all()
                assert ["%.2g" % x for x in ev[:2]] == [hits[0][4], hits[1][4]]
            else:
                assert (d_ev.cpu().numpy() == FILL).all()
            assert [(names[int(p)], int(s)) for p, s in zip(pos[:2], hsc[:2])] == \
                [(hh[0], hh[2]) for hh in hits]


def test_significance_rows_use_their_own_statistics():
    torch = _torch()
    _, res, offs, lens = SC.golden()
    bt = Batch(res, offs, lens)
    queries = _set_queries()
    nq, k, db = 3, 9, bt.n
    stats = [S.make_statistics(0.18 + 0.01 * i, 0.1 / (i + 1), len(q))
             for i, q in enumerate(queries)]
    dev = torch.device("cuda", 0)
    d_scores = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_hits, d_hsc = _filled(nq * k * 8), _filled(nq * k * 4)
    d_bits, d_ev = _filled(nq * k * 8), _filled(nq * k * 8)
    torch.cuda.synchronize()
    for devices in (None, [0, 0]):  # a multi-device bank runs it on its root
        with S.ScoreBank(devices=devices) as bank:
            bank.set_penalties(*SC.REF)
            bank.load_queries(queries)
            bank.score_batch_device(*bt.ptrs(), bt.n, bt.max_len, d_scores.data_ptr())
            bank.top_hits_device(d_scores.data_ptr(), bt.n, k, d_hits.data_ptr(), nq=nq,
                                 d_hit_scores=d_hsc.data_ptr())
            for _ in range(2):  # back to back: the second upload waits for the first kernel
                bank.hit_significance_device(stats, d_hsc.data_ptr(), d_hits.data_ptr(),
                                             bt.d_lens.data_ptr(), k, db,
                                             d_bits=d_bits.data_ptr(), d_evalues=d_ev.data_ptr())
            assert bank.last_kernel() == f"significance nq={nq} k={k}"
            bank.sync()
        pos = d_hits.cpu().numpy().view(np.uint64).reshape(nq, k).astype(np.int64)
        hsc = d_hsc.cpu().numpy().view(np.int32).reshape(nq, k)
        bits = d_bits.cpu().numpy().view(np.float64).reshape(nq, k)
        ev = d_ev.cpu().numpy().view(np.float64).reshape(nq, k)
        for i in range(nq):
            wb, we = _want_sig(stats[i], hsc[i], lens[pos[i]], db)
            assert np.allclose(bits[i], wb, rtol=SIG_RTOL, atol=0), i
            assert np.allclose(ev[i], we, rtol=SIG_RTOL, atol=0), i
            hb, he = S.hit_significance(stats[i], hsc[i], lens[pos[i]], db)
            assert np.allclose(bits[i], hb, rtol=SIG_RTOL, atol=0)
            assert np.allclose(ev[i], he, rtol=SIG_RTOL, atol=0)


# ---- 5. the CLI -----------------------------------------------------------------------------------
def _cli(*args):
    q, lib = O.golden_fasta("query100.fa"), O.golden_fasta("data500.fa")
    r = subprocess.run([S.CLI_PATH, "-q", q, "-l", lib, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_cli_prints_statistics_bits_and_evalues():
    q, res, offs, lens = SC.golden()
    n = len(lens)
    plain = _cli("-A", "2")
    given = _cli("-A", "2", "-S", "0.1840,0.1293")
    assert given[:n] == plain[:n]
    assert given[n] == "Statistics: Lambda= 0.1840;  K=0.1293 (0 samples)"
    opt = [ln for ln in given if ln.startswith(" s-w opt:")]
    assert opt == [" s-w opt: 78  bits: 23.7 E(499): 0.62", " s-w opt: 72  bits: 22.1 E(499): 1.9"]
    # the rest is what the CLI prints without the flags
    strip = lambda lines: [ln.split("  bits:")[0] for ln in lines if not ln.startswith("Statistics:")]
    assert strip(given) == plain
    assert not any("bits:" in ln or ln.startswith("Statistics:") for ln in plain)
    est = _cli("-A", "2", "-E", "1,7")
    with S.ScoreBank() as bank:
        bank.set_penalties(*SC.REF)
        bank.load_query(q)
        (st,) = bank.estimate_statistics(res, offs, lens, seed=7, rounds=1)
    assert est[n] == "Statistics: Lambda= %.4f;  K=%.4f (%d samples)" % (st.lambda_, st.K, n)
    bits, ev = S.hit_significance(st, [78, 72], [128, 128], n)
    assert [ln for ln in est if ln.startswith(" s-w opt:")] == \
        [" s-w opt: %d  bits: %.1f E(%d): %.2g" % (s, b, n, e) for s, b, e in zip((78, 72), bits, ev)]
    assert strip(est) == plain


# ---- 6. arguments and state -----------------------------------------------------------------------
def test_argument_and_state_errors():
    torch = _torch()
    q, res, offs, lens = SC.golden()
    bt = Batch(res, offs, lens)
    d_out = _filled(len(res))
    d_c = _zeros64(SC.BINS)
    d_scores = torch.zeros((bt.n,), dtype=torch.int32, device=torch.device("cuda", 0))
    d_hits = _to_dev(np.arange(4, dtype=np.uint64))
    d_dbl = _filled(4 * 8)
    torch.cuda.synchronize()
    good = S.make_statistics(0.184, 0.1293, 128)

    def err(status, fn, *a, **kw):
        with pytest.raises(S.SwbankError) as e:
            fn(*a, **kw)
        assert e.value.status == status, (fn.__name__, a, kw)

    with S.ScoreBank() as bank:
        r, o, l = bt.ptrs()
        # shuffle
        for a in ((0, o, l, bt.n), (r, 0, l, bt.n), (r, o, 0, bt.n), (r, o, l, 0), (r, o, l, 1 << 32)):
            err(S.ERR_ARG, bank.shuffle_batch_device, *a, bt.max_len, 1, d_out.data_ptr())
        err(S.ERR_ARG, bank.shuffle_batch_device, r, o, l, bt.n, bt.max_len, 1, 0)
        # histogram
        s = d_scores.data_ptr()
        for kw in (dict(d_scores=0), dict(d_counts=0), dict(n=0), dict(nq=0),
                   dict(n=(1 << 32) + 1), dict(nq=1 << 62, n=8), dict(nq=1 << 60, n=1)):
            args = dict(d_scores=s, n=bt.n, d_counts=d_c.data_ptr(), nq=1)
            args.update(kw)
            err(S.ERR_ARG, bank.score_histogram_device, **args)
        # the estimate: state first, then arguments
        err(S.ERR_STATE, bank.estimate_statistics_device, r, o, l, bt.n, bt.max_len)
        err(S.ERR_STATE, bank.estimate_statistics, res, offs, lens)
        bank.set_penalties(*SC.REF)
        err(S.ERR_STATE, bank.estimate_statistics_device, r, o, l, bt.n, bt.max_len)
        bank.load_query(q)
        for a in ((0, o, l, bt.n), (r, 0, l, bt.n), (r, o, 0, bt.n), (r, o, l, 0), (r, o, l, 1 << 32)):
            err(S.ERR_ARG, bank.estimate_statistics_device, *a, bt.max_len)
        err(S.ERR_ARG, bank.estimate_statistics_device, r, o, l, bt.n, bt.max_len, rounds=0)
        err(S.ERR_ARG, bank.estimate_statistics_device, r, o, l, bt.n, 100, min_len=101)
        err(S.ERR_ARG, bank.estimate_statistics, res, offs, lens, rounds=0)
        err(S.ERR_ARG, bank.estimate_statistics, res[:100], offs, lens)  # a target outside
        st1 = S.Statistics()
        L = S.lib()
        assert L.sw_estimate_statistics_device(bank._h, r, o, l, bt.n, 0, bt.max_len, 1, 1, None,
                                               None) == S.ERR_ARG
        assert L.sw_estimate_statistics_device(None, r, o, l, bt.n, 0, bt.max_len, 1, 1,
                                               ctypes.byref(st1), None) == S.ERR_ARG
        assert L.sw_shuffle_batch_device(None, r, o, l, bt.n, bt.max_len, 1, d_out.data_ptr(),
                                         None) == S.ERR_ARG
        assert L.sw_score_histogram_device(None, s, None, bt.n, 1, d_c.data_ptr(), None, None,
                                           None) == S.ERR_ARG
        # significance
        sig = dict(d_hit_scores=s, d_hits=d_hits.data_ptr(), d_lens=l, hits_per_query=4,
                   db_size=9, d_bits=d_dbl.data_ptr())
        for kw in (dict(d_hit_scores=0), dict(d_hits=0), dict(d_lens=0), dict(hits_per_query=0),
                   dict(d_bits=0), dict(hits_per_query=1 << 62)):
            args = dict(sig)
            args.update(kw)
            err(S.ERR_ARG, bank.hit_significance_device, good, **args)
        err(S.ERR_ARG, bank.hit_significance_device, [], **sig)  # nq == 0
        for bad in (S.make_statistics(0.0, 0.1, 10), S.Statistics(lambda_=0.2, K=0.1, query_len=10,
                                                                  flags=S.STAT_DEGENERATE)):
            err(S.ERR_ARG, bank.hit_significance_device, [good, bad], **sig)
        assert L.sw_hit_significance_device(None, None, s, d_hits.data_ptr(), l, 4, 1, 9,
                                            d_dbl.data_ptr(), None, None) == S.ERR_ARG
        bank.sync()
        # nothing was written by any refused call
        assert (d_out.cpu().numpy() == FILL).all() and (d_dbl.cpu().numpy() == FILL).all()
        assert not d_c.cpu().numpy().any()
    assert S.STAT_BINS == SC.BINS == 4096
