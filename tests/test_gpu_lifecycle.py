"""A bank's life on the GPU, seen from outside: every buffer a bank reserved is freed when it is
closed (the library's count of live buffers, swbank_live_buffers, returns to where it was), a
multi-device bank hands its root's refusal on behind "device N: ", and every entry after scoring
brackets as many launch groups for sw_bank_set_timing as it always did.

The shapes are the smallest that cross a seam: 130 ragged targets of 1..40 bases (past the
128-target tile and the 64-target group of the small kernels), a 24-base query, three queries
where an entry takes a set."""
import ctypes
import gc

import numpy as np
import pytest

import swbank as S

pytestmark = pytest.mark.gpu

PEN = (5, -4, -12, -4)
N, K = 130, 5
_RNG = np.random.default_rng(20261020)
SEQS = [_RNG.integers(0, 4, int(l)).astype(np.uint8) for l in _RNG.integers(1, 41, N)]
QUERY = _RNG.integers(0, 4, 24).astype(np.uint8)
QUERIES = [QUERY, _RNG.integers(0, 4, 17).astype(np.uint8), _RNG.integers(0, 4, 9).astype(np.uint8)]
NQ = len(QUERIES)
RES, OFFS, LENS = S.pack_targets(SEQS)
MAX_LEN = int(LENS.max())
assert int(LENS.min()) == 1 and MAX_LEN == 40


def _torch():
    import torch
    return torch


def _to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return _torch().from_numpy(a).to(_torch().device("cuda", 0))


def _zeros(nbytes):
    torch = _torch()
    return torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=torch.device("cuda", 0))


class Dev:
    """The batch (16 zero bytes behind the last target) and the outputs of every device entry."""

    def __init__(self):
        self.res = _to_dev(np.concatenate([RES, np.zeros(16, np.uint8)]))
        self.offs, self.lens = _to_dev(OFFS), _to_dev(LENS)
        self.scores = _zeros(NQ * N * 4)
        self.hits, self.hsc, self.cnt = _zeros(NQ * K * 8), _zeros(NQ * K * 4), _zeros(NQ * 4)
        self.bq, self.bs = _zeros(N * 4), _zeros(N * 4)
        self.bits, self.ev = _zeros(NQ * K * 8), _zeros(NQ * K * 8)
        self.codes = _zeros(len(RES) + 16)
        self.hist = _zeros(NQ * S.STAT_BINS * 8)
        self.recs = _zeros(K * S.ALIGNMENT_DTYPE.itemsize)
        self.cigar = _zeros(K * 2 * (MAX_LEN + 24) * 4)
        _torch().cuda.synchronize()

    def batch(self):
        return self.res.data_ptr(), self.offs.data_ptr(), self.lens.data_ptr()


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _live():
    f = S.lib().swbank_live_buffers
    f.restype = ctypes.c_long
    f.argtypes = []
    return int(f())


def _baseline():
    gc.collect()  # (banks of earlier tests that nobody closed)
    return _live()


STATS = [S.make_statistics(0.19, 0.1, len(q)) for q in QUERIES]


def _every_family(bank, dev):
    """One call of every family of entries, the single-query ones first."""
    bank.set_penalties(*PEN)
    bank.load_query(QUERY)
    scores = bank.score_batch(RES, OFFS, LENS)
    bank.score_batch_device(*dev.batch(), N, MAX_LEN, dev.scores.data_ptr())
    hits = bank.top_hits(scores, K)[0]
    bank.top_hits_device(dev.scores.data_ptr(), N, K, dev.hits.data_ptr(),
                         d_hit_scores=dev.hsc.data_ptr(), d_counts=dev.cnt.data_ptr())
    bank.hit_significance_device(STATS[:1], dev.hsc.data_ptr(), dev.hits.data_ptr(),
                                 dev.lens.data_ptr(), K, N, d_bits=dev.bits.data_ptr(),
                                 d_evalues=dev.ev.data_ptr())
    bank.revcomp_batch_device(*dev.batch(), N, dev.codes.data_ptr())
    bank.sync()
    got = bank.align_hits(RES, OFFS, LENS, hits)  # with CIGARs
    assert len(got) == K and any(a.has_path for a in got)
    bank.load_queries(QUERIES)
    matrix = np.random.default_rng(5).integers(0, 100, (NQ, N)).astype(np.int32)
    bq, bs = bank.best_queries(matrix)
    assert np.array_equal(bs, matrix.max(axis=0))
    assert len(bank.estimate_statistics(RES, OFFS, LENS, seed=7, rounds=1)) == NQ
    merged, strands = bank.score_strands(RES, OFFS, LENS)
    assert merged.shape == (NQ, N)
    top = bank.top_hits(merged, K)[0]
    assert len(bank.align_set_hits(RES, OFFS, LENS, hits=top.reshape(-1), hits_per_query=K)) == NQ * K
    assert len(bank.align_strand_hits(RES, OFFS, LENS, strands=strands, hits=top.reshape(-1),
                                      hits_per_query=K)) == NQ * K


# ---- 1. every family, then close -----------------------------------------------------------------
@pytest.mark.parametrize("devices, slice_mb", [(None, None), ([0, 0], None), (None, "1")],
                         ids=["single", "two-on-one", "single-1MiB-slices"])
def test_every_family_then_close_frees_every_buffer(dev, devices, slice_mb, monkeypatch):
    if slice_mb:  # the slice scratch reserved at a slice's size, not the batch's
        monkeypatch.setenv("SWBANK_STAT_MB", slice_mb)
        monkeypatch.setenv("SWBANK_STRAND_MB", slice_mb)
    base = _baseline()
    bank = S.ScoreBank(devices=devices)
    try:
        _every_family(bank, dev)
        assert _live() > base
    finally:
        bank.close()
    assert _live() == base


# ---- 2. cycles and order --------------------------------------------------------------------------
def _light_use(bank):
    bank.set_penalties(*PEN)
    bank.load_query(QUERY)
    scores = bank.score_batch(RES, OFFS, LENS)
    bank.top_hits(scores, K)
    return scores


def test_create_use_close_cycles_return_to_the_baseline():
    base = _baseline()
    for _ in range(3):
        with S.ScoreBank() as bank:
            _light_use(bank)
            assert _live() > base
        assert _live() == base


@pytest.mark.parametrize("reverse", [False, True], ids=["creation-order", "reverse-order"])
def test_two_banks_open_at_once(reverse):
    base = _baseline()
    banks = [S.ScoreBank(), S.ScoreBank()]
    try:
        want = _light_use(banks[0])
        one = _live()
        assert np.array_equal(_light_use(banks[1]), want)
        two = _live()
        assert two > one > base
        first, second = banks[::-1] if reverse else banks
        first.close()
        assert base < _live() < two
        assert np.array_equal(second.score_batch(RES, OFFS, LENS), want)  # the other one lives on
    finally:
        for bank in banks:
            bank.close()
    assert _live() == base


def test_close_right_after_a_refused_call():
    base = _baseline()
    bank = S.ScoreBank()
    try:
        scores = _light_use(bank)
        with pytest.raises(S.SwbankError) as e:
            bank.top_hits(scores, 0)
        assert e.value.status == S.ERR_ARG
    finally:
        bank.close()
    assert _live() == base


# ---- 3. a multi-device bank hands its root's refusal on -------------------------------------------
REFUSAL = "alignments under merged gaps"


def _refused_calls():
    hits = np.array([0], np.uint64)
    return {
        "align_targets": (False, lambda bank: bank.align_targets(SEQS, [0])),
        "align_set_hits": (True, lambda bank: bank.align_set_hits(RES, OFFS, LENS, hits=hits,
                                                                  hits_per_query=1)),
        "align_strand_hits": (True, lambda bank: bank.align_strand_hits(RES, OFFS, LENS, hits=hits,
                                                                        hits_per_query=1)),
    }


@pytest.mark.parametrize("entry", ["align_targets", "align_set_hits", "align_strand_hits"])
@pytest.mark.parametrize("devices, prefix", [(None, ""), ([0, 0], "device 0: ")],
                         ids=["single", "two-on-one"])
def test_forwarded_refusal_text_and_last_kernel(dev, entry, devices, prefix):
    takes_set, call = _refused_calls()[entry]
    with S.ScoreBank(devices=devices) as bank:
        bank.set_penalties(5, -4, -2, -1)  # merged gaps with match > open + extend
        if takes_set:
            bank.load_queries(QUERIES)
        else:
            bank.load_query(QUERY)
        bank.score_batch_device(*dev.batch(), N, MAX_LEN, dev.scores.data_ptr())
        bank.sync()
        before = bank.last_kernel()
        assert before
        with pytest.raises(S.SwbankError) as e:
            call(bank)
        assert e.value.status == S.ERR_UNSUPPORTED
        text = S.lib().sw_last_error(bank._h).decode()
        assert text.startswith(prefix + REFUSAL), text
        assert bank.last_kernel() == before


# ---- 4. timed groups per call ----------------------------------------------------------------------
def _timed_calls(dev):
    b = dev.batch()
    sc, hits, hsc, lens = (dev.scores.data_ptr(), dev.hits.data_ptr(), dev.hsc.data_ptr(),
                           dev.lens.data_ptr())
    return {
        "top_hits_device": (1, lambda bank: bank.top_hits_device(sc, N, K, hits, d_hit_scores=hsc)),
        "best_queries_device": (1, lambda bank: bank.best_queries_device(
            sc, N, 1, d_best_query=dev.bq.data_ptr(), d_best_score=dev.bs.data_ptr())),
        "shuffle_batch_device": (1, lambda bank: bank.shuffle_batch_device(
            *b, N, MAX_LEN, 3, dev.codes.data_ptr())),
        "score_histogram_device": (1, lambda bank: bank.score_histogram_device(
            sc, N, dev.hist.data_ptr(), d_lens=lens)),
        "hit_significance_device": (1, lambda bank: bank.hit_significance_device(
            STATS[:1], hsc, hits, lens, K, N, d_bits=dev.bits.data_ptr())),
        "revcomp_batch_device": (1, lambda bank: bank.revcomp_batch_device(
            *b, N, dev.codes.data_ptr())),
        "align_hits_device": (1, lambda bank: bank.align_hits_device(
            *b, N, MAX_LEN, hits, K, dev.recs.data_ptr())),
        "align_hits_device-cigar": (2, lambda bank: bank.align_hits_device(
            *b, N, MAX_LEN, hits, K, dev.recs.data_ptr(), d_cigar=dev.cigar.data_ptr(),
            cigar_stride=2 * (MAX_LEN + 24))),
    }


@pytest.mark.parametrize("entry", ["top_hits_device", "best_queries_device", "shuffle_batch_device",
                                   "score_histogram_device", "hit_significance_device",
                                   "revcomp_batch_device", "align_hits_device",
                                   "align_hits_device-cigar"])
def test_timed_groups_of_one_call(dev, entry):
    want, call = _timed_calls(dev)[entry]
    with S.ScoreBank() as bank:
        bank.set_penalties(*PEN)
        bank.load_query(QUERY)
        bank.score_batch_device(*dev.batch(), N, MAX_LEN, dev.scores.data_ptr())
        bank.top_hits_device(dev.scores.data_ptr(), N, K, dev.hits.data_ptr(),
                             d_hit_scores=dev.hsc.data_ptr())
        bank.sync()
        bank.set_timing(True)
        assert bank.timing()[0] == 0
        call(bank)
        assert bank.timing()[0] == want
        assert bank.timing()[0] == 0  # (read and reset)
