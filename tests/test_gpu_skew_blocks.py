"""GPU: the block-framed skewed rows of the merged pair kernel: frames restart
every 8 rows, a block's first row takes T~ of the row above shifted by -8e, and the running best
is four accumulators, each folding two row classes (r mod 8) of all four blocks of a wave.
Everything is compared with the oracle, and `last_kernel` must say " skew".

* the best made in every row class and column class, at every block and wave boundary row;
* live vertical gap runs over the seams inside a wave (rows 7|8, 15|16, 23|24) and between waves
  (31|32, 63|64, 95|96), beside targets of every chunk-edge length;
* balanced ranges whose cuts carry a live value in every accumulator (uniform batch: the
  balanced kernel; ragged: the trimmed one), twice back to back on poisoned buffers;
* all-N targets and an all-N query: nothing leaves the floors.
tests/test_skew_block_model.py restates the rows on the CPU."""
import collections

import numpy as np
import pytest

import seam_cases as SC
import swbank as S
from oracle import oracle as O
from test_gpu_skew import SLOTS, _Batch, _check

pytestmark = pytest.mark.gpu

REF = (5, -4, -12, -4)
E8 = (5, -4, -12, -8)
BOUNDARY_ROWS = (7, 8, 15, 16, 23, 24, 31, 32, 63, 64, 95, 96, 127)


def _bank(pens, q):
    bank = S.ScoreBank()
    bank.set_penalties(*pens)
    bank.load_query(q)
    return bank


def _planted(rng, q, r, c, L):
    """An L-bp random target with query rows [r - 11, r] copied to columns [c - 11, c]."""
    t = rng.integers(0, 4, L).astype(np.uint8)
    t[c - 11:c + 1] = q[r - 11:r + 1]
    return t


def _class_targets(rng, q, n):
    """n targets of 24-64 bp, each with a 12-row hit ending at (r, c): r runs over the boundary
    rows first and then over every row, and for each row class (r mod 8) the column classes
    (c mod 8) come in turn, so n >= 8 x 8 x 2 targets cover all 64 pairs."""
    m = len(q)
    rows = [r for r in BOUNDARY_ROWS if 11 <= r < m] + list(range(11, m))
    turn = collections.Counter()
    seqs, seen = [], set()
    for k in range(n):
        r = rows[k % len(rows)]
        t = turn[r % 8]
        turn[r % 8] += 1
        c = 16 + 3 * t % 8 + 8 * (t // 8 % 3)  # (3 t mod 8 runs through all 8 column classes)
        L = int(rng.integers(max(24, c + 1), 65))
        seqs.append(_planted(rng, q, r, c, L))
        seen.add((r % 8, c % 8))
    return seqs, seen


@pytest.mark.parametrize("pens", [REF, E8], ids=["e4", "e8"])
@pytest.mark.parametrize("qlen", [17, 33, 40, 64, 100, 128])
def test_best_in_every_row_and_column_class(qlen, pens, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    rng = np.random.default_rng(7 * qlen + pens[3])
    q = O.random_codes(300 + qlen, qlen, 4)
    seqs, seen = _class_targets(rng, q, 300)
    assert len(seen) == 8 * len({r % 8 for r in range(11, qlen)}), len(seen)  # (64 from 19 rows)
    assert 5 * min(qlen, 64) + 5 - pens[3] * ((qlen + 31) // 32 * 32 + 64) <= 2048
    for poison in ("0", "1"):
        monkeypatch.setenv("SWBANK_POISON", poison)
        with _bank(pens, q) as bank:
            for n in (1, 127, 128, 129, 300):
                b = _Batch(torch, seqs[:n])
                (got,) = b.score(torch, bank)
                kern = bank.last_kernel()
                assert kern.startswith(f"tile f16 pair R=32 W={(qlen + 31) // 32} segs=1") and \
                    " skew" in kern, kern
                want = b.want(q, pens)
                _check(got, want, kern, qlen, pens, n, poison)
    assert (want >= 60).mean() > 0.9  # (the planted hits are the bests)


@pytest.mark.parametrize("pens", [REF, E8], ids=["e4", "e8"])
def test_live_gaps_over_block_and_wave_seams(pens, monkeypatch):
    """Deletion targets (tests/seam_cases.py) whose vertical gap run lies over rows 7|8, 15|16,
    23|24 (block seams inside a wave: the shifted T~up) and 31|32, 63|64, 95|96 (wave seams: the
    shifted ring entry), at least 4 per cut, in one batch with targets of 1, 7, 8, 9, 17 and 63
    bp.  The CPU mutant that drops the gap state on crossing the cut changes most of a cut's
    scores, so the gaps are live."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    cuts = [8, 16, 24, 32, 64, 96]
    rng = np.random.default_rng(31 - pens[3])
    for attempt in range(64):
        q = rng.integers(0, 4, 128).astype(np.uint8)
        try:  # e = 8: short flanks, so that the batch stays inside the launch bound
            tg, meta = SC.straddle_targets(q, 4, cuts, [], None, rng, per=6,
                                           flank=None if pens is REF else 14)
            break
        except ValueError:
            continue
    count = collections.Counter(m.cut for m in meta)
    assert all(count[c] >= 4 for c in cuts), count
    sub = O.dna_matrix(*pens[:2])
    for c in cuts:  # the seam is live: losing the gap state there changes the score
        ts = [t for t, m in zip(tg, meta) if m.cut == c]
        full = SC.scores_with_cut(q, ts, sub, pens[2], pens[3], SC.GAP_MERGED)
        cut = SC.scores_with_cut(q, ts, sub, pens[2], pens[3], SC.GAP_MERGED, cut_row=c)
        assert (full != cut).mean() >= 0.5, (c, full, cut)
    edge = [q[40:40 + L].copy() if k % 2 else rng.integers(0, 4, L).astype(np.uint8)
            for k, L in enumerate((1, 7, 8, 9, 17, 63) * 4)]
    order = rng.permutation(len(tg) + len(edge))
    seqs = [(tg + edge)[k] for k in order]
    top = max(len(t) for t in seqs)
    assert 5 * min(128, top) + 5 - pens[3] * (128 + (top + 7) // 8 * 8) <= 2048
    for poison in ("0", "1"):
        monkeypatch.setenv("SWBANK_POISON", poison)
        with _bank(pens, q) as bank:
            b = _Batch(torch, seqs)
            (got,) = b.score(torch, bank)
            kern = bank.last_kernel()
        assert kern.startswith("tile f16 pair R=32 W=4 segs=1") and " skew" in kern, kern
        _check(got, b.want(q, pens), kern, pens, poison)


def _plant_hits(q, res, offs, lens):
    """One target in 20 gets query rows [r - 11, r] in its first 16 columns, r stepping through
    every row of the query: at every cut of a balanced range each accumulator holds a best made
    before the cut, which has to cross the hand-off."""
    n, m = len(lens), len(q)
    for i, k in enumerate(range(3, n, 20)):
        r = 11 + i % (m - 11)
        c0 = int(offs[k]) + i % 5
        res[c0:c0 + 12] = q[r - 11:r + 1]
    return n // 20


def _balanced(torch, monkeypatch, q, b, tokens):
    with _bank(REF, q) as bank:
        a1, a2 = b.score(torch, bank, calls=2)
        kern, ctr = bank.last_kernel(), bank.counters()
    assert " skew" in kern and all(t in kern for t in tokens), kern
    assert ctr["balanced_calls"] == 2 and ctr["balanced_timeouts"] == 0, ctr
    assert np.array_equal(a1, a2)
    rng = np.random.default_rng(17)
    rows = np.unique(np.concatenate([rng.choice(b.n, 20_000, replace=False), np.arange(300),
                                     np.arange(b.n - 300, b.n)]))
    want = b.want(q, REF, rows)
    _check(a1[rows], want, kern)
    return want


def test_balanced_cut_carries_every_accumulator(poisoned_buffers, monkeypatch):
    """The smallest uniform batch that runs balanced chunk ranges (as
    test_gpu_skew.py::test_balanced_uniform), with bests planted in the first 16 columns."""
    torch = pytest.importorskip("torch")
    qlen, L = 128, 124
    n = 2 * SLOTS * 128 + 1
    q = O.random_codes(177, qlen, 4)
    res = O.random_codes(178, n * L, 4)
    offs, lens = np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32)
    _plant_hits(q, res, offs, lens)
    b = _Batch(torch, packed=(res, offs, lens))
    want = _balanced(torch, monkeypatch, q, b, ["balanced grid="])
    assert (want >= 60).mean() > 0.04  # (the planted hits are in the sample)


def test_balanced_ragged_cut_carries_every_accumulator(poisoned_buffers, monkeypatch):
    """The ragged [64, 150] batch of test_gpu_skew.py::test_balanced_ragged_trimmed (the trimmed
    kernel), with the same planted bests."""
    torch = pytest.importorskip("torch")
    lo, hi, qlen = 64, 150, 128
    n = (2 * SLOTS * 19 // 8 + 4) * 128
    rng = np.random.default_rng(12)
    q = O.random_codes(191, qlen, 4)
    lens = rng.integers(lo, hi + 1, n).astype(np.uint32)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    res = O.random_codes(192, int(lens.sum(dtype=np.uint64)), 4)
    _plant_hits(q, res, offs, lens)
    b = _Batch(torch, packed=(res, offs, lens))
    want = _balanced(torch, monkeypatch, q, b, ["dsort", "balanced grid="])
    assert (want >= 60).mean() > 0.04


@pytest.mark.parametrize("pens", [REF, E8], ids=["e4", "e8"])
def test_all_n(pens, monkeypatch):
    """All-N targets, and an all-N query against ordinary targets: no H^ leaves its floor."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    rng = np.random.default_rng(6)
    q = O.random_codes(19, 100, 4)
    seqs = [np.full(int(L), 4, np.uint8) for L in rng.integers(1, 65, 200)]
    seqs += [rng.integers(0, 4, int(L)).astype(np.uint8) for L in rng.integers(1, 65, 100)]
    b = _Batch(torch, seqs)
    for query in (q, np.full(100, 4, np.uint8)):
        for poison in ("0", "1"):
            monkeypatch.setenv("SWBANK_POISON", poison)
            with _bank(pens, query) as bank:
                (got,) = b.score(torch, bank)
                kern = bank.last_kernel()
            assert " skew" in kern, kern
            want = b.want(query, pens)
            _check(got, want, kern, pens, poison)
        assert (want[:200] == 0).all()
