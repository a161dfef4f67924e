"""GPU: the skewed rows' running best in eight accumulators named by frame mod 8 (DESIGN §3.1;
the plain and the balanced pair kernel; the trimmed kernel keeps four).  Every score is compared
with the oracle and `last_kernel` pins the path.

* queries of 1, 8, 9 (the 16-row LUT kernel: no skewed rows), 33, 100 and 128 rows against
  uniform targets of 1 ... 216 bp: one chunk, chunk boundaries, whole and partial last chunks,
  the launch bound (128 rows x 216 bp);
* a planted perfect hit ending in each of the 64 (row class, column class) pairs: anywhere, in
  the query's last row, in the target's last column and in the last chunk a tile runs, so every
  accumulator name holds the best at every rotation and the tile-end merge takes it from every
  name, poisoned buffers and not;
* the balanced kernel on the smallest uniform batch that runs balanced ranges (two tiles per
  resident slot and one target more: 262,145), every target of every cut tile holding a 20-row
  hit in the head part, in the tail part or the same hit in both, so the eight accumulators
  cross the hand-off with the best in them, twice back to back on poisoned buffers; the same
  batch through the plain kernel (SWBANK_BAL=0) element for element;
* one ragged batch, 64-150 bp with N codes, through the trimmed kernel (four accumulators).
tests/test_skew_acc8_model.py restates the accumulators on the CPU."""
import re

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O
from test_gpu_skew import SLOTS, _Batch, _check, _targets

pytestmark = pytest.mark.gpu

REF = (5, -4, -12, -4)


def _bank(q, pens=REF):
    bank = S.ScoreBank()
    bank.set_penalties(*pens)
    bank.load_query(q)
    return bank


@pytest.mark.parametrize("qlen", [1, 8, 9, 33, 100, 128])
def test_uniform_lengths(qlen, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    q = O.random_codes(810 + qlen, qlen, 4)
    rows = (qlen + 31) // 32 * 32
    with _bank(q) as bank:
        for L in (1, 7, 8, 9, 15, 16, 17, 120, 128, 216):
            rng = np.random.default_rng(100 * qlen + L)
            seqs = _targets(rng, q, 300, np.full(300, L))
            for k in range(0, 300, 5):  # the query's end at the target's end: the last columns
                hit = min(qlen, L) - k % 4
                if hit > 0:
                    seqs[k][L - hit:] = q[qlen - hit:]
            fits = 5 * min(qlen, L) + 5 + 4 * (rows + (L + 7) // 8 * 8) <= 2048
            for n in (129, 300):
                b = _Batch(torch, seqs[:n])
                (got,) = b.score(torch, bank)
                kern = bank.last_kernel()
                assert (" skew" in kern) == (qlen > 16 and fits), (kern, qlen, L)
                _check(got, b.want(q, REF), kern, qlen, L, n)


def _planted(rng, q, r, c, L, k=12):
    t = rng.integers(0, 4, L).astype(np.uint8)
    t[c - k + 1:c + 1] = q[r - k + 1:r + 1]
    return t


@pytest.mark.parametrize("qlen", [100, 128])
def test_best_in_every_class_pair_and_at_every_end(qlen, monkeypatch):
    """One batch of mixed lengths (the plain kernel, whole last chunks: a tile runs to its
    longest target rounded up to the chunk)."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    rng = np.random.default_rng(qlen)
    q = O.random_codes(900 + qlen, qlen, 4)
    seqs, anywhere, last_row, last_col, last_chunk = [], set(), set(), set(), set()
    for u in range(8):
        for cc in range(8):
            r = 16 + u + 8 * int(rng.integers(0, (qlen - 24) // 8))
            c = 16 + cc + 8 * int(rng.integers(0, 3))
            assert r % 8 == u and c % 8 == cc and r < qlen
            seqs.append(_planted(rng, q, r, c, int(rng.integers(c + 1, 65))))
            anywhere.add((r % 8, c % 8))
            seqs.append(_planted(rng, q, r, c, c + 1))  # the hit ends in the last column
            last_col.add((r % 8, c % 8))
            seqs.append(_planted(rng, q, r, 56 + cc, 64))  # ... in the last chunk the tile runs
            last_chunk.add((r % 8, (56 + cc) % 8))
        for cc in range(8):  # ... in the query's last row (its class is the query's)
            c = 24 + cc
            seqs.append(_planted(rng, q, qlen - 1, c, int(rng.integers(c + 1, 65))))
            seqs.append(_planted(rng, q, qlen - 1, c, c + 1))
            last_row.add(c % 8)
    assert len(anywhere) == len(last_col) == len(last_chunk) == 64 and len(last_row) == 8
    order = rng.permutation(len(seqs))
    seqs = [seqs[k] for k in order]
    for poison in ("0", "1"):
        monkeypatch.setenv("SWBANK_POISON", poison)
        with _bank(q) as bank:
            for n in (128, len(seqs)):
                b = _Batch(torch, seqs[:n])
                (got,) = b.score(torch, bank)
                kern = bank.last_kernel()
                assert kern.startswith("tile f16 pair R=32 W=4 segs=1") and " skew" in kern, kern
                assert "balanced" not in kern, kern
                want = b.want(q, REF)
                _check(got, want, kern, qlen, n, poison)
    assert (want >= 60).all()  # (the planted hits are the bests)


def _cuts(ntiles, K, grid):
    """{tile: first chunk of its tail part} for the tiles a range boundary splits (the uniform
    plan: workgroup g starts at chunk g * ntiles * K // grid)."""
    at = ntiles * K
    return {(at * g // grid) // K: (at * g // grid) % K for g in range(1, grid)
            if (at * g // grid) % K}


def test_balanced_hand_off_carries_the_best(poisoned_buffers, monkeypatch):
    torch = pytest.importorskip("torch")
    qlen, L, K = 128, 128, 16
    n = 2 * SLOTS * 128 + 1
    ntiles = (n + 127) // 128
    q = O.random_codes(277, qlen, 4)
    res = O.random_codes(278, n * L, 4)
    # the plan follows from the grid, which the kernel line reports: planted for SLOTS, checked
    cuts = {t: ch for t, ch in _cuts(ntiles, K, SLOTS).items() if 3 <= ch <= 13}
    assert len(cuts) >= SLOTS // 2 and set(cuts.values()) == set(range(3, 14))
    kinds = np.zeros(3, np.int64)
    planted = []
    for t, ch in cuts.items():
        for i in range(128):
            k = t * 128 + i
            if k >= n:
                continue
            r = 19 + (i + t) % (qlen - 19)  # (every row class, block and wave boundary rows)
            hit = q[r - 19:r + 1]
            head = 19 + (i * 5 + t) % (8 * ch - 19)            # ends in the head's columns
            tail = 8 * ch + 19 + (i * 3 + t) % (L - 8 * ch - 19)  # ... in the tail's
            kind = i % 3
            tg = res[k * L:(k + 1) * L]
            if kind in (0, 2):
                tg[head - 19:head + 1] = hit
            if kind in (1, 2):
                tg[tail - 19:tail + 1] = hit
            kinds[kind] += 1
            planted.append(k)
    planted = np.array(planted)
    assert kinds.min() > 10_000
    b = _Batch(torch, packed=(res, np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32)))
    out = {}
    for bal in ("1", "0"):
        monkeypatch.setenv("SWBANK_BAL", bal)
        with _bank(q) as bank:
            out[bal] = (b.score(torch, bank, calls=2), bank.last_kernel(), bank.counters())
    (a1, a2), kern, ctr = out["1"]
    (p1, p2), kern0, _ = out["0"]
    assert " skew" in kern and f"balanced grid={SLOTS}" in kern, kern
    assert " skew" in kern0 and "balanced" not in kern0, kern0
    assert int(re.search(r"grid=(\d+)", kern).group(1)) == SLOTS
    assert ctr["balanced_calls"] == 2 and ctr["balanced_timeouts"] == 0, ctr
    rng = np.random.default_rng(5)
    rows = np.unique(np.concatenate([planted[::4], rng.choice(n, 5_000, replace=False),
                                     np.arange(300), np.arange(n - 300, n)]))
    want = b.want(q, REF, rows)
    _check(a1[rows], want, kern)
    assert (want[np.isin(rows, planted)] >= 100).all()  # (the planted hits are the bests)
    assert np.array_equal(a2, a1)
    assert np.array_equal(p1, a1) and np.array_equal(p2, a1)


def test_ragged_trimmed(poisoned_buffers, monkeypatch):
    """[64, 150] bp with 1 % N: the device sort's balanced plan, the trimmed kernel, a tile's last
    chunk ending at any column; hits planted in the targets' last columns."""
    torch = pytest.importorskip("torch")
    lo, hi, qlen = 64, 150, 128
    n = (2 * SLOTS * 19 // 8 + 4) * 128
    rng = np.random.default_rng(21)
    q = O.random_codes(391, qlen, 4)
    lens = rng.integers(lo, hi + 1, n).astype(np.uint32)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    res = O.random_codes(392, int(lens.sum(dtype=np.uint64)), 4)
    res[rng.choice(res.size, res.size // 100, replace=False)] = 4
    for i, k in enumerate(range(5, n, 25)):
        r = 11 + i % (qlen - 11)
        end = int(offs[k]) + int(lens[k]) - i % 9
        res[end - 12:end] = q[r - 11:r + 1]
    b = _Batch(torch, packed=(res, offs, lens))
    with _bank(q) as bank:
        a1, a2 = b.score(torch, bank, calls=2)
        kern, ctr = bank.last_kernel(), bank.counters()
    assert " skew" in kern and "dsort" in kern and "balanced grid=" in kern, kern
    assert ctr["balanced_calls"] == 2 and ctr["balanced_timeouts"] == 0, ctr
    assert np.array_equal(a1, a2)
    rows = np.unique(np.concatenate([np.arange(5, n, 25)[::3], rng.choice(n, 5_000, replace=False),
                                     np.arange(300), np.arange(n - 300, n)]))
    _check(a1[rows], b.want(q, REF, rows), kern)
