"""The tile kernel's hand-off rows with one row stride: ring and edge rows of 65
entries, the constant row -1 boundary in entry 64 of the first slot's rows, the last wave's
bottom row written into the slot it is reading.

 a. ring aliasing: merged DNA through the pair-table kernel and (SWBANK_PAIR=0) the row-LUT
    kernel, 1-4 waves (at 2 waves wave 0's consumer is the last wave), one and two chunks per
    tile with both slot parities and a partial last chunk, batch ends at, before and after a
    tile's end;
 b. segments: edge rows in (DMA into 65-entry rows) and out (read back from the aliased slot),
    a first segment of 16 waves, segments of 4 waves and a last one of a single wave, merged and
    Gotoh (4-column chunks), a 3-query set.  A query runs as segments only when it is taller
    than one workgroup (16 waves), so the 129-row query runs as one workgroup of 9 waves here;
 c. balanced ranges: the smallest batch the host sends to the balanced kernel at a grid of
    1,024 (two tiles per workgroup and one more), every score against the oracle.

Every score is checked against the oracle on poisoned device buffers."""
import re

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

REF = (5, -4, -12, -4)
GOTOH = (5, -4, -10, -1)
pytestmark = pytest.mark.gpu


def _exact(got, want, *ctx):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    assert bad.size == 0, (ctx, int(bad.size),
                           [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])


def _uniform(seed, q, n, L):
    """n targets of L codes: every other one a stretch of the query (so alignments start in row
    0 and cross every wave and segment boundary) with a few substitutions, the rest random."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, (n, L), dtype=np.uint8)
    for k in range(0, n, 2):
        a = 0 if k % 4 == 0 or len(q) <= L else int(rng.integers(0, len(q) - L + 1))
        m = min(L, len(q) - a)
        t[k, :m] = q[a:a + m]
        if m > 4:
            t[k, int(rng.integers(0, m))] ^= 1
    return t


def _oracle(q, t, pen, model=O.GAP_MERGED):
    n, L = t.shape
    return O.score_batch(q, np.ascontiguousarray(t.reshape(-1)),
                         np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32),
                         O.dna_matrix(*pen[:2]), pen[2], pen[3], model)


# ---- a. ring aliasing --------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [True, False])
@pytest.mark.parametrize("qlen", [32, 33, 64, 96, 128])
def test_ring_aliasing(qlen, pair, poisoned_buffers, monkeypatch):
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    if not pair:
        monkeypatch.setenv("SWBANK_PAIR", "0")
    q = O.random_codes(900 + qlen, qlen, 4)
    with S.ScoreBank() as bank:
        bank.set_penalties(*REF)
        bank.load_query(q)
        for L in (1, 7, 8, 9, 15, 16, 17, 24):
            t = _uniform(qlen * 100 + L, q, 257, L)
            want = _oracle(q, t, REF)
            for n in (1, 127, 128, 129, 257):
                got = bank.score_targets(list(t[:n]))
                kern = bank.last_kernel()
                m = re.match(r"tile f16( pair)? R=32 W=(\d+) segs=1", kern)
                assert m and bool(m.group(1)) == pair and int(m.group(2)) == -(-qlen // 32), kern
                _exact(got, want[:n], kern, qlen, L, n)


# ---- b. segments -------------------------------------------------------------------------------
def _seg_env(monkeypatch, seg):
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    monkeypatch.setenv("SWBANK_R", "16")
    if seg:
        monkeypatch.setenv("SWBANK_SEG", seg)


@pytest.mark.parametrize("model", ["merged", "gotoh"])
@pytest.mark.parametrize("qlen,seg,segs", [(257, None, 2), (257, "64", 5), (129, "64", 1)])
def test_segments_through_wide_rows(qlen, seg, segs, model, poisoned_buffers, monkeypatch):
    """257 rows at 16 rows per wave: 256 + 1 (16 waves writing edge rows, then one wave reading
    them: its boundary and its sink are both edge / ring rows), or 4 x 64 + 1; 129 rows stay one
    workgroup of 9 waves."""
    _seg_env(monkeypatch, seg)
    pen, gm, om = (GOTOH, S.GAP_GOTOH, O.GAP_GOTOH) if model == "gotoh" else \
        (REF, S.GAP_MERGED, O.GAP_MERGED)
    q = O.random_codes(1300 + qlen, qlen, 4)
    with S.ScoreBank(gap_model=gm) as bank:
        bank.set_penalties(*pen)
        bank.load_query(q)
        for L in (17, 128):
            t = _uniform(qlen + L, q, 300, L)
            got = bank.score_targets(list(t))
            kern = bank.last_kernel()
            m = re.search(r" R=16 W=(\d+) segs=(\d+)", kern)
            assert kern.startswith("tile f16") and m and int(m.group(2)) == segs, kern
            if model == "gotoh":
                assert " pair " in kern, kern
            _exact(got, _oracle(q, t, pen, om), kern, qlen, L)


def test_segments_query_set(poisoned_buffers, monkeypatch):
    """Three queries in one launch per segment (units = (query, tile) pairs, per-unit edge
    rows): the tallest sets the layout, several segments with a last one of a single row."""
    torch = pytest.importorskip("torch")
    _seg_env(monkeypatch, "64")
    dev = torch.device("cuda", 0)
    queries = [O.random_codes(1500 + L, L, 4) for L in (257, 129, 33)]
    with S.ScoreBank() as bank:
        bank.set_penalties(*REF)
        bank.load_queries(queries)
        for L in (17, 128):
            t = _uniform(2000 + L, queries[0], 300, L)
            n = len(t)
            d_res = torch.from_numpy(np.ascontiguousarray(t.reshape(-1))).to(dev)
            d_offs = torch.from_numpy(np.arange(n, dtype=np.int64) * L).to(dev)
            d_lens = torch.from_numpy(np.full(n, L, np.int32)).to(dev)
            d_sc = torch.full((len(queries), n), -1, dtype=torch.int32, device=dev)
            st = torch.cuda.Stream()
            bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                    d_sc.data_ptr(), st.cuda_stream)
            st.synchronize()
            kern = bank.last_kernel()
            m = re.search(r" segs=(\d+) queries=3", kern)  # (the set's own segment layout)
            assert kern.startswith("tile f16") and m and int(m.group(1)) >= 2, kern
            got = d_sc.cpu().numpy()
            for i, q in enumerate(queries):
                _exact(got[i], _oracle(q, t, REF), kern, i, L)


# ---- c. balanced ranges ------------------------------------------------------------------------
@pytest.mark.parametrize("L", [24, 128])
def test_balanced_smallest_batch(L, poisoned_buffers):
    """262,144 + 128 targets: 2,049 tiles, two per workgroup of a 1,024 grid and one more.  The
    targets are drawn from 8,192 distinct ones, so the oracle scores every one of them."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n, P = 262_144 + 128, 8192
    q = O.random_codes(77, 100, 4)
    pool = _uniform(L, q, P, L)
    pick = np.random.default_rng(L).integers(0, P, n)
    want = _oracle(q, pool, REF)[pick]
    d_res = torch.from_numpy(np.ascontiguousarray(pool[pick].reshape(-1))).to(dev)
    d_offs = torch.from_numpy(np.arange(n, dtype=np.int64) * L).to(dev)
    d_lens = torch.from_numpy(np.full(n, L, np.int32)).to(dev)
    sc = torch.full((n,), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    with S.ScoreBank() as bank:
        bank.set_penalties(*REF)
        bank.load_query(q)
        before = bank.counters()
        bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                sc.data_ptr(), st.cuda_stream, min_len=L)
        st.synchronize()
        kern, ctr = bank.last_kernel(), bank.counters()
    assert "pair" in kern and "balanced grid=" in kern, kern
    assert ctr["balanced_calls"] == before["balanced_calls"] + 1, ctr
    assert all(ctr[k] == before[k] for k in ctr if "timeout" in k), ctr
    grid = int(re.search(r"grid=(\d+)", kern).group(1))
    assert 2 * grid <= (n + 127) // 128, kern
    _exact(sc.cpu().numpy(), want, kern, L)
