"""GPU: the skewed rows of the merged pair kernel: cells held in the frame of
their anti-diagonal, 5 VALU per row.  Every score is compared with the oracle and `last_kernel`
pins the path: " skew" when the batch fits the bound max(s) min(|q|, L) + max(s) + e (rows +
cols) <= 2048 (rows: the query padded to whole 32-row waves; cols: L rounded up to the 8-column
chunk, the columns a tile runs), the unskewed rows past it and with SWBANK_SKEW=0.  The two
balanced batches (262,145 and 623,104 targets) are compared on every target with the unskewed
rows and on 20,000 sampled targets plus the first and last 300 with the oracle, as
test_gpu_balanced.py does; every other batch is compared with the oracle on every target.

Shapes: target lengths at the chunk edges (column 0 pairing with the virtual column -1, the
tile-end fold of the last column's odd rows, a partial last chunk), batches of less than a tile,
a tile and a lane more, queries of 1-4 waves with padded rows, homologous targets scoring near
5 min(m, n) (the top of the range at the largest offsets), N codes; the smallest uniform and
ragged batches that run balanced chunk ranges (the frames resume across a cut tile; poisoned
buffers, back-to-back calls, equal to the unskewed rows element for element); the bound's edge;
penalties with e = 1, e = 8 and larger opens."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REF = (5, -4, -12, -4)
SLOTS = 1024  # resident workgroup slots of the 4-wave pair kernel (4 per CU x 256 CUs)


def _targets(rng, q, n, lens):
    """n targets: mostly the query repeated to the target's length with point changes and 1 % N
    (scores near 5 min(m, n)), some random, some all N."""
    seqs = []
    for k in range(n):
        L = int(lens[k])
        if k % 7 == 3:
            t = rng.integers(0, 4, L).astype(np.uint8)
        else:
            a = int(rng.integers(0, len(q))) if k % 3 == 0 else 0
            t = np.resize(np.roll(q, -a), L).copy()
            x = rng.random(L) < (0.02 if k % 2 else 0.0)
            t[x] = rng.integers(0, 4, int(x.sum()))
            t[rng.random(L) < 0.01] = 4
        if k % 61 == 17:
            t[:] = 4
        seqs.append(t)
    return seqs


class _Batch:
    def __init__(self, torch, seqs=None, packed=None):
        self.res, self.offs, self.lens = packed if packed is not None else O.pack_residues(seqs)
        self.n = len(self.lens)
        dev = torch.device("cuda", 0)
        res = self.res if self.res.size else np.zeros(1, np.uint8)
        self.d_res = torch.from_numpy(res).to(dev)
        self.d_offs = torch.from_numpy(self.offs.astype(np.uint64).view(np.int64)).to(dev)
        self.d_lens = torch.from_numpy(self.lens.astype(np.uint32).view(np.int32)).to(dev)
        self.lo, self.hi = int(self.lens.min()), int(self.lens.max())

    def score(self, torch, bank, calls=1):
        st = torch.cuda.Stream()
        out = []
        for _ in range(calls):
            sc = torch.full((self.n,), -7, dtype=torch.int32, device=self.d_res.device)
            bank.score_batch_device(self.d_res.data_ptr(), self.d_offs.data_ptr(),
                                    self.d_lens.data_ptr(), self.n, self.hi, sc.data_ptr(),
                                    st.cuda_stream, min_len=self.lo)
            out.append(sc)
        st.synchronize()
        return [x.cpu().numpy() for x in out]

    def want(self, q, pens, rows=None):
        offs, lens = self.offs, self.lens
        if rows is not None:
            offs, lens = np.ascontiguousarray(offs[rows]), np.ascontiguousarray(lens[rows])
        return O.score_batch(q, self.res, offs, lens, O.dna_matrix(*pens[:2]), *pens[2:])


def _check(got, want, kern, *ctx):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (kern, ctx, bad.size,
                           [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])


@pytest.mark.parametrize("L", [1, 7, 8, 9, 16, 127, 128, 150])
def test_chunk_edges(L, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    rng = np.random.default_rng(1000 + L)
    for qlen in (2, 31, 32, 33, 64, 127, 128):
        q = O.random_codes(40 + qlen, qlen, 4)
        if qlen > 40:
            q[qlen // 2] = 4  # an N row
        seqs = _targets(rng, q, 1000, np.full(1000, L))
        with S.ScoreBank() as bank:
            bank.set_penalties(*REF)
            bank.load_query(q)
            for n in (1, 127, 128, 129, 1000):
                b = _Batch(torch, seqs[:n])
                (got,) = b.score(torch, bank)
                kern = bank.last_kernel()
                # (<= 16 rows run the 16-row LUT kernel: no pair table, no skewed rows)
                assert (" skew" in kern) == (qlen > 16), (kern, qlen, L, n)
                if qlen > 16:
                    assert kern.startswith(f"tile f16 pair R=32 W={(qlen + 31) // 32} segs=1"), kern
                _check(got, b.want(q, REF), kern, qlen, L, n)


def test_all_n_and_short_batches(monkeypatch):
    """100 % N targets and queries (nothing ever rises above a frame's floor) and 1 % N."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    rng = np.random.default_rng(5)
    q = O.random_codes(9, 100, 4)
    seqs = [np.full(int(L), 4, np.uint8) for L in rng.integers(1, 151, 300)]
    seqs += _targets(rng, q, 300, rng.integers(1, 151, 300))
    b = _Batch(torch, seqs)
    for query in (q, np.full(100, 4, np.uint8)):
        with S.ScoreBank() as bank:
            bank.set_penalties(*REF)
            bank.load_query(query)
            (got,) = b.score(torch, bank)
            kern = bank.last_kernel()
        assert " skew" in kern, kern
        _check(got, b.want(query, REF), kern)


def _ab(torch, monkeypatch, q, b, pens=REF):
    """(scores of two back-to-back calls with the skewed rows, scores without, kernels)"""
    out = []
    for skew in ("1", "0"):
        monkeypatch.setenv("SWBANK_SKEW", skew)
        with S.ScoreBank() as bank:
            bank.set_penalties(*pens)
            bank.load_query(q)
            got = b.score(torch, bank, calls=2)
            out.append((got, bank.last_kernel(), bank.counters()))
    return out


def test_balanced_uniform(poisoned_buffers, monkeypatch):
    """The smallest uniform batch that runs balanced chunk ranges (two tiles per resident slot
    and one more): tiles cut at any chunk resume in their frames in another workgroup."""
    torch = pytest.importorskip("torch")
    qlen, L = 128, 124  # (16 chunks, the last one partial)
    n = 2 * SLOTS * 128 + 1
    q = O.random_codes(77, qlen, 4)
    res = O.random_codes(78, n * L, 4)
    rng = np.random.default_rng(3)
    for k in rng.choice(n, n // 20, replace=False):  # homologous: live values at every cut
        res[k * L:(k + 1) * L] = np.resize(np.roll(q, -int(rng.integers(0, 60))), L)
    res[rng.choice(res.size, res.size // 100, replace=False)] = 4
    b = _Batch(torch, packed=(res, np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32)))
    ((a1, a2), kern, ctr), ((b1, b2), kern0, _) = _ab(torch, monkeypatch, q, b)
    assert " skew" in kern and "balanced grid=" in kern and " skew" not in kern0, (kern, kern0)
    assert "balanced grid=" in kern0
    assert ctr["balanced_calls"] == 2 and ctr["balanced_timeouts"] == 0, ctr
    assert np.array_equal(a1, b1) and np.array_equal(a2, b1) and np.array_equal(b2, b1)
    rows = np.unique(np.concatenate([rng.choice(n, 20_000, replace=False), np.arange(300),
                                     np.arange(n - 300, n)]))
    _check(a1[rows], b.want(q, REF, rows), kern)
    assert a1.max() >= 5 * L - 40  # (the top of the range is reached)


def test_balanced_ragged_trimmed(poisoned_buffers, monkeypatch):
    """The smallest ragged batch ([64, 150] bp) the device sort plans as balanced ranges: the
    trimmed kernel, a tile's last chunk ending at any column."""
    torch = pytest.importorskip("torch")
    lo, hi, qlen = 64, 150, 128
    n = (2 * SLOTS * 19 // 8 + 4) * 128  # tiles x 8 chunks >= 2 x slots x 19 chunks
    rng = np.random.default_rng(11)
    q = O.random_codes(91, qlen, 4)
    lens = rng.integers(lo, hi + 1, n).astype(np.uint32)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    res = O.random_codes(92, int(lens.sum(dtype=np.uint64)), 4)
    res[rng.choice(res.size, res.size // 100, replace=False)] = 4
    for k in rng.choice(n, n // 25, replace=False):
        res[int(offs[k]):int(offs[k]) + int(lens[k])] = np.resize(q, int(lens[k]))
    b = _Batch(torch, packed=(res, offs, lens))
    ((a1, a2), kern, ctr), ((b1, _), kern0, _) = _ab(torch, monkeypatch, q, b)
    assert " skew" in kern and "dsort" in kern and "balanced grid=" in kern, kern
    assert " skew" not in kern0 and "balanced grid=" in kern0, kern0
    assert ctr["balanced_calls"] == 2 and ctr["balanced_timeouts"] == 0, ctr
    assert np.array_equal(a1, b1) and np.array_equal(a2, b1)
    rows = np.unique(np.concatenate([rng.choice(n, 20_000, replace=False), np.arange(300),
                                     np.arange(n - 300, n)]))
    _check(a1[rows], b.want(q, REF, rows), kern)


def _cols(L):
    """Columns the plain and balanced kernels run for L-bp targets: whole 8-column chunks."""
    return (L + 7) // 8 * 8


@pytest.mark.parametrize("qlen,L,skew", [(128, 216, True), (128, 217, False), (128, 222, False),
                                         (100, 249, True), (100, 250, True), (100, 252, True),
                                         (100, 256, True), (100, 257, False)])
def test_bound_edge(qlen, L, skew, monkeypatch):
    """5 / -4 / -12 / -4: the skewed rows run while 5 min(|q|, L) + 5 + 4 (128 + cols) <= 2048,
    cols = L rounded up to the chunk, since the untrimmed kernels carry the frames and the best
    through the last chunk's padding.  128 rows: up to L = 216 and not at 217; 100 rows: up to
    256, at lengths that leave 4-7 pad columns too, and not at 257, where the bare length would
    still pass (2,045) but the best of a 99-match hit would reach 2,051 and round.  Hits of
    near-maximal odd and even scores end in the last wave at the last real column."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    rng = np.random.default_rng(L)
    q = O.random_codes(12, qlen, 4)
    assert (5 * min(qlen, L) + 5 + 4 * (128 + _cols(L)) <= 2048) == skew
    seqs = _targets(rng, q, 500, np.full(500, L))
    for k in range(300):  # the query's last 85..100 % at the target's end
        t = rng.integers(0, 4, L).astype(np.uint8)
        hit = qlen - k % 16
        t[L - hit:] = q[qlen - hit:]
        seqs.append(t)
    b = _Batch(torch, seqs)
    with S.ScoreBank() as bank:
        bank.set_penalties(*REF)
        bank.load_query(q)
        (got,) = b.score(torch, bank)
        kern = bank.last_kernel()
    assert kern.startswith("tile f16 pair R=32 W=4 segs=1") and (" skew" in kern) == skew, kern
    want = b.want(q, REF)
    _check(got, want, kern, qlen, L)
    assert want.max() == 5 * qlen and (want == 5 * qlen - 5).any()  # (even and odd top scores)


@pytest.mark.parametrize("pens,qlen,L", [((5, -4, -20, -1), 128, 150), ((5, -4, -40, -1), 100, 150),
                                         ((2, -3, -16, -8), 64, 100), ((4, -6, -30, -8), 33, 60),
                                         ((1, -1, -2, -2), 127, 149)])
def test_penalties(pens, qlen, L, monkeypatch):
    """e = 1 and e = 8, larger opens: the offsets furthest from those of 5 / -4 / -12 / -4."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    rng = np.random.default_rng(qlen + L)
    q = O.random_codes(33 + qlen, qlen, 4)
    rows = (qlen + 31) // 32 * 32
    assert max(pens[0], 0) * (min(qlen, L) + 1) - pens[3] * (rows + _cols(L)) <= 2048
    lens = np.concatenate([np.full(400, L), rng.integers(1, L + 1, 400)])
    b = _Batch(torch, _targets(rng, q, 800, lens))
    with S.ScoreBank() as bank:
        bank.set_penalties(*pens)
        bank.load_query(q)
        (got,) = b.score(torch, bank)
        kern = bank.last_kernel()
    assert kern.startswith("tile f16 pair R=32") and " skew" in kern, kern
    _check(got, b.want(q, pens), kern, pens)
