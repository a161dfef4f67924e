"""The global-local search on the GPU (include/swbank.h "global-local search").
Every test compares sw_score_glocal[_device] exactly -- scores, end positions and strands -- with
the C model of tests/glocal_cases.py (itself checked against the plain-Python restatement of the
definition by tests/test_glocal_cases.py), with poisoned device buffers: the lane seams of the
kernel's three row counts and the targets' edges in all three modes on one strand and on both,
scores that no floor may touch, the boundary column, planted gaps across lane and block seams,
an asymmetric matrix, the penalty envelope and the range rule, one long target among short ones,
query sets, the chains into top_hits_device and best_queries_device, the host form, a multi-device
bank, the bookkeeping and the refusals.  The CPU references are computed once per process."""
import ctypes

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import fshift_envelope_cases as E
import glocal_cases as G
import seam_cases as SEAMS
import set_cases as SETS
import strand_cases as SC
import top_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_buffers")]

FILL = 0x3C
FILL32 = 0x3C3C3C3C
QLENS = sorted({1, 2, 3} | {64 * k + d for k in G.ROWS for d in (-1, 0, 1)} - {1025} | {1024})
EDGE_LENS = [0, 1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 194, 195, 1021]
SETS3 = {"dna": ("dna", G.DNA_PEN), "blosum62": ("blosum62", G.PROT_PEN)}


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


class Batch:
    """A packed batch on the device: (residues, offsets, lengths) as given, or packed from a list
    of code arrays."""

    def __init__(self, seqs=None, packed=None):
        if packed is None:
            res, offs, lens = S.pack_targets([np.asarray(s, np.uint8) for s in seqs])
        else:
            res, offs, lens = packed
        self.res, self.offs, self.lens = res, offs, lens
        self.n = len(lens)
        self.max_len = int(lens.max())
        self.d_res, self.d_offs, self.d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)

    def ptrs(self):
        return self.d_res.data_ptr(), self.d_offs.data_ptr(), self.d_lens.data_ptr()


def _bank(matrix="dna", pen=G.DNA_PEN, **kw):
    sub = SEAMS.MATRICES[matrix]() if isinstance(matrix, str) else matrix
    alphabet = S.ALPHABET_PROTEIN if sub.shape[0] == 24 else S.ALPHABET_DNA
    bank = S.ScoreBank(alphabet=alphabet, gap_model=O.GAP_GOTOH, **kw)
    bank.set_matrix(sub, *pen)
    return bank


def _live():
    f = S.lib().swbank_live_buffers
    f.restype = ctypes.c_long
    f.argtypes = []
    return int(f())


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _score_device(bank, bt, nq, ends, both, want_ends=True, want_strands=True, stream=0,
                  max_len=None):
    """(scores, end positions, strands) [nq, n] of the device form, every output poisoned first,
    and what last_kernel reported."""
    torch = _torch()
    dev = torch.device("cuda", 0)
    d_sc = torch.full((nq * bt.n,), FILL32, dtype=torch.int32, device=dev)
    d_ep = torch.full((nq * bt.n,), FILL32, dtype=torch.int32, device=dev)
    d_sd = _filled(nq * bt.n)
    torch.cuda.synchronize()
    bank.score_glocal_device(*bt.ptrs(), bt.n, bt.max_len if max_len is None else max_len, ends,
                             d_sc.data_ptr(), d_end_pos=d_ep.data_ptr() if want_ends else 0,
                             d_strands=d_sd.data_ptr() if want_strands else 0, both_strands=both,
                             stream=stream)
    name = bank.last_kernel()
    bank.sync()
    return (d_sc.cpu().numpy().reshape(nq, bt.n),
            d_ep.cpu().numpy().view(np.uint32).reshape(nq, bt.n),
            d_sd.cpu().numpy().reshape(nq, bt.n)), name


def _same(got, want, what):
    for g, w, part in zip(got, want, ("scores", "ends", "strands")):
        g, w = np.asarray(g), np.asarray(w)
        bad = np.nonzero(g != w)
        assert bad[0].size == 0, (what, part, [b[:8] for b in bad], g[bad][:8], w[bad][:8])


def _check(bank, bt, want, ends, both, what, nq=1):
    got, name = _score_device(bank, bt, nq, ends, both)
    assert name == f"glocal ends={ends} nq={nq} n={bt.n}"
    _same(got, want if nq > 1 else [w[None] for w in want], what)
    return got


# ---- 1. lane seams and target edges -------------------------------------------------------------
def _gapped_batch(n, pool, q, alpha, seed):
    """n targets whose lengths walk through the pool, at odd byte offsets, each followed by 1-3
    guard bytes of the alphabet's last code: windows of q (on either strand for DNA) with a
    substitution, an insertion or a deletion in random flanks, cut to length, and random targets
    (N in some).  (residues, offsets, lengths)."""
    rng = np.random.default_rng([251, n, len(q), seed])
    letters = 4 if alpha == 5 else 20
    guard_code = alpha - 1
    lens = np.array([pool[(5 * k + 3) % len(pool)] for k in range(n)], np.uint32)
    offs = np.zeros(n, np.int64)
    parts, pos = [], 0
    for k in range(n):
        guard = int(rng.integers(1, 4))
        guard += (pos + guard + 1) % 2  # every start is odd
        L = int(lens[k])
        t = rng.integers(0, letters, L).astype(np.uint8)
        if k % 3 and L >= 2:
            w = min(len(q), L, int(rng.integers(2, 200)))
            a = len(q) - w if k % 2 else int(rng.integers(0, len(q) - w + 1))
            core = q[a:a + w].copy()
            if k % 5 == 1 and w > 8:
                core = np.delete(core, [w // 2, w // 2 + 1])
            elif k % 5 == 2 and w > 8:
                core = np.insert(core, w // 2, rng.integers(0, letters, 2))
            core = core[:L]
            at = 0 if k % 4 == 0 else L - len(core) if k % 4 == 1 else \
                int(rng.integers(0, L - len(core) + 1))
            t[at:at + len(core)] = core
            if alpha == 5 and k % 7 >= 4:
                t = SC.revcomp(t)
        if k % 6 == 0 and L:
            t[rng.integers(0, L, 1 + L // 40)] = guard_code
        parts += [np.full(guard, guard_code, np.uint8), t]
        offs[k] = pos + guard
        pos += guard + L
    res = np.concatenate(parts + [np.full(3, guard_code, np.uint8)])
    assert (offs % 2 == 1).all()
    return res, offs.astype(np.uint64), lens


def _shape_case(name, m):
    def make():
        matrix, pen = SETS3[name]
        sub = SEAMS.MATRICES[matrix]()
        alpha = sub.shape[0]
        rng = np.random.default_rng([257, m, alpha])
        q = rng.integers(0, 4 if alpha == 5 else 20, m).astype(np.uint8)
        packed = _gapped_batch(64, EDGE_LENS, q, alpha, 0)
        want = {(e, b): G.c_search_packed(q, *packed, sub, *pen, e, b)
                for e in G.MODES for b in ((False, True) if alpha == 5 else (False,))}
        return q, packed, want
    return _cached(("shape", name, m), make)


@pytest.mark.parametrize("ends", G.MODES)
@pytest.mark.parametrize("name", list(SETS3))
def test_lane_seams_and_target_edges(name, ends):
    """Queries of 1, 2, 3 rows, each side of 256, 512 and 1,024 rows (64 lanes of each rows-per-
    lane count; swk_glocal_rows changes at 257 and 513) and SW_GLOCAL_MAX_QUERY, against 64
    targets of 0..3, 62..66, 127..129, 191..195 and 1,021 codes at odd offsets between guard
    bytes; DNA 5 / -4 at -12 / -4 on one strand and on both, BLOSUM62 at -11 / -1."""
    rows = S.lib().swk_glocal_rows
    assert [rows(m) for m in (255, 256, 257, 511, 512, 513, 1023, 1024)] == [4, 4, 8, 8, 8, 16, 16, 16]
    assert S.GLOCAL_MAX_QUERY == 1024
    assert {1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024} == set(QLENS)
    matrix, pen = SETS3[name]
    with _bank(matrix, pen) as bank:
        for m in QLENS:
            q, packed, want = _shape_case(name, m)
            assert set(EDGE_LENS) == set(packed[2].tolist())
            bt = _cached(("shape-batch", name, m), lambda: Batch(packed=packed))
            bank.load_query(q)
            for both in ((False, True) if name == "dna" else (False,)):
                got = _check(bank, bt, want[ends, both], ends, both, (name, m, ends, both))
                if not both:
                    assert not got[2].any()  # d_strands without both_strands is written 0
            assert np.array_equal(bt.d_res.cpu().numpy(), packed[0])  # the input is left alone
    q, packed, want = _shape_case(name, 257)
    sc, ep, sd = want[ends, name == "dna"]
    assert (sc < 0).any() and len(set(sc.tolist())) >= 16
    if ends == G.BOTH:
        assert (ep == G.END_NONE).all()
    else:
        assert (ep[packed[2] == 0] == G.END_NONE).all() and (ep != G.END_NONE).sum() >= 16
    if name == "dna":
        assert sd.any() and not sd.all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_sizes_and_the_host_form(n):
    pool = EDGE_LENS[13:] + EDGE_LENS[:13] if n == 1 else EDGE_LENS  # (n = 1: one 195-code target)
    q = np.random.default_rng(263).integers(0, 4, 23).astype(np.uint8)
    packed = _gapped_batch(n, pool, q, 5, 1)
    q2 = np.random.default_rng(264).integers(0, 4, 41).astype(np.uint8)
    bt = Batch(packed=packed)
    with _bank() as bank:
        for ends in G.MODES:
            # strands on: a workgroup per target; strands off: a workgroup per two targets, whose
            # second wave stands down behind the last target of an odd batch
            for both in (True, False):
                bank.load_query(q)
                want = _cached(("sizes", n, ends, both), lambda: G.c_search_packed(
                    q, *packed, G.dna(), *G.DNA_PEN, ends, both))
                _check(bank, bt, want, ends, both, (n, ends, both))
                _same(bank.score_glocal(packed, ends, both_strands=both), want,
                      (n, ends, both, "host"))
                # a query set: what a wave stores past the batch's last target would land in the
                # next query's row of the exactly sized, poisoned outputs
                bank.load_queries([q, q2])
                want2 = _cached(("sizes-set", n, ends, both), lambda: tuple(
                    np.stack(p) for p in zip(want, G.c_search_packed(
                        q2, *packed, G.dna(), *G.DNA_PEN, ends, both))))
                _check(bank, bt, want2, ends, both, (n, ends, both, "set"), nq=2)


# ---- 2. no floor ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ends", [G.QUERY, G.BOTH])
def test_no_floor(ends):
    """300 rows against at most 60 columns: at most 60 matches and at least 240 query residues
    against gaps, so every score is at most 5 x 60 - 16 - 4 x 239 < 0."""
    rng = np.random.default_rng(269)
    q = rng.integers(0, 4, 300).astype(np.uint8)
    seqs = [q[a:a + L].copy() if k % 2 else rng.integers(0, 4, L).astype(np.uint8)
            for k, (a, L) in enumerate(zip(rng.integers(0, 240, 40), rng.integers(0, 61, 40)))]
    seqs[3] = SC.revcomp(q[100:160])
    want = G.c_search(q, seqs, G.dna(), *G.DNA_PEN, ends, True)
    assert want[0].max() <= 5 * 60 - 16 - 4 * 239 < 0
    with _bank() as bank:
        bank.load_query(q)
        got = _check(bank, Batch(seqs), want, ends, True, ends)
    assert got[0].max() <= 5 * 60 - 16 - 4 * 239 and int(got[2][0][3]) == 1


# ---- 3. the boundary column ---------------------------------------------------------------------
def _boundary_case(m):
    rng = np.random.default_rng([271, m])
    q = G._codes(rng, m)
    h = m // 2
    begins = [np.concatenate([q[h:], rng.integers(0, 4, f)]).astype(np.uint8) for f in (0, 1, 5)]
    ends_ = [np.concatenate([rng.integers(0, 4, f), q[:h]]).astype(np.uint8) for f in (0, 1, 5)]
    return q, begins + ends_ + [SC.revcomp(t) for t in begins + ends_]


@pytest.mark.parametrize("m", [8, 12, 16, 24, 32, 48, 300, 700])
def test_boundary_column(m):
    """Targets that begin with the query's second half, and targets that end with its first half:
    the other half pays o + i e from the boundary column (or as a closing run of gaps), held by
    lanes that have not reached their first column.  8 to 48 rows run the 4-row kernel over 2 to
    12 lanes (the boundary spans 1 to 6 of them); 300 and 700 rows run the 8- and 16-row kernels,
    where it spans 19 and 22 lanes."""
    q, seqs = _boundary_case(m)
    h = m // 2
    bt = Batch(seqs)
    with _bank() as bank:
        bank.load_query(q)
        for ends in G.MODES:
            want = G.c_search(q, seqs, G.dna(), *G.DNA_PEN, ends, True)
            if ends == G.QUERY:
                # no end lies past the query's length here (SW_END_NONE aside)
                assert (want[1][want[1] != G.END_NONE] <= m).all()
                if m >= 300:  # the half is worth its gap: the score is the arithmetic's
                    assert int(want[0][0]) == 5 * (m - h) - 16 - 4 * (h - 1)
                    assert int(want[1][0]) == m - h - 1
                    assert int(want[0][3]) == 5 * h - 16 - 4 * (m - h - 1)
            _check(bank, bt, want, ends, True, (m, ends))


# ---- 4. lane and block seams ----------------------------------------------------------------------
@pytest.mark.parametrize("K", G.ROWS)
def test_planted_gaps_across_lane_and_block_seams(K):
    """The plants of glocal_cases.seam_plants that test_glocal_cases found live: a kernel that
    loses F between two lanes, or E between two 64-column blocks, scores them differently."""
    q, plants = G.seam_plants(K)
    flags = G.live(q, plants, G.dna(), *G.DNA_PEN)
    kept = [t for (_, t, _), f in zip(plants, flags) if f]
    assert len(kept) >= 6
    bt = Batch(kept)
    with _bank() as bank:
        bank.load_query(q)
        assert S.lib().swk_glocal_rows(len(q)) == K
        for ends in G.MODES:
            want = G.c_search(q, kept, G.dna(), *G.DNA_PEN, ends, True)
            _check(bank, bt, want, ends, True, (K, ends))
    assert want[2].any() and not want[2].all()


# ---- 5. an asymmetric matrix ----------------------------------------------------------------------
@pytest.mark.parametrize("ends", G.MODES)
def test_asymmetric_matrix(ends):
    """asym-pair at -12 / -4: the transposed matrix changes most of the model's scores, so a
    kernel reading s(t, q) cannot pass; asym-prot on a protein bank likewise."""
    q, seqs = G.asym_case()
    sub = SEAMS.MATRICES[G.ASYM]()
    assert G.transposed_share(q, seqs, sub, *G.ASYM_PEN, ends, True) > 0.5
    with _bank(G.ASYM, G.ASYM_PEN) as bank:
        bank.load_query(q)
        _check(bank, Batch(seqs), G.c_search(q, seqs, sub, *G.ASYM_PEN, ends, True), ends, True, ends)
    rng = np.random.default_rng(277)
    pq = rng.integers(0, 24, 90).astype(np.uint8)
    pseqs = [np.concatenate([rng.integers(0, 24, 5), pq[a:a + 40], rng.integers(0, 24, 4)])
             .astype(np.uint8) for a in range(0, 48, 3)]
    psub = SEAMS.MATRICES["asym-prot"]()
    assert G.transposed_share(pq, pseqs, psub, *G.PROT_PEN, ends, False) > 0.5
    with _bank("asym-prot", G.PROT_PEN) as bank:
        bank.load_query(pq)
        _check(bank, Batch(pseqs), G.c_search(pq, pseqs, psub, *G.PROT_PEN, ends, False), ends,
               False, (ends, "protein"))


# ---- 6. the penalty envelope and the range rule ---------------------------------------------------
@pytest.mark.parametrize("pen", G.ENVELOPE)
def test_penalty_envelope(pen):
    q, seqs = G.asym_case()
    rng = np.random.default_rng(281)
    q2 = rng.integers(0, 4, 300).astype(np.uint8)
    seqs2 = seqs[:12] + [q2[20:280], SC.revcomp(np.delete(q2, np.arange(100, 130)))]
    for qq, ss in ((q, seqs), (q2, seqs2)):
        bt = Batch(ss)
        with _bank("dna", pen) as bank:
            bank.load_query(qq)
            for ends in G.MODES:
                _check(bank, bt, G.c_search(qq, ss, G.dna(), *pen, ends, True), ends, True,
                       (pen, len(qq), ends))


def test_range_rule():
    """e = -32757: |o| + (1,024 + 64 + max_len) x |e| reaches 2^30 at max_len = 40,000 (refused,
    nothing written) and not at 1,000 (exact)."""
    pen = (0, -32757)
    assert 32757 + (1024 + 64 + 40000) * 32757 >= 1 << 30 > 32757 + (1024 + 64 + 1000) * 32757
    rng = np.random.default_rng(283)
    q = rng.integers(0, 4, 150).astype(np.uint8)
    seqs = [rng.integers(0, 4, L).astype(np.uint8) for L in (0, 1, 150, 999, 1000)] + [q[10:140]]
    bt = Batch(seqs)
    with _bank("dna", pen) as bank:
        bank.load_query(q)
        for ends in G.MODES:
            with pytest.raises(S.SwbankError) as ei:
                _score_device(bank, bt, 1, ends, True, max_len=40000)
            assert ei.value.status == S.ERR_RANGE
            want = G.c_search(q, seqs, G.dna(), *pen, ends, True)
            _check(bank, bt, want, ends, True, ends)
        torch = _torch()
        d = torch.full((bt.n * 3,), FILL32, dtype=torch.int32, device=torch.device("cuda", 0))
        p = d.data_ptr()
        with pytest.raises(S.SwbankError):
            bank.score_glocal_device(*bt.ptrs(), bt.n, 40000, G.QUERY, p, d_end_pos=p + 4 * bt.n,
                                     d_strands=p + 8 * bt.n)
        bank.sync()
        assert (d.cpu().numpy() == FILL32).all()  # no write
        long = [np.zeros(40000, np.uint8)]  # the host form takes the longest listed target
        with pytest.raises(S.SwbankError) as ei:
            bank.score_glocal(long, G.QUERY)
        assert ei.value.status == S.ERR_RANGE
        assert _c_host_call(bank, Batch(long), 1, G.QUERY, True) == (S.ERR_RANGE, True)
        _same(bank.score_glocal(seqs, G.BOTH, both_strands=True), want, "host")


# ---- 7. one long target among short ones ------------------------------------------------------------
@pytest.mark.parametrize("ends", G.MODES)
def test_one_long_target_among_short_ones(ends):
    """A 70,000-nt target (one workgroup walks it) and its reverse complement in a batch of 100-nt
    ones, the query planted near its far end."""
    rng = np.random.default_rng(293)
    q = rng.integers(0, 4, 40).astype(np.uint8)
    seqs = [rng.integers(0, 4, 100).astype(np.uint8) for _ in range(66)]
    long = rng.integers(0, 4, 70000).astype(np.uint8)
    long[69001:69041] = q
    seqs[17] = long
    seqs[40] = SC.revcomp(long)
    want = _cached(("long", ends), lambda: G.c_search(q, seqs, G.dna(), *G.DNA_PEN, ends, True))
    with _bank() as bank:
        bank.load_query(q)
        got = _check(bank, Batch(seqs), want, ends, True, ends)
        _same(bank.score_glocal(seqs, ends, both_strands=True), want, "host")
    if ends == G.QUERY:
        assert got[0][0][[17, 40]].tolist() == [200, 200]
        assert got[1][0][[17, 40]].tolist() == [69040, 70000 - 1 - 69040]
        assert got[2][0][[17, 40]].tolist() == [0, 1]


# ---- 8. query sets, NULL outputs, bookkeeping -------------------------------------------------------
def _set_case():
    def make():
        rng = np.random.default_rng(307)
        qs = [rng.integers(0, 4, m).astype(np.uint8) for m in (17, 130, 300)]
        seqs = []
        for k in range(70):
            q = qs[k % 3]
            if k % 5 == 4:
                seqs.append(rng.integers(0, 5, int(rng.integers(0, 200))).astype(np.uint8))
                continue
            t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 12))),
                                np.delete(q, len(q) // 2) if k % 2 else q,
                                rng.integers(0, 4, int(rng.integers(0, 12)))]).astype(np.uint8)
            seqs.append(SC.revcomp(t) if k % 4 >= 2 else t)
        return qs, seqs, {e: G.c_search_set(qs, seqs, G.dna(), *G.DNA_PEN, e, True) for e in G.MODES}
    return _cached("set", make)


def test_query_set_null_outputs_and_bookkeeping():
    qs, seqs, want = _set_case()
    bt = Batch(seqs)
    base = _live()
    with _bank() as bank:
        bank.load_queries(qs)
        for ends in G.MODES:
            got = _check(bank, bt, want[ends], ends, True, ends, nq=3)
            _same(bank.score_glocal((bt.res, bt.offs, bt.lens), ends, both_strands=True), got,
                  (ends, "host"))
        got2, _ = _score_device(bank, bt, 3, G.QUERY, True, want_ends=False, want_strands=False)
        assert np.array_equal(got2[0], want[G.QUERY][0])
        assert (got2[1] == FILL32).all() and (got2[2] == FILL).all()  # NULL outputs: not written
        with pytest.raises(S.SwbankError) as ei:  # no best hit is tracked
            bank.best()
        assert ei.value.status == S.ERR_STATE
        bank.load_query(qs[1])
        _same(bank.score_glocal(seqs, G.TARGET, both_strands=True),
              [w[1] for w in want[G.TARGET]], "one query")
        bank.score_glocal_device(*bt.ptrs(), 0, bt.max_len, G.QUERY, 0)  # an empty batch is fine
        sc, ep, sd = bank.score_glocal([], G.QUERY)
        assert sc.shape == ep.shape == sd.shape == (0,)
        bank.set_timing(True)
        _score_device(bank, bt, 1, G.QUERY, True)
        launches, _, ms = bank.timing()
        assert launches == 1 and ms > 0  # one timing bracket
    assert _live() == base  # the live-buffer count returns to its baseline


def test_multi_device_bank():
    qs, seqs, want = _set_case()
    bt = Batch(seqs)
    with _bank(devices=[0, 0]) as bank:
        bank.load_query(qs[1])
        for ends in G.MODES:
            _check(bank, bt, [w[1] for w in want[ends]], ends, True, ends)
            _same(bank.score_glocal(seqs, ends, both_strands=True), [w[1] for w in want[ends]],
                  (ends, "host"))


# ---- 9. the chains ----------------------------------------------------------------------------------
def test_chains_into_top_hits_and_best_queries_on_one_stream():
    """score_glocal_device -> top_hits_device and -> best_queries_device on one stream with no
    host step; BOTH mode, where most scores are negative."""
    torch = _torch()
    qs, seqs, want = _set_case()
    w = want[G.BOTH]
    assert (w[0] < 0).mean() > 0.5 and (w[0] > 0).any()
    bt = Batch(seqs)
    k, nq, dev = 32, 3, torch.device("cuda", 0)  # (deep enough to list negative scores)
    stream = torch.cuda.Stream()
    with _bank() as bank:
        bank.load_queries(qs)
        d_sc = torch.full((nq * bt.n,), FILL32, dtype=torch.int32, device=dev)
        d_hits = _filled(nq * k * 8)
        d_hsc = torch.zeros(nq * k, dtype=torch.int32, device=dev)
        d_bq = torch.full((bt.n,), FILL32, dtype=torch.int32, device=dev)
        d_bs = torch.full((bt.n,), FILL32, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_glocal_device(*bt.ptrs(), bt.n, bt.max_len, G.BOTH, d_sc.data_ptr(),
                                 both_strands=True, stream=h)
        bank.top_hits_device(d_sc.data_ptr(), bt.n, k, d_hits.data_ptr(), nq=nq,
                             d_hit_scores=d_hsc.data_ptr(), stream=h)
        bank.best_queries_device(d_sc.data_ptr(), bt.n, nq, d_best_query=d_bq.data_ptr(),
                                 d_best_score=d_bs.data_ptr(), stream=h)
        bank.sync()
        stream.synchronize()
    whits, wsc, _ = TC.ref_top(w[0], k)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint64).reshape(nq, k), whits)
    assert np.array_equal(d_hsc.cpu().numpy().reshape(nq, k), wsc) and (wsc < 0).any()
    wq, ws = SETS.ref_best(w[0])
    assert np.array_equal(d_bq.cpu().numpy().view(np.uint32), wq)
    assert np.array_equal(d_bs.cpu().numpy(), ws) and (ws < 0).any()


# ---- 10. refusals -----------------------------------------------------------------------------------
def test_refusals_in_the_headers_order():
    qs, seqs, _ = _set_case()
    bt = Batch(seqs[:8])
    host = (bt.res, bt.offs, bt.lens)
    torch = _torch()
    out = torch.full((1 << 10,), FILL32, dtype=torch.int32, device=torch.device("cuda", 0))
    p = out.data_ptr()

    def status(fn, *a, **kw):
        with pytest.raises(S.SwbankError) as ei:
            fn(*a, **kw)
        return ei.value.status

    def both_forms(bank, ends=G.QUERY, strands=False, batch=host):
        return {status(bank.score_glocal_device, *bt.ptrs(), bt.n, bt.max_len, ends, p,
                       d_end_pos=p + 1024, d_strands=p + 2048, both_strands=strands),
                status(bank.score_glocal, batch, ends, both_strands=strands)}

    pq = np.arange(20, dtype=np.uint8)
    # 1. both_strands on a protein bank comes first: merged gaps, a bad ends and no query behind it
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_MERGED) as bank:
        bank.set_matrix(O.BLOSUM62, *G.PROT_PEN)
        assert both_forms(bank, ends=0, strands=True) == {S.ERR_UNSUPPORTED}
        # 2. then the gap model, a bad ends and no query behind it
        assert both_forms(bank, ends=0) == {S.ERR_UNSUPPORTED}
        bank.load_query(pq)
        assert both_forms(bank) == {S.ERR_UNSUPPORTED}
    with S.ScoreBank(gap_model=O.GAP_MERGED) as bank:  # (a DNA bank)
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(qs[0])
        assert both_forms(bank, strands=True) == {S.ERR_UNSUPPORTED}
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH) as bank:
        bank.set_matrix(O.BLOSUM62, *G.PROT_PEN)
        bank.load_query(pq)
        assert both_forms(bank, strands=True) == {S.ERR_UNSUPPORTED}
        sc, ep, sd = bank.score_glocal(host, G.QUERY)  # (codes 0..4 are protein codes too)
        assert sc.shape == (8,) and not sd.any()
    with S.ScoreBank(gap_model=O.GAP_GOTOH) as bank:
        # 3. ends, no query behind it;  4. the state
        for bad in (0, 4, -1):
            assert both_forms(bank, ends=bad) == {S.ERR_ARG}
        assert both_forms(bank) == {S.ERR_STATE}
        bank.set_penalties(5, -4, -12, -4)
        assert both_forms(bank) == {S.ERR_STATE}
        # 5. the query length, NULL buffers behind it
        rng = np.random.default_rng(311)
        bank.load_query(rng.integers(0, 4, S.GLOCAL_MAX_QUERY + 1).astype(np.uint8))
        assert both_forms(bank) == {S.ERR_UNSUPPORTED}
        assert status(bank.score_glocal_device, 0, 0, 0, bt.n, bt.max_len, G.QUERY, 0) == S.ERR_UNSUPPORTED
        bank.load_queries([qs[0], rng.integers(0, 4, S.GLOCAL_MAX_QUERY + 1).astype(np.uint8)])
        assert both_forms(bank) == {S.ERR_UNSUPPORTED}  # any query of the set
        bank.load_query(qs[0])
        # the argument checks
        assert status(bank.score_glocal_device, *bt.ptrs(), bt.n, bt.max_len, G.QUERY, 0) == S.ERR_ARG
        assert status(bank.score_glocal_device, 0, bt.d_offs.data_ptr(), bt.d_lens.data_ptr(),
                      bt.n, bt.max_len, G.QUERY, p) == S.ERR_ARG
        assert status(bank.score_glocal_device, bt.d_res.data_ptr(), 0, bt.d_lens.data_ptr(),
                      bt.n, bt.max_len, G.QUERY, p) == S.ERR_ARG
        assert status(bank.score_glocal_device, bt.d_res.data_ptr(), bt.d_offs.data_ptr(), 0,
                      bt.n, bt.max_len, G.QUERY, p) == S.ERR_ARG
        bad = bt.res.copy()
        bad[int(bt.offs[5]) + 1] = 5  # a host code outside the alphabet
        assert status(bank.score_glocal, (bad, bt.offs, bt.lens), G.QUERY) == S.ERR_ARG
        outside = bt.lens.copy()
        outside[7] += len(bt.res)  # a target outside the buffer
        assert status(bank.score_glocal, (bt.res, bt.offs, outside), G.QUERY) == S.ERR_ARG
        bank.sync()
        assert (out.cpu().numpy() == FILL32).all()  # every refusal left the outputs alone
        sc, ep, sd = bank.score_glocal(host, G.TARGET)  # and the bank usable
        assert sc.shape == (8,)


def _c_host_call(bank, bt, n, ends, both):
    """sw_score_glocal through the C entry itself with poisoned host outputs: (status, untouched)."""
    L, P = S.lib(), G._p
    cells = max(bank.query_count(), 1) * bt.n
    sc = np.full(cells, FILL32, np.int32)
    ep = np.full(cells, FILL32, np.uint32)
    sd = np.full(cells, FILL, np.uint8)
    st = L.sw_score_glocal(bank._h, P(bt.res), bt.res.size, P(bt.offs), P(bt.lens), n, ends,
                           int(both), P(sc), P(ep), P(sd))
    return st, bool((sc == FILL32).all() and (ep == FILL32).all() and (sd == FILL).all())


def test_refusals_leave_the_host_outputs_alone_and_refuse_a_batch_of_2_to_the_32():
    """The host form's scores_out, end_pos_out and strands_out keep their fill after every kind of
    refusal (the opening checks, the argument checks, the staging's checks); n >= 2^32 is
    SW_ERR_ARG from both forms before anything is read or written.  (nq x n cannot overflow
    size_t with n < 2^32 unless a set of more than 2^30 queries is loaded; the check is there as
    in the frameshift entries, no test reaches it.)"""
    qs, seqs, _ = _set_case()
    bt = Batch(seqs[:9])
    torch = _torch()
    out = torch.full((3 * 2 * bt.n,), FILL32, dtype=torch.int32, device=torch.device("cuda", 0))
    p = out.data_ptr()
    with S.ScoreBank(gap_model=O.GAP_MERGED) as bank:
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(qs[0])
        assert _c_host_call(bank, bt, bt.n, G.QUERY, True) == (S.ERR_UNSUPPORTED, True)
    with S.ScoreBank(gap_model=O.GAP_GOTOH) as bank:
        assert _c_host_call(bank, bt, bt.n, G.QUERY, True) == (S.ERR_STATE, True)
        bank.set_penalties(5, -4, -12, -4)
        bank.load_queries(qs[:2])
        assert _c_host_call(bank, bt, bt.n, 0, True) == (S.ERR_ARG, True)
        for big in (1 << 32, (1 << 32) + 1):
            assert _c_host_call(bank, bt, big, G.QUERY, True) == (S.ERR_ARG, True)
            with pytest.raises(S.SwbankError) as ei:
                bank.score_glocal_device(*bt.ptrs(), big, bt.max_len, G.QUERY, p,
                                         d_end_pos=p + 8 * bt.n, d_strands=p + 16 * bt.n,
                                         both_strands=True)
            assert ei.value.status == S.ERR_ARG
        bad = Batch(packed=(bt.res.copy(), bt.offs, bt.lens))
        bad.res[int(bt.offs[8]) + 1] = 5  # the last target: everything before it was staged
        assert _c_host_call(bank, bad, bt.n, G.TARGET, True) == (S.ERR_ARG, True)
        far = Batch(packed=(bt.res, bt.offs, bt.lens.copy()))
        far.lens[8] += len(bt.res)
        assert _c_host_call(bank, far, bt.n, G.BOTH, False) == (S.ERR_ARG, True)
        rng = np.random.default_rng(337)
        bank.load_query(rng.integers(0, 4, S.GLOCAL_MAX_QUERY + 1).astype(np.uint8))
        assert _c_host_call(bank, bt, bt.n, G.QUERY, False) == (S.ERR_UNSUPPORTED, True)
        bank.sync()
        assert (out.cpu().numpy() == FILL32).all()
        bank.load_queries(qs[:2])
        st, untouched = _c_host_call(bank, bt, bt.n, G.QUERY, True)  # the bank stays usable
        assert st == 0 and not untouched


@pytest.mark.parametrize("which", [0, 1])
def test_the_banks_range_refusals_write_nothing(which):
    """A matrix of span 255 and Gotoh penalties with o + e + S = 65536 are refused with
    SW_ERR_RANGE by both forms, as by the frameshift entries (the call prepares the bank's query
    tables, which are built for the 16-bit kernels): after the opening checks, before anything is
    written, and the bank stays usable."""
    torch = _torch()
    case = E.REFUSED[which]
    rng = np.random.default_rng([347, which])
    q = rng.integers(0, 20, 33).astype(np.uint8)
    seqs = [rng.integers(0, 20, L).astype(np.uint8) for L in (0, 1, 33, 64, 65, 200)] + [q[3:30]]
    bt = Batch(seqs)
    n, dev = bt.n, torch.device("cuda", 0)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH) as bank:
        bank.set_matrix(E.matrix(case.matrix), case.go, case.ge)  # (loading it is accepted)
        bank.load_query(q)
        d_sc = torch.full((n,), FILL32, dtype=torch.int32, device=dev)
        d_ep = torch.full((n,), FILL32, dtype=torch.int32, device=dev)
        d_sd = _filled(n)
        torch.cuda.synchronize()
        for ends in G.MODES:
            with pytest.raises(S.SwbankError) as ei:
                bank.score_glocal_device(*bt.ptrs(), n, bt.max_len, ends, d_sc.data_ptr(),
                                         d_end_pos=d_ep.data_ptr(), d_strands=d_sd.data_ptr())
            assert ei.value.status == S.ERR_RANGE
            assert _c_host_call(bank, bt, n, ends, False) == (S.ERR_RANGE, True)
        # the opening checks come first
        assert _c_host_call(bank, bt, n, 4, False) == (S.ERR_ARG, True)
        assert _c_host_call(bank, bt, n, G.QUERY, True) == (S.ERR_UNSUPPORTED, True)
        bank.sync()
        torch.cuda.synchronize()
        assert (d_sc.cpu().numpy() == FILL32).all() and (d_ep.cpu().numpy() == FILL32).all()
        assert (d_sd.cpu().numpy() == FILL).all()
        assert np.array_equal(bt.d_res.cpu().numpy(), bt.res)
        # an accepted matrix and the bank scores again
        bank.set_matrix(O.BLOSUM62, *G.PROT_PEN)
        want = G.c_search(q, seqs, O.BLOSUM62, *G.PROT_PEN, G.QUERY)
        _check(bank, bt, want, G.QUERY, False, "after a refusal")
        _same(bank.score_glocal(seqs, G.QUERY), want, "host after a refusal")


def test_device_form_reads_a_code_past_the_alphabet_as_its_last_code():
    qs, seqs, _ = _set_case()
    res, offs, lens = S.pack_targets(seqs[:16])
    odd = res.copy()
    at = np.arange(7, len(res), 29)
    odd[at] = 5 + (at % 250)
    as_n = res.copy()
    as_n[at] = 4
    bt = Batch(packed=(odd, offs, lens))
    with _bank() as bank:
        bank.load_query(qs[2])
        for ends in G.MODES:
            want = G.c_search_packed(qs[2], as_n, offs, lens, G.dna(), *G.DNA_PEN, ends, True)
            _check(bank, bt, want, ends, True, ends)
    rng = np.random.default_rng(313)
    pq = rng.integers(0, 20, 50).astype(np.uint8)
    pres = rng.integers(0, 20, 400).astype(np.uint8)
    poffs, plens = np.arange(0, 400, 50, dtype=np.uint64), np.full(8, 50, np.uint32)
    podd = pres.copy()
    podd[::13] = 24 + (np.arange(0, 400, 13) % 200)
    as_stop = pres.copy()
    as_stop[::13] = 23
    with _bank("blosum62", G.PROT_PEN) as bank:
        bank.load_query(pq)
        want = G.c_search_packed(pq, as_stop, poffs, plens, O.BLOSUM62, *G.PROT_PEN, G.QUERY)
        _check(bank, Batch(packed=(podd, poffs, plens)), want, G.QUERY, False, "protein")
