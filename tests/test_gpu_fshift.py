"""The frameshift-tolerant translated search on the GPU (include/swbank.h "frameshift-tolerant
translated search").  Every test compares sw_score_fshift[_device] exactly with
the C model of tests/fshift_cases.py (itself checked against the plain-Python restatement of the
definition by tests/test_fshift_cases.py): the lane and block seams of the kernel's three row
counts, the targets' edges, one long target among short ones, the six-frame anchor at
fs = -32767, planted shifts, query sets, an asymmetric matrix, a custom table, scores past 16
bits, the chain into top_hits_device, leaks and the refusals.  The CPU references are computed
once per process and shared."""
import ctypes

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fshift_cases as FS
import matrix_cases as MC
import seam_cases as SEAMS
import top_cases as TC

pytestmark = pytest.mark.gpu

FILL = 0x3C
ROWS = (4, 8, 16)  # the kernel's rows per lane: queries of at most 256, 512 and 1,024 rows
QLENS = sorted({1, 2, 3} | {k + d for k in ROWS for d in (-1, 0, 1)} | {63, 64, 65} |
               {64 * k + d for k in ROWS for d in (-1, 0, 1)} - {1025} |
               {1023, 1024, S.FSHIFT_MAX_QUERY})
EDGE_LENS = list(range(10)) + [62, 63, 64, 65, 66, 191, 192, 193, 194, 195, 1021]


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
    """A packed DNA batch on the device: (residues, offsets, lengths) as given, or packed from a
    list of code arrays."""

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


def _bank(sub=O.BLOSUM62, pen=F.PEN, **kw):
    bank = S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH, **kw)
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


def _score_device(bank, bt, nq, fs, strands=True, table=None, stream=0):
    torch = _torch()
    dev = torch.device("cuda", 0)
    d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_sd = _filled(nq * bt.n)
    torch.cuda.synchronize()
    bank.score_frameshift_device(*bt.ptrs(), bt.n, bt.max_len, fs, d_sc.data_ptr(),
                                 d_strands=d_sd.data_ptr() if strands else 0, codon_table=table,
                                 stream=stream)
    name = bank.last_kernel()
    bank.sync()
    return d_sc.cpu().numpy().reshape(nq, bt.n), d_sd.cpu().numpy().reshape(nq, bt.n), name


def _same(got, want, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))
    assert bad[0].size == 0, (what, [b[:8] for b in bad], np.asarray(got)[bad][:8],
                              np.asarray(want)[bad][:8])


# ---- 1. lane and block seams ------------------------------------------------------------------------
def _seam_targets(q, seed):
    """64 DNA targets of 0..260 codes for query q: windows of q (anywhere, its last rows among
    them) back-translated with one base inserted or removed near the middle, on either strand, in
    random flanks; random targets, N codes in some; an empty and a codon-less one."""
    rng = np.random.default_rng([109, len(q), seed])
    seqs = []
    for k in range(64):
        if k % 4 == 3:
            seqs.append(rng.integers(0, 5 if k % 8 == 7 else 4, int(rng.integers(0, 261))).astype(np.uint8))
            continue
        ln = min(len(q), int(rng.integers(1, 61)))
        a = len(q) - ln if k % 8 == 0 else int(rng.integers(0, len(q) - ln + 1))
        core = F.back_translate(rng, q[a:a + ln])
        at = 3 * (ln // 2) + int(rng.integers(0, 3))
        if k % 3 == 0:
            core = np.insert(core, at, int(rng.integers(0, 4)))
        elif k % 3 == 1 and len(core) > 3:
            core = np.delete(core, at)
        left, right = (rng.integers(0, 4, int(rng.integers(0, 30))).astype(np.uint8) for _ in range(2))
        t = np.concatenate([left, core, right]).astype(np.uint8)
        seqs.append(F.SC.revcomp(t) if k % 2 else t)
    seqs[5], seqs[9] = np.zeros(0, np.uint8), np.array([1, 2], np.uint8)
    return seqs


def _seam_case(m):
    def make():
        rng = np.random.default_rng([113, m])
        q = rng.integers(0, 20, m).astype(np.uint8)
        seqs = _seam_targets(q, 0)
        return q, seqs, {fs: FS.c_search(q, seqs, O.BLOSUM62, *F.PEN, fs) for fs in (0, -7, -15, -32767)}
    return _cached(("seam", m), make)


@pytest.mark.parametrize("fs", [0, -7, -15, -32767])
def test_lane_and_block_seams(fs):
    """Queries of 1, 2, 3 rows, each side of 4, 8, 16 rows (a lane), of 64 rows, of 256, 512 and
    1,024 rows (64 lanes of each row count), and SW_FSHIFT_MAX_QUERY."""
    assert S.FSHIFT_MAX_QUERY == 1024 and {1, 5, 17, 65, 257, 513, 1023, 1024} <= set(QLENS)
    with _bank() as bank:
        for m in QLENS:
            q, seqs, want = _seam_case(m)
            bt = _cached(("seam-batch", m), lambda: Batch(seqs))
            bank.load_query(q)
            got, gsd, name = _score_device(bank, bt, 1, fs)
            assert name == f"fshift nq=1 n={bt.n}"
            _same(got[0], want[fs][0], (m, fs))
            _same(gsd[0], want[fs][1], (m, fs, "strands"))
    if fs == -15:  # the shifts are alive: dearer shifts lower scores, free ones raise them
        q, seqs, want = _seam_case(257)
        assert (want[-15][0] > want[-32767][0]).sum() >= 10
        assert (want[0][0] > want[-15][0]).sum() >= 10


# ---- 2. target edges --------------------------------------------------------------------------------
def _gapped_batch(n, pool):
    """n targets whose lengths walk through the pool, at odd byte offsets, each followed by 1-3
    guard bytes of code 4, N codes inside every third one: (residues, offsets, lengths)."""
    rng = np.random.default_rng([127, n, len(pool)])
    lens = np.array([pool[(5 * k + 3) % len(pool)] for k in range(n)], np.uint32)
    offs = np.zeros(n, np.int64)
    parts, pos = [], 0
    for k in range(n):
        guard = int(rng.integers(1, 4))
        guard += (pos + guard + 1) % 2  # every start is odd
        t = rng.integers(0, 4, int(lens[k])).astype(np.uint8)
        if k % 3 == 0 and len(t):
            t[rng.integers(0, len(t), 1 + len(t) // 40)] = 4
        parts += [np.full(guard, 4, np.uint8), t]
        offs[k] = pos + guard
        pos += guard + int(lens[k])
    res = np.concatenate(parts + [np.full(3, 4, np.uint8)])
    assert (offs % 2 == 1).all()
    return res, offs.astype(np.uint64), lens


@pytest.mark.parametrize("table", ["standard", "custom"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_target_edges(n, table):
    tab = F.custom_table() if table == "custom" else None
    pool = EDGE_LENS[16:] + EDGE_LENS[:16] if n == 1 else EDGE_LENS  # (n = 1: one 195-code target)
    res, offs, lens = _gapped_batch(n, pool)
    if n >= 63:
        assert set(EDGE_LENS) <= set(lens.tolist())
    q = np.random.default_rng(131).integers(0, 20, 23).astype(np.uint8)
    want = _cached(("edges", n, table),
                   lambda: FS.c_search_packed(q, res, offs, lens, O.BLOSUM62, *F.PEN, -7, tab))
    bt = Batch(packed=(res, offs, lens))
    with _bank() as bank:
        bank.load_query(q)
        got, gsd, _ = _score_device(bank, bt, 1, -7, table=tab)
        _same(got[0], want[0], "scores")
        _same(gsd[0], want[1], "strands")
        sc, sd = bank.score_frameshift((res, offs, lens), -7, codon_table=tab)
        _same(sc, want[0], "host scores")
        _same(sd, want[1], "host strands")
    assert np.array_equal(bt.d_res.cpu().numpy(), res)  # the input is left alone
    assert want[0].max() > 0 and (want[0][lens < 3] == 0).all()


# ---- 3. one long target among short ones ------------------------------------------------------------
def test_one_long_target_among_short_ones(poisoned_buffers):
    """A 70,000-nt target (23,333 codon indices on one workgroup) in a batch of 100-nt ones, the
    query planted with a shift near its far end, with poisoned device buffers."""
    rng = np.random.default_rng(137)
    q = rng.integers(0, 20, 40).astype(np.uint8)
    seqs = [rng.integers(0, 4, 100).astype(np.uint8) for _ in range(66)]
    long = rng.integers(0, 4, 70000).astype(np.uint8)
    core = np.insert(F.back_translate(rng, q), 60, 2)  # between codons 19 and 20
    long[69001:69001 + len(core)] = core
    seqs[17] = long
    seqs[40] = F.SC.revcomp(long)
    want = _cached("long", lambda: FS.c_search(q, seqs, O.BLOSUM62, *F.PEN, -15))
    bt = Batch(seqs)
    with _bank() as bank:
        bank.load_query(q)
        got, gsd, _ = _score_device(bank, bt, 1, -15)
        sc, sd = bank.score_frameshift(seqs, -15)
    _same(got[0], want[0], "scores")
    _same(gsd[0], want[1], "strands")
    _same(sc, want[0], "host scores")
    assert int(got[0][17]) == int(got[0][40]) >= F.self_score(q) - 15
    assert (int(gsd[0][17]), int(gsd[0][40])) == (0, 1)


# ---- 4. the six-frame anchor ------------------------------------------------------------------------
def test_anchor_equals_score_frames():
    """fs = -32767 can never win: the scores are those of score_frames on the same batch, the
    strands (frames >= 3)."""
    torch = _torch()
    qs, seqs, _ = F.search_case()
    bt = Batch(seqs)
    dev = torch.device("cuda", 0)
    with _bank() as bank:
        bank.load_queries(qs)
        d_sc = torch.zeros(3 * bt.n, dtype=torch.int32, device=dev)
        d_fr = _filled(3 * bt.n)
        bank.score_frames_device(*bt.ptrs(), bt.n, bt.max_len, d_sc.data_ptr(),
                                 d_frames=d_fr.data_ptr())
        bank.sync()
        got, gsd, _ = _score_device(bank, bt, 3, -32767)
    _same(got, d_sc.cpu().numpy().reshape(3, bt.n), "scores")
    _same(gsd, (d_fr.cpu().numpy().reshape(3, bt.n) >= 3).astype(np.uint8), "strands")
    assert got.max() > 100 and gsd.any() and not gsd.all()


# ---- 5. planted shifts ------------------------------------------------------------------------------
def test_planted_shifts():
    cases = FS.shift_cases()
    with _bank() as bank:
        for kind, rev, q, t, A, B in cases:
            want = FS.c_search(q, [t], O.BLOSUM62, *F.PEN, FS.SHIFT_FS)
            six, _ = FS.six_frames(q, [t])
            bank.load_query(q)
            sc, sd = bank.score_frameshift([t], FS.SHIFT_FS)
            assert (int(sc[0]), int(sd[0])) == (int(want[0][0]), int(want[1][0]))
            assert int(sc[0]) >= FS.shift_bound(kind, A, B, FS.SHIFT_FS)
            assert int(sc[0]) > int(six[0]) and int(sd[0]) == int(rev)


# ---- 6. query sets, NULL strands, host form, timing, leaks ------------------------------------------
def _set_case():
    def make():
        qs, seqs, _ = F.search_case()
        rng = np.random.default_rng(139)
        for k in range(0, len(seqs), 7):  # shifted plants of every query
            q = qs[k % 3]
            core = np.insert(F.back_translate(rng, q), 3 * (len(q) // 2) + 1, 0)
            t = np.concatenate([rng.integers(0, 4, 11), core, rng.integers(0, 4, 8)]).astype(np.uint8)
            seqs[k] = F.SC.revcomp(t) if k % 2 else t
        return qs, seqs, FS.c_search_set(qs, seqs, O.BLOSUM62, *F.PEN, -15)
    return _cached("set", make)


def test_query_set_null_strands_and_host_form():
    qs, seqs, want = _set_case()
    assert [len(q) for q in qs] == [17, 130, 60]
    bt = Batch(seqs)
    base = _live()
    with _bank() as bank:
        bank.load_queries(qs)
        got, gsd, name = _score_device(bank, bt, 3, -15)
        assert name == f"fshift nq=3 n={bt.n}"
        _same(got, want[0], "scores")
        _same(gsd, want[1], "strands")
        got2, gsd2, _ = _score_device(bank, bt, 3, -15, strands=False)  # d_strands NULL
        assert np.array_equal(got2, got) and (gsd2 == FILL).all()
        sc, sd = bank.score_frameshift((bt.res, bt.offs, bt.lens), -15)
        assert np.array_equal(sc, got) and np.array_equal(sd, gsd)
        with pytest.raises(S.SwbankError) as ei:  # no best hit is tracked
            bank.best()
        assert ei.value.status == S.ERR_STATE
        bank.load_query(qs[1])
        sc, sd = bank.score_frameshift(seqs, -15)
        assert np.array_equal(sc, want[0][1]) and np.array_equal(sd, want[1][1])
        bank.score_frameshift_device(*bt.ptrs(), 0, bt.max_len, -15, 0)  # an empty batch is fine
        sc, sd = bank.score_frameshift([], -15)
        assert sc.shape == (0,) and sd.shape == (0,)
        bank.set_timing(True)
        _score_device(bank, bt, 1, -15)
        launches, _, ms = bank.timing()
        assert launches == 1 and ms > 0
    assert _live() == base  # the live-buffer count returns to its baseline


def test_multi_device_bank():
    qs, seqs, want = _set_case()
    bt = Batch(seqs)
    with _bank(devices=[0, 0]) as bank:
        bank.load_query(qs[1])
        got, gsd, name = _score_device(bank, bt, 1, -15)
        assert name == f"fshift nq=1 n={bt.n}"
        _same(got[0], want[0][1], "scores")
        _same(gsd[0], want[1][1], "strands")


# ---- 7. an asymmetric matrix, a custom table --------------------------------------------------------
@pytest.mark.parametrize("table", ["standard", "stop-x"])
def test_asymmetric_matrix_and_custom_table(table):
    """asym-prot at -11 / -1 over matrix_cases.frame_case: the transposed matrix changes the model's
    result, so a kernel reading s(a, q) cannot pass.  The custom table (two more stops, a codon for
    X; X and * in the queries) reads rows and columns 22 / 23 of the matrix."""
    tab = MC.stop_x_table() if table == "stop-x" else None
    sub = SEAMS.MATRICES[MC.PROTEIN]()
    pen = MC.MATRIX_SETS[MC.PROTEIN]
    qs, seqs, planted = MC.frame_case(tab)
    want, wrong = _cached(("asym", table), lambda: (
        FS.c_search_set(qs, seqs, sub, *pen, -15, tab),
        FS.c_search_set(qs, seqs, np.ascontiguousarray(sub.T), *pen, -15, tab)))
    changed = [k for k, (i, _) in planted.items() if want[0][i][k] != wrong[0][i][k]]
    assert len(changed) >= 0.8 * len(planted)
    if tab is not None:
        assert all((q == F.X).any() and (q == F.STOP).any() for q in qs)
    bt = Batch(seqs)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH) as bank:
        bank.set_matrix(sub, *pen)
        bank.load_queries(qs)
        got, gsd, _ = _score_device(bank, bt, len(qs), -15, table=tab)
        _same(got, want[0], "scores")
        _same(gsd, want[1], "strands")
        sc, sd = bank.score_frameshift(seqs, -15, codon_table=tab)
        assert np.array_equal(sc, got) and np.array_equal(sd, gsd)
    for k, (i, f) in planted.items():
        assert int(gsd[i][k]) == int(f >= 3)


# ---- 8. scores past 16 bits -------------------------------------------------------------------------
def test_scores_past_16_bits():
    """A diagonal of 127: a 600-residue single-letter query against its back-translation scores
    76,200, past both 16-bit ranges; exact int32, on either strand."""
    sub = np.full((24, 24), -4, np.int8)
    np.fill_diagonal(sub, 127)
    rng = np.random.default_rng(149)
    q = np.full(600, 9, np.uint8)
    t = np.concatenate([rng.integers(0, 4, 7), F.back_translate(rng, q), rng.integers(0, 4, 5)])
    seqs = [t.astype(np.uint8), F.SC.revcomp(t.astype(np.uint8)), rng.integers(0, 4, 900).astype(np.uint8)]
    want = FS.c_search(q, seqs, sub, *F.PEN, -15)
    assert want[0][:2].tolist() == [76200, 76200] and want[1][:2].tolist() == [0, 1]
    with _bank(sub) as bank:
        bank.load_query(q)
        sc, sd = bank.score_frameshift(seqs, -15)
    _same(sc, want[0], "scores")
    _same(sd, want[1], "strands")


# ---- 9. the chain into the top-k list ---------------------------------------------------------------
def test_chain_into_top_hits_on_one_stream():
    """score_frameshift_device -> top_hits_device on one stream with no host step."""
    torch = _torch()
    qs, seqs, want = _set_case()
    bt = Batch(seqs)
    k, nq, dev = 8, 3, torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    with _bank() as bank:
        bank.load_queries(qs)
        d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        d_sd, d_hits = _filled(nq * bt.n), _filled(nq * k * 8)
        d_hsc = torch.zeros(nq * k, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_frameshift_device(*bt.ptrs(), bt.n, bt.max_len, -15, d_sc.data_ptr(),
                                     d_strands=d_sd.data_ptr(), stream=h)
        bank.top_hits_device(d_sc.data_ptr(), bt.n, k, d_hits.data_ptr(), nq=nq,
                             d_hit_scores=d_hsc.data_ptr(), stream=h)
        bank.sync()
        stream.synchronize()
    whits, wsc, _ = TC.ref_top(want[0], k)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint64).reshape(nq, k), whits)
    assert np.array_equal(d_hsc.cpu().numpy().reshape(nq, k), wsc)
    _same(d_sd.cpu().numpy().reshape(nq, bt.n), want[1], "strands")


# ---- 10. refusals -----------------------------------------------------------------------------------
def test_refusals():
    qs, seqs, _ = _set_case()
    bt = Batch(seqs[:8])
    host = (bt.res, bt.offs, bt.lens)
    p = _filled(1 << 12).data_ptr()

    def status(fn, *a, **kw):
        with pytest.raises(S.SwbankError) as ei:
            fn(*a, **kw)
        return ei.value.status

    def both(bank, fs=-15, table=None, batch=host):
        return {status(bank.score_frameshift_device, *bt.ptrs(), bt.n, bt.max_len, fs, p,
                       codon_table=table),
                status(bank.score_frameshift, batch, fs, codon_table=table)}

    with S.ScoreBank() as bank:  # a DNA bank
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(np.arange(20, dtype=np.uint8) % 4)
        assert both(bank) == {S.ERR_UNSUPPORTED}
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_MERGED) as bank:  # merged gaps
        bank.set_matrix(O.BLOSUM62, *F.PEN)
        bank.load_query(qs[0])
        assert both(bank) == {S.ERR_UNSUPPORTED}
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH) as bank:
        assert both(bank) == {S.ERR_STATE}  # no query (a protein bank starts with penalties)
        bank.load_query(qs[0])
        assert both(bank, fs=1) == {S.ERR_ARG}
        assert both(bank, fs=-32768) == {S.ERR_ARG}
        bad_tab = F.standard_table()
        bad_tab[63] = 24
        assert both(bank, table=bad_tab) == {S.ERR_ARG}
        assert status(bank.score_frameshift_device, *bt.ptrs(), bt.n, bt.max_len, -15, 0) == S.ERR_ARG
        assert status(bank.score_frameshift_device, 0, bt.d_offs.data_ptr(), bt.d_lens.data_ptr(),
                      bt.n, bt.max_len, -15, p) == S.ERR_ARG
        bad = bt.res.copy()
        bad[int(bt.offs[5]) + 1] = 5  # a host code of 5 or more
        assert status(bank.score_frameshift, (bad, bt.offs, bt.lens), -15) == S.ERR_ARG
        outside = bt.lens.copy()
        outside[7] += len(bt.res)  # a target outside the buffer
        assert status(bank.score_frameshift, (bt.res, bt.offs, outside), -15) == S.ERR_ARG
        rng = np.random.default_rng(151)
        bank.load_query(rng.integers(0, 20, S.FSHIFT_MAX_QUERY + 1).astype(np.uint8))
        assert both(bank) == {S.ERR_UNSUPPORTED}
        bank.load_queries([qs[0], rng.integers(0, 20, S.FSHIFT_MAX_QUERY + 1).astype(np.uint8)])
        assert both(bank) == {S.ERR_UNSUPPORTED}  # any query of the set
        bank.load_query(qs[0])
        sc, _ = bank.score_frameshift(host, 0)  # fs = 0 and fs = -32767 are the ends of the range
        assert sc.shape == (8,)
        bank.score_frameshift(host, -32767)


def test_device_form_reads_a_code_past_4_as_n():
    qs, seqs, _ = _set_case()
    res, offs, lens = S.pack_targets(seqs[:16])
    odd = res.copy()
    at = np.arange(7, len(res), 29)
    odd[at] = 5 + (at % 250)
    as_n = res.copy()
    as_n[at] = 4
    want = FS.c_search_packed(qs[2], as_n, offs, lens, O.BLOSUM62, *F.PEN, -7)
    bt = Batch(packed=(odd, offs, lens))
    with _bank() as bank:
        bank.load_query(qs[2])
        got, gsd, _ = _score_device(bank, bt, 1, -7)
    _same(got[0], want[0], "scores")
    _same(gsd[0], want[1], "strands")
