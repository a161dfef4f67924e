"""Alignments of frameshift hits on the GPU (include/swbank.h "alignments of frameshift hits",
DESIGN.md §3.16).  Every test compares sw_align_fshift_hits[_device] exactly, record fields and
ops, with the C model of tests/fsalign_cases.py (itself checked against the plain-Python
restatement with its brute-force start by tests/test_fsalign_cases.py), through the host form's
plan and through the device form's slots, plain and with poisoned buffers: the kernels' three row
counts, each pass at its own lane and block seams, the targets' edges, both tables, an asymmetric matrix, a query set in both pair layouts,
the budget and the CIGAR space, one long target, the chain from the score call, every record's
score and strand against the score call's, the six-frame anchor, the refusals.  The CPU references are computed once per process and shared."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fsalign_cases as A
import matrix_cases as MC
import seam_cases as SEAMS
import test_gpu_fshift as TG

pytestmark = pytest.mark.gpu

QLENS = sorted({1, 2, 3} | {k + d for k in (4, 8, 16) for d in (-1, 0, 1)} |
               {255, 256, 257, 511, 512, 513, 1023, 1024})
EDGE_LENS = list(range(10)) + [62, 63, 64, 65, 66, 191, 192, 193, 194, 195, 383, 384, 385, 386,
                               1020, 1021]  # (26 lengths: _gapped_batch walks them in steps of 5)
HIT_NONE, QUERY_NONE = S.HIT_NONE, 0xFFFFFFFF


def _want(qs, seqs, pairs, sub, pen, fs, table=None, cap=None):
    """[(record, ops) | None] by the C model for the pairs (query, target); None: no pair."""
    out = []
    for i, k in pairs:
        if i == QUERY_NONE or k == HIT_NONE:
            out.append(None)
        else:
            out.append(A.c_align(qs[i], seqs[k], sub, *pen, fs, table, cap))
    return out


def _check(got, want, pairs, what, ids=None):
    assert len(got) == len(want) == len(pairs)
    for h, (a, w, (i, k)) in enumerate(zip(got, want, pairs)):
        if w is None:
            assert (a.index, a.id, a.score, a.flags, a.ops) == \
                (HIT_NONE, HIT_NONE, 0, S.ALIGN_EMPTY | S.ALIGN_NO_HIT, ()), (what, h, a)
            assert (a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns, a.n_identities) == (0,) * 6
            continue
        rec = (a.score, a.flags, a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns,
               a.n_identities)
        assert (rec, tuple(a.ops)) == w, (what, h, i, k, rec, S.cigar_string(a.ops), w[0],
                                          S.cigar_string(w[1]))
        assert a.index == k and a.id == (k if ids is None else int(ids[k])), (what, h)


def _host(bank, packed, pairs, fs, table=None, layout="list", cigar_cap=None, ids=None, k=0):
    hq = np.array([i for i, _ in pairs], np.uint32)
    hv = np.array([t for _, t in pairs], np.uint64)
    kw = dict(hits=hv, hit_queries=hq)
    if layout == "top":       # the nq x k layout of top_hits_device
        kw = dict(hits=hv, hits_per_query=k)
    elif layout == "best":    # one entry per target, as best_queries_device writes
        kw = dict(hit_queries=hq)
    return bank.align_frameshift_hits(*packed, fs, codon_table=table, cigar_cap=cigar_cap,
                                      ids=ids, **kw)


def _device(bank, bt, pairs, fs, stride, table=None, layout="list", ids=None, k=0, cigar=True,
            stream=0):
    torch = TG._torch()
    dev = torch.device("cuda", 0)
    n_hits = len(pairs)
    d_hq = TG._to_dev(np.array([i for i, _ in pairs], np.uint32))
    d_hv = TG._to_dev(np.array([t for _, t in pairs], np.uint64))
    d_ids = TG._to_dev(np.asarray(ids, np.uint64)) if ids is not None else None
    d_out = TG._filled(n_hits * S.ALIGNMENT_DTYPE.itemsize)
    d_cig = torch.full((max(1, n_hits * stride),), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    bank.align_frameshift_hits_device(
        *bt.ptrs(), bt.n, bt.max_len, fs, n_hits, d_out.data_ptr(),
        d_hits=0 if layout == "best" else d_hv.data_ptr(),
        d_hit_queries=0 if layout == "top" else d_hq.data_ptr(),
        hits_per_query=k if layout == "top" else 0,
        d_cigar=d_cig.data_ptr() if cigar else 0, cigar_stride=stride, stream=stream,
        d_ids=d_ids.data_ptr() if d_ids is not None else 0, codon_table=table)
    bank.sync()
    rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
    if cigar and stride:
        assert [int(r["cigar_offset"]) for r in rec] == [h * stride for h in range(n_hits)]
    return S.alignments_from(rec, d_cig.cpu().numpy().view(np.uint32))


def _both(bank, seqs, pairs, want, fs, what, table=None, stride=None):
    """The host form's plan and the device form's slots against the model."""
    bt = TG.Batch(seqs)
    stride = stride or max(len(w[1]) for w in want if w is not None) + 1
    _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, fs, table), want, pairs, what + " host")
    assert bank.last_kernel() == f"align-fshift i32 nq={max(bank.query_count(), 1)} " \
        f"hits={len(pairs)} chunks=1"
    _check(_device(bank, bt, pairs, fs, stride, table), want, pairs, what + " device")


# ---- 1. query rows: the lane counts of the three kernels ------------------------------------------
def _rows_case(m):
    def make():
        rng = np.random.default_rng([113, m])
        q = rng.integers(0, 20, m).astype(np.uint8)
        seqs = TG._seam_targets(q, 0)
        pairs = [(0, k) for k in range(len(seqs))]
        return q, seqs, pairs, _want([q], seqs, pairs, O.BLOSUM62, F.PEN, -7)
    return TG._cached(("fsalign-rows", m), make)


@pytest.mark.parametrize("poison", ["plain", "poison"])
@pytest.mark.parametrize("m", QLENS)
def test_query_rows(m, poison, monkeypatch):
    """Queries of 1, 2, 3 rows and each side of 4, 8, 16, 256, 512 and 1,024 rows against 64
    targets holding windows of the query (anywhere in it, so passes B and C start at rows that
    are no multiple of K) with a base inserted or removed, on both strands."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    q, seqs, pairs, want = _rows_case(m)
    with TG._bank() as bank:
        bank.load_query(q)
        _both(bank, seqs, pairs, want, -7, f"rows {m}")
    if m == 257:
        kinds = {c: sum(op & 15 == x for w in want for op in w[1]) for x, c in enumerate(A.OP_TEXT)}
        print(kinds)
        assert kinds["/"] >= 5 and kinds["\\"] >= 5 and min(w[0][2] for w in want if w[1]) % 8


@pytest.mark.parametrize("poison", ["plain", "poison"])
@pytest.mark.parametrize("K", [4, 8, 16])
def test_passes_at_their_seams(K, poison, monkeypatch):
    """fsalign_cases.seam_family: per pass an I run across a lane seam and a D run across a
    64-codon block seam in that pass's own numbering; every target is live by the C model's
    mutant of that pass (tests/test_fsalign_cases.py states the count kept)."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    q, kept, _ = TG._cached(("fsalign-seams", K), lambda: A.seam_family(K, O.BLOSUM62, F.PEN))
    seqs = [t for t, _, _, _, _ in kept]
    pairs = [(0, k) for k in range(len(seqs))]
    want = TG._cached(("fsalign-seams-want", K),
                      lambda: _want([q], seqs, pairs, O.BLOSUM62, F.PEN, -15))
    assert len(seqs) >= 10
    with TG._bank() as bank:
        bank.load_query(q)
        _both(bank, seqs, pairs, want, -15, f"seams {K}")


# ---- 2. target lengths, tables, edges ---------------------------------------------------------------
def _edge_targets(q, rng):
    """[(target, where)]: a base inserted or removed so that the shift lies within the first 4
    bases of a strand ("start"), at the codon indices 63 | 64 ("block"), or within the last 4 bases
    of a strand ("end": the last codon is reached over the p - 4 or the p - 2 link at the matrix's
    far edge), each on both strands."""
    out = []
    for where in (1, 2, 3, 4, 189, 190, 191, 192, 193):  # codons 63 | 64 start at 189 | 192
        for kind in ("ins", "del"):
            core = F.back_translate(rng, q)
            pre = 0 if where < 10 else 9  # random bases before the plant
            core = np.insert(core, where - pre, 1) if kind == "ins" else np.delete(core, where - pre)
            t = np.concatenate([rng.integers(0, 4, pre), core]).astype(np.uint8)
            out += [(t, "start" if where < 10 else "block"), (F.SC.revcomp(t), "start" if where < 10 else "block")]
    for kind, tails in (("ins", (3, 4, 5, 6, 7)), ("del", (1, 3, 4, 5, 6, 7))):
        for tail in tails:  # ... `tail` bases before the strand's end, which is the plant's
            core = F.back_translate(rng, q[:20])
            core = np.insert(core, len(core) - tail, 2) if kind == "ins" else \
                np.delete(core, len(core) - tail)
            t = np.concatenate([rng.integers(0, 4, 5), core]).astype(np.uint8)
            out += [(t, "end"), (F.SC.revcomp(t), "end")]
    return out


def _edge_case(table):
    def make():
        tab = F.custom_table() if table == "custom" else None
        rng = np.random.default_rng(191)
        q = rng.integers(0, 20, 70).astype(np.uint8)
        made = _edge_targets(q, rng)
        seqs = [t for t, _ in made]
        pairs = [(0, k) for k in range(len(seqs))]
        return tab, q, made, seqs, pairs, {fs: _want([q], seqs, pairs, O.BLOSUM62, F.PEN, fs, tab)
                                           for fs in (-7, 0)}
    return TG._cached(("fsalign-edges", table), make)


def _strand_window(rec, L):
    """(p_start, last base of the last codon) of a record on its own strand."""
    return (L - 1 - rec[5], L - 1 - rec[4]) if rec[1] & S.ALIGN_REVERSE else (rec[4], rec[5])


@pytest.mark.parametrize("poison", ["plain", "poison"])
@pytest.mark.parametrize("table", ["standard", "custom"])
def test_shifts_at_the_strand_edges_and_the_block_seam(table, poison, monkeypatch):
    """All 58 plants of _edge_targets in one batch, at fs = -7 and with free shifts (fs = 0, where
    a hit follows a shift even two codons from its end).  Under the standard table, at fs = 0:
    on each strand some hits shift within the first two codons of a window that starts within the
    strand's first 4 bases, and some within the last two codons of a window that ends at the
    strand's last base; at fs = -7 the block plants shift at codon index 63 | 64."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    tab, q, made, seqs, pairs, want = _edge_case(table)
    assert len(made) == 58 and len(pairs) <= 64
    with TG._bank() as bank:
        bank.load_query(q)
        for fs in (-7, 0):
            _both(bank, seqs, pairs, want[fs], fs, f"edges fs={fs}", tab)
    if tab is not None:
        return
    first = {False: 0, True: 0}
    last = {False: 0, True: 0}
    for (t, where), (rec, ops) in zip(made, want[0]):
        if len(ops) < 3:
            continue
        rev, (ps, pe) = bool(rec[1] & S.ALIGN_REVERSE), _strand_window(rec, len(t))
        if where == "start" and ops[0] >> 4 <= 2 and ops[1] & 15 >= A.OP_SKIP and ps <= 3:
            first[rev] += 1
        if where == "end" and ops[-1] >> 4 <= 2 and ops[-2] & 15 >= A.OP_SKIP and pe == len(t) - 1:
            last[rev] += 1
    print("first two codons", first, "last two codons", last)
    assert min(first.values()) >= 4 and min(last.values()) >= 4
    block = [ops for (t, where), (rec, ops) in zip(made, want[-7]) if where == "block"]
    assert sum(len(o) == 3 and o[1] & 15 >= A.OP_SKIP and o[0] >> 4 in (59, 60, 61, 62)
               for o in block) >= 12


@pytest.mark.parametrize("poison", ["plain", "poison"])
@pytest.mark.parametrize("table", ["standard", "custom"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_target_lengths(n, table, poison, monkeypatch):
    """Targets of {0..9, 62..66, 191..195, 383..386, 1020, 1021} nt at odd offsets between guard
    bytes of code 4, N inside every third; both codon tables."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    tab = F.custom_table() if table == "custom" else None
    rng = np.random.default_rng([157, n])
    q = rng.integers(0, 20, 70).astype(np.uint8)
    pool = EDGE_LENS[19:] + EDGE_LENS[:19] if n == 1 else EDGE_LENS
    res, offs, lens = TG._gapped_batch(n, pool)
    assert n < 63 or set(EDGE_LENS) <= set(lens.tolist())
    seqs = [res[int(o):int(o) + int(ln)] for o, ln in zip(offs, lens)]
    pairs = [(0, k) for k in range(n)]
    want = TG._cached(("fsalign-len", n, table),
                      lambda: _want([q], seqs, pairs, O.BLOSUM62, F.PEN, -7, tab))
    bt = TG.Batch(packed=(res, offs, lens))
    stride = max(len(w[1]) for w in want) + 1
    with TG._bank() as bank:
        bank.load_query(q)
        _check(_host(bank, (res, offs, lens), pairs, -7, tab), want, pairs, "host")
        _check(_device(bank, bt, pairs, -7, stride, tab), want, pairs, "device")
    assert np.array_equal(bt.d_res.cpu().numpy(), res)  # the input is left alone
    assert all(w == A.EMPTY for w, ln in zip(want, lens) if ln < 3)
    assert n < 63 or sum(w[0][0] > 0 for w in want) >= 20


# ---- 3. strands, an asymmetric matrix, X and *, a query set in both layouts -------------------------
def _asym_case(table):
    def make():
        tab = MC.stop_x_table() if table == "stop-x" else None
        sub, pen = SEAMS.MATRICES[MC.PROTEIN](), MC.MATRIX_SETS[MC.PROTEIN]
        qs, seqs, planted = MC.frame_case(tab)
        seqs = seqs[:40]
        pairs = [(i, k) for k in range(len(seqs)) for i in range(len(qs))][:64]
        want = _want(qs, seqs, pairs, sub, pen, -15, tab)
        wrong = _want(qs, seqs, pairs, np.ascontiguousarray(sub.T), pen, -15, tab)
        return tab, sub, pen, qs, seqs, pairs, want, wrong
    return TG._cached(("fsalign-asym", table), make)


@pytest.mark.parametrize("poison", ["plain", "poison"])
@pytest.mark.parametrize("table", ["standard", "stop-x"])
def test_asymmetric_matrix(table, poison, monkeypatch):
    """matrix_cases.frame_case under the asymmetric protein matrix: its transpose changes more
    than half the model's records, so a kernel reading s(a, q) cannot pass; X and * in the
    queries under the table with two more stops and a codon for X; both strands occur."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    tab, sub, pen, qs, seqs, pairs, want, wrong = _asym_case(table)
    assert 2 * sum(w != x for w, x in zip(want, wrong)) > len(want)
    assert {bool(w[0][1] & S.ALIGN_REVERSE) for w in want if w[0][0] > 0} == {False, True}
    if tab is not None:
        assert all((q == F.X).any() and (q == F.STOP).any() for q in qs)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH) as bank:
        bank.set_matrix(sub, *pen)
        bank.load_queries(qs)
        _both(bank, seqs, pairs, want, -15, "asym", tab)


def _set_pairs(want_scores, nq, n, k):
    """The top-hits layout: per query its k best targets, sentinel tails where fewer score."""
    pairs = []
    for i in range(nq):
        order = [t for t in np.argsort(-want_scores[i], kind="stable")[:k] if want_scores[i][t] > 0]
        pairs += [(i, int(t)) for t in order] + [(i, HIT_NONE)] * (k - len(order))
    return pairs


@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_query_set_in_both_layouts(poison, monkeypatch):
    """A set of three queries: a scrambled pair list with SW_QUERY_NONE / SW_HIT_NONE sentinels,
    the nq x k top-hits layout with sentinel tails, and the best-query layout (one entry per
    target, thresholded); ids; host against device form."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    qs, seqs, wsc = TG._set_case()
    seqs = seqs[:60]
    sc = wsc[0][:, :60].copy()
    sc[1, sc[1] < 60] = 0  # (a query with fewer than k hits: sentinel tails)
    rng = np.random.default_rng(163)
    ids = rng.integers(0, 1 << 62, len(seqs)).astype(np.uint64)
    lists = {}
    scr = [(int(i), int(k)) for i, k in zip(rng.integers(0, 3, 40), rng.integers(0, 60, 40))]
    scr[3], scr[17], scr[29] = (QUERY_NONE, 5), (1, HIT_NONE), (QUERY_NONE, HIT_NONE)
    lists["list"] = (scr, 0)
    lists["top"] = (_set_pairs(sc, 3, 60, 8), 8)
    best = wsc[0][:, :60].argmax(axis=0)
    lists["best"] = ([(int(best[k]) if wsc[0][best[k], k] >= 40 else QUERY_NONE, k)
                      for k in range(60)], 0)
    assert any(k == HIT_NONE for _, k in lists["top"][0])
    assert any(i == QUERY_NONE for i, _ in lists["best"][0])
    bt = TG.Batch(seqs)
    base = TG._live()
    with TG._bank() as bank:
        bank.load_queries(qs)
        for layout, (pairs, k) in lists.items():
            model_pairs = [(i, HIT_NONE if i == QUERY_NONE else t) for i, t in pairs]
            want = TG._cached(("fsalign-set", layout),
                              lambda: _want(qs, seqs, model_pairs, O.BLOSUM62, F.PEN, -15))
            got_h = _host(bank, (bt.res, bt.offs, bt.lens), pairs, -15, layout=layout, ids=ids, k=k)
            _check(got_h, want, pairs, layout + " host", ids)
            assert bank.last_kernel() == f"align-fshift i32 nq=3 hits={len(pairs)} chunks=1"
            got_d = _device(bank, bt, pairs, -15, 140, layout=layout, ids=ids, k=k)
            _check(got_d, want, pairs, layout + " device", ids)
            assert [a.score for a in got_h if a.score] == \
                [int(wsc[0][i][t]) for (i, t), w in zip(pairs, want) if w and w[0][0]]
    assert TG._live() == base  # the live-buffer count returns to its baseline


# ---- 4. the budget and the CIGAR space --------------------------------------------------------------
def _budget_case():
    def make():
        rng = np.random.default_rng(167)
        q = rng.integers(0, 20, 1024).astype(np.uint8)
        seqs = []
        for k in range(24):  # windows of 100..250 rows with a shift, 300..760 nt
            ln = int(rng.integers(100, 251))
            a = int(rng.integers(0, 1024 - ln))
            core = np.insert(F.back_translate(rng, q[a:a + ln]), 3 * (ln // 2) + 1, 3)
            t = np.concatenate([rng.integers(0, 4, 7), core, rng.integers(0, 4, 4)]).astype(np.uint8)
            seqs.append(F.SC.revcomp(t) if k % 2 else t)
        # one window over 1 MiB of direction store: 340 rows x 1,021 nt at K = 16
        seqs[11] = np.concatenate([F.back_translate(rng, q[400:740]), [0]]).astype(np.uint8)
        pairs = [(0, k) for k in range(24)]
        return q, seqs, pairs, _want([q], seqs, pairs, O.BLOSUM62, F.PEN, -15)
    return TG._cached("fsalign-budget", make)


@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_budget_chunks_and_one_window_over_it(poison, monkeypatch):
    """SWBANK_ALIGN_MB=1: the host form runs its windows in several chunks and only the window
    over the budget loses its path, with exact coordinates; the device form's slot (1,024 rows x
    1,021 nt) does not fit, so every non-empty hit keeps its coordinates without a path."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    q, seqs, pairs, want = _budget_case()
    rows, nt = want[11][0][3] - want[11][0][2] + 1, want[11][0][5] - want[11][0][4] + 1
    assert ((nt - 2 + 2) // 3 + (rows + 15) // 16 - 1) * 192 * 16 > 1 << 20
    bt = TG.Batch(seqs)
    with TG._bank() as bank:
        bank.load_query(q)
        _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, -15), want, pairs, "default budget")
        assert bank.last_kernel() == "align-fshift i32 nq=1 hits=24 chunks=1"
        monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
        lost = [(A.no_path(w[0]), ()) if k == 11 else w for k, w in enumerate(want)]
        _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, -15), lost, pairs, "1 MiB host")
        name = bank.last_kernel()
        assert name.startswith("align-fshift i32 nq=1 hits=24 chunks=") and \
            int(name.rsplit("=", 1)[1]) > 1, name
        none = [(A.no_path(w[0]), ()) for w in want]
        _check(_device(bank, bt, pairs, -15, 300), none, pairs, "1 MiB device")
        assert bank.last_kernel() == "align-fshift i32 nq=1 hits=24 chunks=0"


@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_cigar_space(poison, monkeypatch):
    """cigar_stride one op too small for some hits, d_cigar NULL, and a host cigar_cap that runs
    out mid-list: those hits keep exact coordinates and lose their paths, the others keep them."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    q, seqs, pairs, want = _rows_case(65)
    need = [len(w[1]) for w in want]
    stride = max(need) - 1  # one op too small for the longest paths
    assert stride >= 3 and sum(n > stride for n in need) >= 1 and sum(0 < n <= stride for n in need)
    bt = TG.Batch(seqs)
    with TG._bank() as bank:
        bank.load_query(q)
        cut = [w if len(w[1]) <= stride else (A.no_path(w[0]), ()) for w in want]
        _check(_device(bank, bt, pairs, -7, stride), cut, pairs, "stride")
        none = [w if not w[1] else (A.no_path(w[0]), ()) for w in want]
        _check(_device(bank, bt, pairs, -7, stride, cigar=False), none, pairs, "no cigar")
        _check(_device(bank, bt, pairs, -7, 0), none, pairs, "stride 0")
        cap, left, fit = sum(need) // 2, sum(need) // 2, []
        for w in want:  # packed in hit order; a hit that no longer fits is skipped
            ok = len(w[1]) <= left
            left -= len(w[1]) if ok else 0
            fit.append(w if ok else (A.no_path(w[0]), ()))
        assert any(f != w for f, w in zip(fit, want))
        _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, -7, cigar_cap=cap), fit, pairs, "cap")
        _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, -7, cigar_cap=0), none, pairs, "cap 0")


# ---- 5. one long target among short ones ------------------------------------------------------------
@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_one_long_target_among_short_ones(poison, monkeypatch):
    """A 70,000-nt target with a 40-aa shifted plant at its far end on the reverse strand, among
    100-nt ones: coordinates past 65,535; hit lists with repeats, long and short hits by turns."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    rng = np.random.default_rng(173)
    q = rng.integers(0, 20, 40).astype(np.uint8)
    seqs = [rng.integers(0, 4, 100).astype(np.uint8) for _ in range(12)]
    long = rng.integers(0, 4, 70000).astype(np.uint8)
    core = np.insert(F.back_translate(rng, q), 61, 2)
    long[69001:69001 + len(core)] = core
    seqs[5] = F.SC.revcomp(long)
    seqs[8][10:10 + 60] = F.back_translate(rng, q[:20])
    pairs = [(0, k) for k in (5, 8, 5, 0, 5, 11, 8, 5)]
    want = TG._cached("fsalign-long", lambda: _want([q], seqs, pairs, O.BLOSUM62, F.PEN, -15))
    assert want[0][0][1] & S.ALIGN_REVERSE and want[0][0][4] < 1000 and len(want[0][1]) == 3
    fwd = A.c_align(q, long, O.BLOSUM62, *F.PEN, -15)
    assert fwd[0][4] > 65535 and fwd[1] == want[0][1]  # (the same hit, seen from the other strand)
    with TG._bank() as bank:
        bank.load_query(q)
        _both(bank, seqs, pairs, want, -15, "long")
        seqs[5] = long  # ... and on the forward strand, its coordinates past 65,535
        want2 = [fwd if k == 5 else w for (_, k), w in zip(pairs, want)]
        _both(bank, seqs, pairs, want2, -15, "long forward")


# ---- 6. the chain, the anchor, timing, the multi-device bank ----------------------------------------
@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_chain_from_the_score_call_on_one_stream(poison, monkeypatch):
    """score_frameshift_device -> top_hits_device -> align_frameshift_hits_device on one stream
    with no host step: the record scores are the score call's, the strand flags its strands."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    torch = TG._torch()
    qs, seqs, wsc = TG._set_case()
    bt = TG.Batch(seqs)
    k, nq, dev = 8, 3, torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    with TG._bank() as bank:
        bank.load_queries(qs)
        d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        d_sd, d_hits = TG._filled(nq * bt.n), TG._filled(nq * k * 8)
        d_out = TG._filled(nq * k * S.ALIGNMENT_DTYPE.itemsize)
        d_cig = torch.full((nq * k * 150,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        d_hsc = torch.zeros(nq * k, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_frameshift_device(*bt.ptrs(), bt.n, bt.max_len, -15, d_sc.data_ptr(),
                                     d_strands=d_sd.data_ptr(), stream=h)
        bank.top_hits_device(d_sc.data_ptr(), bt.n, k, d_hits.data_ptr(), nq=nq,
                             d_hit_scores=d_hsc.data_ptr(), stream=h)
        bank.align_frameshift_hits_device(*bt.ptrs(), bt.n, bt.max_len, -15, nq * k,
                                          d_out.data_ptr(), d_hits=d_hits.data_ptr(),
                                          hits_per_query=k, d_cigar=d_cig.data_ptr(),
                                          cigar_stride=150, stream=h)
        bank.sync()
        stream.synchronize()
    hits = d_hits.cpu().numpy().view(np.uint64)
    sc = d_sc.cpu().numpy().reshape(nq, bt.n)
    sd = d_sd.cpu().numpy().reshape(nq, bt.n)
    got = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                            d_cig.cpu().numpy().view(np.uint32))
    pairs = [(h // k, int(t)) for h, t in enumerate(hits)]
    assert all(t != HIT_NONE for _, t in pairs)
    for a, (i, t) in zip(got, pairs):
        assert a.score == sc[i][t] == wsc[0][i][t] and a.reverse == bool(sd[i][t]) and a.has_path
    _check(got, _want(qs, seqs, pairs, O.BLOSUM62, F.PEN, -15), pairs, "chain")


@pytest.mark.parametrize("fs", [-15, -32767])
@pytest.mark.parametrize("m", [5, 257, 513])
def test_record_scores_are_the_score_calls_on_every_target(m, fs):
    """One query per row count of the kernels against the 64 seam targets, every target a hit with
    no selection in between, so ties between the strands and zero scores are among them: the
    record's score is score_frameshift_device's, its strand flag that call's strand, and a target
    that scores 0 comes back SW_ALIGN_EMPTY.  (The two calls run the same walk; this holds them
    to it.)"""
    q, seqs, _ = TG._seam_case(m)
    assert len(seqs) == 64 and max(len(t) for t in seqs) <= 260
    bt = TG._cached(("seam-batch", m), lambda: TG.Batch(seqs))
    pairs = [(0, k) for k in range(bt.n)]
    with TG._bank() as bank:
        bank.load_query(q)
        sc, sd, _ = TG._score_device(bank, bt, 1, fs)
        got = _device(bank, bt, pairs, fs, 0, cigar=False)
    assert (sc[0] > 0).sum() >= 32 and sc[0][5] == sc[0][9] == 0  # (5 and 9 hold no codon)
    for k, a in enumerate(got):
        assert a.index == k and a.score == sc[0][k], (m, fs, k, a.score, sc[0][k])
        if sc[0][k] > 0:
            assert a.reverse == bool(sd[0][k]) and not a.empty, (m, fs, k, a.flags, sd[0][k])
        else:
            assert a.flags == S.ALIGN_EMPTY, (m, fs, k, a.flags)


@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_anchor_equals_align_frame_hits(poison, monkeypatch):
    """fs = -32767 and a strictly best frame: the record of align_frame_hits for that frame,
    field for field and op for op (the pairs of the CPU anchor test, on the device)."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    import test_fsalign_cases as TA
    qs, seqs, pairs = TG._cached("fsalign-anchor", TA.anchor_pairs)
    untied = [(i, k, f) for i, k, f, _ in pairs if f is not None][:64]
    res, offs, lens = S.pack_targets(seqs)
    frames = np.zeros((3, len(seqs)), np.uint8)
    for i, k, f in untied:
        frames[i, k] = f
    hq = np.array([i for i, _, _ in untied], np.uint32)
    hv = np.array([k for _, k, _ in untied], np.uint64)
    with TG._bank() as bank:
        bank.load_queries(qs)
        want = bank.align_frame_hits(res, offs, lens, frames, hits=hv, hit_queries=hq)
        got = bank.align_frameshift_hits(res, offs, lens, -32767, hits=hv, hit_queries=hq)
        by_slot = _device(bank, TG.Batch(seqs), [(i, k) for i, k, _ in untied], -32767,
                          max(len(a.ops) for a in want) + 1)
    assert len(got) >= 60 and all(a.has_path for a in got)
    assert got == want, "host form"
    # (the device form's cigar_offset is h * stride; everything else is the frame record)
    assert [(a.index, a.id, a.score, a.flags, a.q_start, a.q_end, a.t_start, a.t_end,
             a.n_columns, a.n_identities, tuple(a.ops)) for a in by_slot] == \
        [(a.index, a.id, a.score, a.flags, a.q_start, a.q_end, a.t_start, a.t_end,
          a.n_columns, a.n_identities, tuple(a.ops)) for a in want], "device form"


@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_timing_brackets_multi_device_and_empty_calls(poison, monkeypatch):
    """With sw_bank_set_timing the end / start passes and the path passes are one launch each; a
    [0, 0] bank runs the call on its root; n_hits = 0 is fine."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    q, seqs, pairs, want = _rows_case(17)
    bt = TG.Batch(seqs)
    stride = max(len(w[1]) for w in want) + 1
    base = TG._live()
    with TG._bank() as bank:
        bank.load_query(q)
        bank.set_timing(True)
        _device(bank, bt, pairs, -7, stride)
        launches, _, ms = bank.timing()
        assert launches == 2 and ms > 0
        _device(bank, bt, pairs, -7, stride, cigar=False)
        assert bank.timing()[0] == 1
        _host(bank, (bt.res, bt.offs, bt.lens), pairs, -7)
        assert bank.timing()[0] == 2
        assert _host(bank, (bt.res, bt.offs, bt.lens), [], -7) == []
        bank.align_frameshift_hits_device(*bt.ptrs(), bt.n, bt.max_len, -7, 0, 0, hits_per_query=1)
    with TG._bank(devices=[0, 0]) as bank:
        bank.load_query(q)
        _both(bank, seqs, pairs, want, -7, "[0, 0]")
    assert TG._live() == base


# ---- 7. refusals -------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_refusals(poison, monkeypatch):
    """Every refusal, in the order of the header's list, by both forms."""
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")
    qs, seqs, _ = TG._set_case()
    bt = TG.Batch(seqs[:8])
    host = (bt.res, bt.offs, bt.lens)
    p = TG._filled(1 << 14).data_ptr()
    hv = np.arange(8, dtype=np.uint64)

    def status(fn, *a, **kw):
        with pytest.raises(S.SwbankError) as ei:
            fn(*a, **kw)
        return ei.value.status

    def both(bank, fs=-15, table=None):
        return {status(bank.align_frameshift_hits_device, *bt.ptrs(), bt.n, bt.max_len, fs, 8, p,
                       hits_per_query=8, codon_table=table),
                status(bank.align_frameshift_hits, *host, fs, hits=hv, hits_per_query=8,
                       codon_table=table)}

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
        assert status(bank.align_frameshift_hits_device, *bt.ptrs(), bt.n, bt.max_len, -15, 8, 0,
                      hits_per_query=8) == S.ERR_ARG  # a NULL record buffer
        assert status(bank.align_frameshift_hits_device, 0, bt.d_offs.data_ptr(),
                      bt.d_lens.data_ptr(), bt.n, bt.max_len, -15, 8, p,
                      hits_per_query=8) == S.ERR_ARG
        assert status(bank.align_frameshift_hits_device, *bt.ptrs(), bt.n, bt.max_len, -15, 8, p) \
            == S.ERR_ARG  # neither hit_queries nor hits_per_query
        assert status(bank.align_frameshift_hits_device, *bt.ptrs(), bt.n, 1 << 29, -15, 8, p,
                      hits_per_query=8) == S.ERR_UNSUPPORTED  # strands of less than 2^29 codes
        bad = bt.res.copy()
        bad[int(bt.offs[5]) + 1] = 5  # a host code of 5 or more in a listed target
        assert status(bank.align_frameshift_hits, bad, bt.offs, bt.lens, -15, hits=hv,
                      hits_per_query=8) == S.ERR_ARG
        assert status(bank.align_frameshift_hits, *host, -15, hits=np.array([8], np.uint64),
                      hits_per_query=1) == S.ERR_ARG  # a target >= n
        rng = np.random.default_rng(179)
        bank.load_query(rng.integers(0, 20, S.FSHIFT_MAX_QUERY + 1).astype(np.uint8))
        assert both(bank) == {S.ERR_UNSUPPORTED}
        bank.load_query(qs[0])
        assert len(bank.align_frameshift_hits(*host, 0, hits=hv, hits_per_query=8)) == 8
        assert len(bank.align_frameshift_hits(*host, -32767, hits=hv, hits_per_query=8)) == 8
