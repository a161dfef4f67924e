"""Alignments of global-local hits on the GPU (include/swbank.h "alignments of global-local hits",
DESIGN.md §3.18).  Every test compares sw_align_glocal_hits[_device] exactly, record fields and
ops, with the C model of tests/glalign_cases.py (itself checked against the plain-Python
restatement with its brute-force start by tests/test_glalign_cases.py), through the host form's
plan and through the device form's slots, plain and with poisoned buffers: the kernels' three row
counts and the targets' edges in all three modes, each pass at its own lane and block seams, gaps
at the boundaries and empty pairs, tie-rich pairs, an asymmetric matrix, a query set in the three
pair layouts, the chain from the score call, the budget and the CIGAR space, one long target, the
refusals.  The CPU references are computed once per process and shared."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import glalign_cases as A
import glocal_cases as G
import seam_cases as SEAMS
import strand_cases as SC
import test_gpu_glocal as TG

pytestmark = pytest.mark.gpu

QLENS = [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024]
TLENS = [0, 1, 2, 63, 64, 65, 129, 200, 333]  # (the last two: room for the noisy windows)
HIT_NONE, QUERY_NONE = S.HIT_NONE, S.QUERY_NONE
FILL32 = TG.FILL32
POISON = pytest.mark.parametrize("poison", ["plain", "poison"])


def _poison(poison, monkeypatch):
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")


def _want(qs, seqs, pairs, sub, pen, ends, both, cap=None):
    """[(record, ops) | None] by the C model for the pairs (query, target); None: no pair."""
    return [None if i == QUERY_NONE or k == HIT_NONE else
            A.c_align(qs[i], seqs[k], sub, *pen, ends, both, cap=cap) for i, k in pairs]


def _check(got, want, pairs, what, ids=None):
    assert len(got) == len(want) == len(pairs)
    for h, (a, w, (i, k)) in enumerate(zip(got, want, pairs)):
        if w is None:  # a sentinel slot is fully defined
            assert (a.index, a.id, a.score, a.flags, a.ops) == \
                (HIT_NONE, HIT_NONE, 0, S.ALIGN_EMPTY | S.ALIGN_NO_HIT, ()), (what, h, a)
            assert (a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns, a.n_identities) == (0,) * 6
            continue
        rec = (a.score, a.flags, a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns,
               a.n_identities)
        assert (rec, tuple(a.ops)) == w, (what, h, i, k, rec, A.cigar(a.ops), w[0], A.cigar(w[1]))
        assert a.index == k and a.id == (k if ids is None else int(ids[k])), (what, h)


def _lists(pairs, layout, k):
    hq = np.array([i for i, _ in pairs], np.uint32)
    hv = np.array([t for _, t in pairs], np.uint64)
    if layout == "top":       # the nq x k layout of top_hits_device
        return dict(hits=hv, hits_per_query=k)
    if layout == "best":      # one entry per target, as best_queries_device writes
        return dict(hit_queries=hq)
    return dict(hits=hv, hit_queries=hq)


def _host(bank, packed, pairs, ends, both, layout="list", cigar_cap=None, ids=None, k=0):
    return bank.align_glocal_hits(*packed, ends, both_strands=both, cigar_cap=cigar_cap, ids=ids,
                                  **_lists(pairs, layout, k))


def _device(bank, bt, pairs, ends, both, stride, layout="list", ids=None, k=0, cigar=True,
            stream=0, max_len=None):
    torch = TG._torch()
    n_hits = len(pairs)
    kw = _lists(pairs, layout, k)
    keep = {name: TG._to_dev(kw[name]) for name in ("hits", "hit_queries") if name in kw}
    d_ids = TG._to_dev(np.asarray(ids, np.uint64)) if ids is not None else None
    d_out = TG._filled(n_hits * S.ALIGNMENT_DTYPE.itemsize)
    d_cig = torch.full((max(1, n_hits * stride),), FILL32, dtype=torch.int32,
                       device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    bank.align_glocal_hits_device(
        *bt.ptrs(), bt.n, bt.max_len if max_len is None else max_len, ends, n_hits,
        d_out.data_ptr(), both_strands=both,
        d_hits=keep["hits"].data_ptr() if "hits" in keep else 0,
        d_hit_queries=keep["hit_queries"].data_ptr() if "hit_queries" in keep else 0,
        hits_per_query=kw.get("hits_per_query", 0),
        d_cigar=d_cig.data_ptr() if cigar else 0, cigar_stride=stride, stream=stream,
        d_ids=d_ids.data_ptr() if d_ids is not None else 0)
    bank.sync()
    rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
    if cigar and stride:
        assert [int(r["cigar_offset"]) for r in rec] == [h * stride for h in range(n_hits)]
    return S.alignments_from(rec, d_cig.cpu().numpy().view(np.uint32))


def _both_forms(bank, bt, pairs, want, ends, both, what, stride=None, chunks=1, **kw):
    """The host form's plan and the device form's slots against the model."""
    stride = stride or max([len(w[1]) for w in want if w is not None] + [0]) + 1
    _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, ends, both, **kw), want, pairs,
           (what, "host"), kw.get("ids"))
    if chunks is not None:
        assert bank.last_kernel() == f"align-glocal i32 ends={ends} " \
            f"nq={max(bank.query_count(), 1)} hits={len(pairs)} chunks={chunks}"
    _check(_device(bank, bt, pairs, ends, both, stride, **kw), want, pairs, (what, "device"),
           kw.get("ids"))


# ---- 1. shapes ------------------------------------------------------------------------------------
def _shape_case(name, m):
    def make():
        matrix, pen = TG.SETS3[name]
        sub = SEAMS.MATRICES[matrix]()
        alpha = sub.shape[0]
        rng = np.random.default_rng([353, m, alpha])
        q = rng.integers(0, 4 if alpha == 5 else 20, m).astype(np.uint8)
        packed = TG._gapped_batch(27, TLENS, q, alpha, 2)
        seqs = [packed[0][int(o):int(o) + int(n)] for o, n in zip(packed[1], packed[2])]
        pairs = [(0, k) for k in range(len(seqs))]
        want = {(e, b): _want([q], seqs, pairs, sub, pen, e, b)
                for e in G.MODES for b in ((False, True) if alpha == 5 else (False,))}
        return q, packed, pairs, want
    return TG._cached(("glalign-shape", name, m), make)


@POISON
@pytest.mark.parametrize("ends", G.MODES)
@pytest.mark.parametrize("name", list(TG.SETS3))
def test_query_rows_and_target_edges(name, ends, poison, monkeypatch):
    """Queries of 1 to 5 rows and each side of 256, 512 and 1,024 rows against 27 targets of 0, 1,
    2, 63, 64, 65, 129, 200 and 333 codes at odd offsets between guard bytes: noisy windows of the
    query with a substitution, an insertion or a deletion, on either strand, and random targets;
    DNA 5 / -4 at -12 / -4 on one strand and on both, BLOSUM62 at -11 / -1."""
    _poison(poison, monkeypatch)
    matrix, pen = TG.SETS3[name]
    seen = set()
    with TG._bank(matrix, pen) as bank:
        for m in QLENS:
            q, packed, pairs, want = _shape_case(name, m)
            assert set(TLENS) == set(packed[2].tolist())
            bt = TG._cached(("glalign-shape-batch", name, m), lambda: TG.Batch(packed=packed))
            bank.load_query(q)
            for both in ((False, True) if name == "dna" else (False,)):
                _both_forms(bank, bt, pairs, want[ends, both], ends, both, (name, m, ends, both))
                seen |= {(w[0][1], w[1][0] & 15, w[1][-1] & 15) for w in want[ends, both] if w[1]}
    flags = {f for f, _, _ in seen}
    assert 0 in flags and (name != "dna" or S.ALIGN_REVERSE in flags)
    assert len({(a, b) for _, a, b in seen}) >= 3  # paths that begin or end in a gap occur


# ---- 2. every pass at its own seams -----------------------------------------------------------------
@POISON
@pytest.mark.parametrize("K", G.ROWS)
def test_passes_at_their_seams(K, poison, monkeypatch):
    """glalign_cases.pass_plants: per pass a run of query residues against gaps across a lane seam
    and a run of target residues against gaps across a 64-step block seam in that pass's own rows
    and columns (pass B's reversed ones; pass C's window, which under TARGET starts at q_start).
    A plant counts only if the C model's mutant of that pass changes its record; at least 3 of 4
    count per family (tests/test_glalign_cases.py and DESIGN.md §3.18 state the counts)."""
    _poison(poison, monkeypatch)
    fams = TG._cached(("glalign-plants", K), lambda: A.pass_plants(K))
    with TG._bank() as bank:
        for family, plants in fams.items():
            ends = A.ENDS_OF[family]
            flags = TG._cached(("glalign-live", K, family),
                               lambda: A.live(plants, G.dna(), *G.DNA_PEN, ends))
            kept = [p for p, f in zip(plants, flags) if f]
            assert len(kept) >= 3, (K, family, flags)
            for q in {p[0].tobytes(): p[0] for p in kept}.values():
                seqs = [t for qq, t, _ in kept if qq.tobytes() == q.tobytes()]
                pairs = [(0, k) for k in range(len(seqs))]
                want = TG._cached(("glalign-seam-want", K, family, len(q)),
                                  lambda: _want([q], seqs, pairs, G.dna(), G.DNA_PEN, ends, True))
                assert S.lib().swk_glocal_rows(len(q)) == K
                assert all(not w[0][1] & ~S.ALIGN_REVERSE for w in want)  # every one has a path
                bank.load_query(q)
                _both_forms(bank, TG.Batch(seqs), pairs, want, ends, True, (K, family))


# ---- 3. gaps at the boundaries, empty pairs --------------------------------------------------------
def _boundary_case(pen):
    def make():
        rng = np.random.default_rng([359, abs(pen[0]), abs(pen[1])])
        qs, seqs = [], []
        for k in range(60):
            m, L = int(rng.integers(2, 40)), int(rng.integers(0, 50))
            q = rng.integers(0, 4, m).astype(np.uint8)
            t = rng.integers(0, 4, L).astype(np.uint8)
            if k % 4 == 0:    # the target lacks the query's first or last rows
                t = np.concatenate([q[3:], rng.integers(0, 4, 4)]) if k % 8 else q[:-3]
            elif k % 4 == 1:  # the query lacks the target's first or last columns (TARGET)
                t = np.concatenate([rng.integers(0, 4, 3), q[m // 2:]]) if k % 8 == 1 else \
                    np.concatenate([q[:m // 2 + 1], rng.integers(0, 4, 2)])
            elif k % 4 == 2:  # nothing in common
                q, t = np.full(m, 2, np.uint8), np.full(min(L, 6), 1, np.uint8)
            qs.append(q)
            seqs.append((SC.revcomp(t) if k % 3 == 0 else t).astype(np.uint8))
        qs.append(rng.integers(0, 4, 7).astype(np.uint8))
        seqs.append(np.zeros(0, np.uint8))   # L = 0: empty in every mode
        pairs = [(k, k) for k in range(len(qs))]
        return qs, seqs, pairs, {e: _want(qs, seqs, pairs, G.dna(), pen, e, True) for e in G.MODES}
    return TG._cached(("glalign-boundary", pen), make)


@POISON
@pytest.mark.parametrize("pen", [G.DNA_PEN, (0, 0), (0, -3)], ids=str)
def test_gaps_at_the_boundaries_and_empty_pairs(pen, poison, monkeypatch):
    """61 pairs of a query set, each query against its own target: records whose first op is I,
    whose last op is I, under TARGET whose first or last op is D, a BOTH pair with no M at all,
    and empty pairs of each kind (SW_END_NONE under QUERY and TARGET with L > 0 and with L = 0,
    L = 0 under BOTH) with the boundary's score."""
    _poison(poison, monkeypatch)
    qs, seqs, pairs, want = _boundary_case(pen)
    first = {e: {w[1][0] & 15 for w in want[e] if w[1]} for e in G.MODES}
    last = {e: {w[1][-1] & 15 for w in want[e] if w[1]} for e in G.MODES}
    assert A.OP_I in first[A.QUERY] and A.OP_I in last[A.QUERY]
    assert A.OP_D in first[A.TARGET] and A.OP_D in last[A.TARGET]
    if pen == (0, 0):
        assert any(w[1] and all(op & 15 for op in w[1]) for w in want[A.BOTH])  # no M at all
    for e in (A.QUERY, A.TARGET):
        empty = [len(t) for w, t in zip(want[e], seqs) if w[0][1] & S.ALIGN_EMPTY]
        assert 0 in empty
        # (a target all against gaps beats one aligned residue only where a gap costs nothing)
        assert any(L > 0 for L in empty) or (e == A.TARGET and pen[0] < 0)
    assert want[A.BOTH][-1][0] == (sum(pen) + 6 * pen[1], S.ALIGN_EMPTY, 0, 0, 0, 0, 0, 0)
    if pen == G.DNA_PEN:
        assert want[A.QUERY][-1][0][0] == -16 - 4 * 6 and want[A.TARGET][-1][0][0] == 0
    bt = TG.Batch(seqs)
    with TG._bank("dna", pen) as bank:
        bank.load_queries(qs)
        for ends in G.MODES:
            _both_forms(bank, bt, pairs, want[ends], ends, True, (pen, ends))


# ---- 4. ties ----------------------------------------------------------------------------------------
@POISON
@pytest.mark.parametrize("pen", [(0, 0), (0, -3)], ids=str)
def test_tie_rich_pairs(pen, poison, monkeypatch):
    """Two-letter pairs at (0, 0) and (0, -3): the model counts path cells with a co-optimal
    diagonal/gap, left/up and open/extend alternative, each count above zero, and the ops are
    the model's op for op."""
    _poison(poison, monkeypatch)
    made = A.tie_pairs()
    qs, seqs = [q for q, _ in made], [t for _, t in made]
    pairs = [(k, k) for k in range(len(qs))]
    bt = TG.Batch(seqs)
    with TG._bank("dna", pen) as bank:
        bank.load_queries(qs)
        for ends in G.MODES:
            def make():
                full = [A.c_align(qs[k], seqs[k], G.dna(), *pen, ends, True, ties=True)
                        for k in range(len(qs))]
                return [w[:2] for w in full], np.sum([w[2] for w in full], axis=0)
            want, ties = TG._cached(("glalign-ties", pen, ends), make)
            assert (ties > 0).all(), (pen, ends, ties)
            _both_forms(bank, bt, pairs, want, ends, True, (pen, ends))


# ---- 5. an asymmetric matrix ------------------------------------------------------------------------
@POISON
@pytest.mark.parametrize("ends", G.MODES)
def test_asymmetric_matrix(ends, poison, monkeypatch):
    """glocal_cases.asym_case on both strands: the transposed matrix changes a majority of the
    model's records, so a kernel (or a profile) reading s(t, q) cannot pass."""
    _poison(poison, monkeypatch)
    q, seqs = G.asym_case()
    sub = SEAMS.MATRICES[G.ASYM]()
    pairs = [(0, k) for k in range(len(seqs))]

    def make():
        want = _want([q], seqs, pairs, sub, G.ASYM_PEN, ends, True)
        wrong = _want([q], seqs, pairs, np.ascontiguousarray(sub.T), G.ASYM_PEN, ends, True)
        return want, sum(a != b for a, b in zip(want, wrong))
    want, moved = TG._cached(("glalign-asym", ends), make)
    assert 2 * moved > len(seqs)
    with TG._bank(G.ASYM, G.ASYM_PEN) as bank:
        bank.load_query(q)
        _both_forms(bank, TG.Batch(seqs), pairs, want, ends, True, ends)


# ---- 6. pair layouts --------------------------------------------------------------------------------
def _set_case():
    qs, seqs, _ = TG._set_case()
    return qs, seqs[:30]


@POISON
@pytest.mark.parametrize("layout", ["list", "top", "best"])
def test_pair_layouts(layout, poison, monkeypatch):
    """Three queries: a scrambled pair list with repeats; the nq x k layout of top_hits_device
    with sentinel tails; the one-entry-per-target layout of best_queries_device with
    SW_QUERY_NONE entries.  Sentinel slots are fully defined, and nothing of the batch is read
    for them: their targets' offsets point far outside the residues."""
    _poison(poison, monkeypatch)
    qs, seqs = _set_case()
    n, k = len(seqs), 5
    rng = np.random.default_rng(367)
    if layout == "list":
        pairs = [(int(rng.integers(0, 3)), int(rng.integers(0, n))) for _ in range(40)]
        pairs[7] = pairs[3]
        pairs[11] = (QUERY_NONE, 2)
        pairs[19] = (1, HIT_NONE)
    elif layout == "top":
        pairs = [(i, int(rng.integers(0, n)) if x < (5, 2, 0)[i] else HIT_NONE)
                 for i in range(3) for x in range(k)]
    else:
        pairs = [(QUERY_NONE if t % 4 == 1 else int(rng.integers(0, 3)), t) for t in range(n)]
    ids = np.arange(n, dtype=np.uint64) * 3 + 100
    bt = TG.Batch(seqs)
    wants = {}
    with TG._bank() as bank:
        bank.load_queries(qs)
        for ends in G.MODES:
            wants[ends] = TG._cached(("glalign-layout", layout, ends), lambda: _want(
                qs, seqs, pairs, G.dna(), G.DNA_PEN, ends, True))
            _both_forms(bank, bt, pairs, wants[ends], ends, True, (layout, ends), layout=layout,
                        k=k, ids=ids)
    if layout == "best":  # the targets no pair names are never read
        offs = bt.offs.copy()
        offs[[t for i, t in pairs if i == QUERY_NONE]] = 1 << 60
        far = TG.Batch(packed=(bt.res, offs, bt.lens))
        with TG._bank() as bank:
            bank.load_queries(qs)
            _check(_device(bank, far, pairs, A.TARGET, True, 400, layout=layout),
                   wants[A.TARGET], pairs, "unread")


# ---- 7. the read-mapping chain ----------------------------------------------------------------------
@POISON
def test_read_mapping_chain_on_one_stream(poison, monkeypatch):
    """score_glocal_device(ENDS_TARGET, both strands) -> best_queries_device ->
    align_glocal_hits_device(d_hit_queries = the best queries) on one stream with no host step:
    every record's score, end and strand are the score call's outputs for its pair, and the
    records are the model's."""
    _poison(poison, monkeypatch)
    torch = TG._torch()
    dev = torch.device("cuda", 0)
    qs, seqs, wsearch = TG._set_case()      # three references as queries, 70 reads as the batch
    n, nq, stride = len(seqs), 3, 700
    bt = TG.Batch(seqs)
    stream = torch.cuda.Stream()
    with TG._bank() as bank:
        bank.load_queries(qs)
        d_sc = torch.full((nq * n,), FILL32, dtype=torch.int32, device=dev)
        d_ep = torch.full((nq * n,), FILL32, dtype=torch.int32, device=dev)
        d_sd = TG._filled(nq * n)
        d_bq = torch.full((n,), FILL32, dtype=torch.int32, device=dev)
        d_out = TG._filled(n * S.ALIGNMENT_DTYPE.itemsize)
        d_cig = torch.full((n * stride,), FILL32, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_glocal_device(*bt.ptrs(), n, bt.max_len, G.TARGET, d_sc.data_ptr(),
                                 d_end_pos=d_ep.data_ptr(), d_strands=d_sd.data_ptr(),
                                 both_strands=True, stream=h)
        bank.best_queries_device(d_sc.data_ptr(), n, nq, d_best_query=d_bq.data_ptr(), stream=h)
        bank.align_glocal_hits_device(*bt.ptrs(), n, bt.max_len, G.TARGET, n, d_out.data_ptr(),
                                      both_strands=True, d_hit_queries=d_bq.data_ptr(),
                                      d_cigar=d_cig.data_ptr(), cigar_stride=stride, stream=h)
        bank.sync()
        stream.synchronize()
    sc = d_sc.cpu().numpy().reshape(nq, n)
    ep = d_ep.cpu().numpy().view(np.uint32).reshape(nq, n)
    sd = d_sd.cpu().numpy().reshape(nq, n)
    bq = d_bq.cpu().numpy().view(np.uint32)
    got = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                            d_cig.cpu().numpy().view(np.uint32))
    assert np.array_equal(sc, wsearch[G.TARGET][0])
    pairs = [(int(bq[t]), t) for t in range(n)]
    for t, a in enumerate(got):
        i = int(bq[t])
        assert a.score == int(sc[i, t]) and a.reverse == bool(sd[i, t])
        assert (a.q_end == int(ep[i, t])) if not a.empty else int(ep[i, t]) == G.END_NONE
    _check(got, _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, G.TARGET, True), pairs, "chain")
    assert sum(a.has_path for a in got) >= 40 and any(a.reverse for a in got)


# ---- 8. the budget and the CIGAR space ----------------------------------------------------------------
@POISON
def test_budget_chunks_and_cigar_space(poison, monkeypatch):
    """SWBANK_ALIGN_MB = 1: the host form plans several chunks from the windows, the device form
    from its slots, with identical records.  A cigar_stride or a cigar_cap too small for a path
    gives SW_ALIGN_NO_PATH with exact coordinates."""
    _poison(poison, monkeypatch)
    monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
    q, packed, pairs, want = _shape_case("dna", 513)
    w = want[A.QUERY, True]
    bt = TG.Batch(packed=packed)
    K = 16
    windows = [((r[3] - r[2] + 1), (r[5] - r[4] + 1)) for r, ops in w if ops]
    need = sum((c + (rows + K - 1) // K - 1) * (K // 4) * 64 for rows, c in windows)
    assert need > 2 * (1 << 18)  # dwords: more than two budgets' worth
    with TG._bank() as bank:
        bank.load_query(q)
        got = _host(bank, (bt.res, bt.offs, bt.lens), pairs, A.QUERY, True)
        _check(got, w, pairs, "host chunks")
        chunks = int(bank.last_kernel().split("chunks=")[1])
        assert chunks >= 3
        stride = max(len(x[1]) for x in w) + 1
        _check(_device(bank, bt, pairs, A.QUERY, True, stride), w, pairs, "device chunks")
        slot = (bt.max_len + (513 + K - 1) // K - 1) * (K // 4) * 64
        per = (1 << 18) // slot
        assert bank.last_kernel().endswith(f"chunks={-(-len(pairs) // per)}") and per < len(pairs)
        # too little CIGAR space
        longest = max(len(x[1]) for x in w)
        assert longest >= 3
        cut = [A.c_align(q, packed[0][int(o):int(o) + int(n)], G.dna(), *G.DNA_PEN, A.QUERY, True,
                         cap=longest - 1) for o, n in zip(packed[1], packed[2])]
        assert any(x[0][1] & S.ALIGN_NO_PATH for x in cut)
        _check(_device(bank, bt, pairs, A.QUERY, True, longest - 1), cut, pairs, "small stride")
        coords = _device(bank, bt, pairs, A.QUERY, True, 0, cigar=False)
        for a, x in zip(coords, w):
            assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == \
                (x[0][0],) + x[0][2:6] and (a.empty or a.flags & S.ALIGN_NO_PATH) and not a.ops
        # the host form packs in hit order: a cap one short of everything drops the last path
        total = sum(len(x[1]) for x in w)
        short = _host(bank, (bt.res, bt.offs, bt.lens), pairs, A.QUERY, True, cigar_cap=total - 1)
        lastp = max(h for h, x in enumerate(w) if x[1])
        for h, (a, x) in enumerate(zip(short, w)):
            if h == lastp:
                assert a.flags == x[0][1] | S.ALIGN_NO_PATH and not a.ops
                assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns) == \
                    (x[0][0],) + x[0][2:6] + (0,)
            else:
                assert tuple(a.ops) == x[1] and a.flags == x[0][1]


# ---- 9. one long target -------------------------------------------------------------------------------
@POISON
def test_one_long_target_on_the_reverse_strand(poison, monkeypatch):
    """One QUERY hit planted near the far end of a 70,000-code target, on the reverse strand: pass
    B walks 69,000 columns back and stops at the window; the direction store is the window's."""
    _poison(poison, monkeypatch)
    rng = np.random.default_rng(373)
    q = rng.integers(0, 4, 250).astype(np.uint8)
    long = rng.integers(0, 4, 70000).astype(np.uint8)
    long[69001:69249] = np.delete(q, [100, 101])
    seqs = [rng.integers(0, 4, 90).astype(np.uint8), SC.revcomp(long)]
    pairs = [(0, 1), (0, 0)]
    want = TG._cached("glalign-long", lambda: _want([q], seqs, pairs, G.dna(), G.DNA_PEN, A.QUERY,
                                                    True))
    rec, ops = want[0]
    assert rec[1] == S.ALIGN_REVERSE and (rec[4], rec[5]) == (70000 - 1 - 69248, 70000 - 1 - 69001)
    assert len(ops) == 3 and ops[1] == (2 << 4 | A.OP_I) and rec[6:] == (250, 248)
    with TG._bank() as bank:
        bank.load_query(q)
        _both_forms(bank, TG.Batch(seqs), pairs, want, A.QUERY, True, "long")


# ---- 10. refusals -------------------------------------------------------------------------------------
def test_refusals_in_the_headers_order():
    """Both forms refuse in the header's order and write nothing: the device outputs and the host
    outputs keep their fill, and the bank stays usable."""
    qs, seqs = _set_case()
    bt = TG.Batch(seqs[:8])
    host = (bt.res, bt.offs, bt.lens)
    torch = TG._torch()
    out = torch.full((1 << 12,), FILL32, dtype=torch.int32, device=torch.device("cuda", 0))
    p = out.data_ptr()
    hq = np.zeros(8, np.uint32)
    hrec = np.full(8 * S.ALIGNMENT_DTYPE.itemsize, 0x3C, np.uint8)
    hcig = np.full(4096, FILL32, np.uint32)
    P = G._p

    def dev(bank, ends=A.QUERY, both=False, res=None, n_hits=8, hpq=8, hitq=0, stride=64,
            max_len=None, d_out=p):
        b = bt.ptrs() if res is None else res
        return S.lib().sw_align_glocal_hits_device(
            bank._h, b[0] or None, b[1] or None, b[2] or None, None, bt.n,
            bt.max_len if max_len is None else max_len, ends, int(both), hitq or None, hpq, None,
            n_hits, d_out or None, p + 4096, stride, None)

    def hst(bank, ends=A.QUERY, both=False, batch=host, n_hits=8, hpq=0, hitq=hq):
        used = np.zeros(1, np.uint64)
        st = S.lib().sw_align_glocal_hits(
            bank._h, P(batch[0]), batch[0].size, P(batch[1]), P(batch[2]), None, bt.n, ends,
            int(both), P(hitq) if hitq is not None else None, hpq, None, n_hits, P(hrec), P(hcig),
            hcig.size, P(used))
        assert st == 0 or ((hrec == 0x3C).all() and (hcig == FILL32).all() and used[0] == 0)
        return st

    def forms(bank, **kw):  # (the device form: hits_per_query = 8; the host form: hit_queries)
        return {dev(bank, **kw), hst(bank, **kw)}

    pq = np.arange(20, dtype=np.uint8)
    # 1. both_strands on a protein bank: merged gaps, a bad ends and no query behind it
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_MERGED) as bank:
        bank.set_matrix(O.BLOSUM62, *G.PROT_PEN)
        assert forms(bank, ends=0, both=True) == {S.ERR_UNSUPPORTED}
        assert forms(bank, ends=0) == {S.ERR_UNSUPPORTED}      # 2. the gap model
        bank.load_query(pq)
        assert forms(bank) == {S.ERR_UNSUPPORTED}
    with S.ScoreBank(gap_model=O.GAP_GOTOH) as bank:
        for bad in (0, 4, -1):                                     # 3. ends
            assert forms(bank, ends=bad) == {S.ERR_ARG}
        assert forms(bank) == {S.ERR_STATE}                      # 4. the state
        bank.set_penalties(5, -4, -12, -4)
        assert forms(bank) == {S.ERR_STATE}
        rng = np.random.default_rng(379)                           # 5. the query length
        bank.load_query(rng.integers(0, 4, S.GLOCAL_MAX_QUERY + 1).astype(np.uint8))
        assert forms(bank) == {S.ERR_UNSUPPORTED}
        assert dev(bank, res=(0, 0, 0)) == S.ERR_UNSUPPORTED       # (NULL buffers behind it)
        bank.load_queries(qs)
        assert forms(bank, n_hits=0, ends=A.BOTH) == {0}           # 6. no hits: nothing to do
        assert dev(bank, res=(0, 0, 0)) == S.ERR_ARG               # 7. NULL buffers
        assert dev(bank, d_out=0) == S.ERR_ARG
        assert S.lib().sw_align_glocal_hits(bank._h, P(host[0]), host[0].size, P(host[1]),
                                            P(host[2]), None, bt.n, 1, 0, P(hq), 0, None, 8, None,
                                            None, 0, None) == S.ERR_ARG
        # 8. the pair list: both hit_queries and hits_per_query, or neither; too many hits
        d_hq = TG._to_dev(hq)
        assert dev(bank, hitq=d_hq.data_ptr(), hpq=8) == S.ERR_ARG
        assert dev(bank, hpq=0) == S.ERR_ARG
        assert hst(bank, hpq=1) == S.ERR_ARG and hst(bank, hitq=None) == S.ERR_ARG
        assert dev(bank, n_hits=9, hpq=9) == S.ERR_ARG             # no hit list: n_hits > n
        assert hst(bank, hitq=np.full(8, 3, np.uint32)) == S.ERR_ARG   # a query >= nq (host)
        # 9. n_hits x cigar_stride
        assert dev(bank, stride=1 << 30) == S.ERR_ARG
        # 10. the listed targets (host), then the range rule
        bad = bt.res.copy()
        bad[int(bt.offs[5]) + 1] = 5
        assert hst(bank, batch=(bad, bt.offs, bt.lens)) == S.ERR_ARG
        outside = bt.lens.copy()
        outside[7] += len(bt.res)
        assert hst(bank, batch=(bt.res, bt.offs, outside)) == S.ERR_ARG
        assert dev(bank, max_len=1 << 23) == S.ERR_RANGE
        bank.sync()
        assert (out.cpu().numpy() == FILL32).all()                 # the device outputs keep their fill
        pairs = [(0, k) for k in range(8)]
        _check(_host(bank, host, pairs, A.QUERY, True), _want(
            qs, seqs, pairs, G.dna(), G.DNA_PEN, A.QUERY, True), pairs, "usable")
    with TG._bank("dna", (0, -32757)) as bank:                     # the range rule, host form
        bank.load_query(qs[0])
        long = TG.Batch([np.zeros(40000, np.uint8)])
        used = np.zeros(1, np.uint64)
        assert S.lib().sw_align_glocal_hits(
            bank._h, P(long.res), long.res.size, P(long.offs), P(long.lens), None, 1, 1, 0, None, 1,
            None, 1, P(hrec), P(hcig), hcig.size, P(used)) == S.ERR_RANGE
        assert (hrec == 0x3C).all() and (hcig == FILL32).all()


def test_timing_brackets_and_a_multi_device_bank():
    """Under set_timing the end / start passes and the path passes are one launch group each; a
    multi-device bank runs the call on its root with the same records."""
    qs, seqs = _set_case()
    pairs = [(k % 3, k) for k in range(len(seqs))]
    want = _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, A.TARGET, True)
    bt = TG.Batch(seqs)
    with TG._bank() as bank:
        bank.load_queries(qs)
        bank.set_timing(True)
        _check(_device(bank, bt, pairs, A.TARGET, True, 700), want, pairs, "timed")
        launches, _, ms = bank.timing()
        assert launches == 2 and ms > 0
        _device(bank, bt, pairs, A.TARGET, True, 0, cigar=False)
        assert bank.timing()[0] == 1
    with TG._bank(devices=[0, 0]) as bank:
        bank.load_queries(qs)
        _both_forms(bank, bt, pairs, want, A.TARGET, True, "multi", chunks=None)
