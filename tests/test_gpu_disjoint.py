"""Non-intersecting local alignments on the GPU (include/swbank.h "non-intersecting local
alignments").  Every test compares sw_align_disjoint_hits[_device] exactly, record
fields and ops of every round, with the C model of tests/disjoint_cases.py (itself checked against
the plain-Python restatement by tests/test_disjoint_cases.py), through the host form's plan and
through the device form's slots, plain and with poisoned buffers: the kernel's three row counts and
the targets' edges, planted copies and an internal repeat, the lane, block, row and column seams,
hit lists and query sets, the chain from the score call, the budget and the CIGAR space, min_score,
a protein bank, one long target, a multi-device bank, the cross-checks against the existing calls,
the refusals and the reports.  The CPU references are computed once per process and shared."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import disjoint_cases as D
import glocal_cases as G
import seam_cases as SEAMS
import test_gpu_glocal as TG

pytestmark = pytest.mark.gpu

QLENS = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024]
TLENS = [0, 1, 63, 64, 65, 129, 290, 301, 333]
HIT_NONE, QUERY_NONE = S.HIT_NONE, S.QUERY_NONE
FILL32 = TG.FILL32
REC = S.ALIGNMENT_DTYPE.itemsize
POISON = pytest.mark.parametrize("poison", ["plain", "poison"])


def _poison(poison, monkeypatch):
    if poison == "poison":
        monkeypatch.setenv("SWBANK_POISON", "1")


def _error(bank):
    return S.lib().sw_last_error(bank._h).decode()


def _want(qs, seqs, pairs, sub, pen, rounds, min_score=1, cap=None):
    """Per pair (query, target) the C model's `rounds` (record, ops); None: the slot names no pair."""
    return [None if i == QUERY_NONE or k == HIT_NONE else
            D.c_rounds(qs[i], seqs[k], sub, *pen, rounds, min_score, cap=cap) for i, k in pairs]


def _check(got, want, pairs, rounds, what, ids=None):
    assert len(got) == len(want) == len(pairs)
    for h, (hit, w, (i, k)) in enumerate(zip(got, want, pairs)):
        assert len(hit) == rounds
        for r, a in enumerate(hit):
            if w is None:  # all the rounds of a sentinel slot are fully defined
                assert (a.index, a.id, a.score, a.flags, a.ops) == \
                    (HIT_NONE, HIT_NONE, 0, S.ALIGN_EMPTY | S.ALIGN_NO_HIT, ()), (what, h, r, a)
                assert (a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns,
                        a.n_identities) == (0,) * 6
                continue
            rec = (a.score, a.flags, a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns,
                   a.n_identities)
            assert (rec, tuple(a.ops)) == w[r], (what, h, r, i, k, rec, D.cigar(a.ops), w[r][0],
                                                 D.cigar(w[r][1]))
            assert a.index == k and a.id == (k if ids is None else int(ids[k])), (what, h, r)


def _lists(pairs, layout, k):
    hq = np.array([i for i, _ in pairs], np.uint32)
    hv = np.array([t for _, t in pairs], np.uint64)
    if layout == "top":       # the nq x k layout of top_hits_device
        return dict(hits=hv, hits_per_query=k)
    if layout == "best":      # one entry per target, as best_queries_device writes
        return dict(hit_queries=hq)
    return dict(hits=hv, hit_queries=hq)


def _host(bank, packed, pairs, rounds, min_score=1, layout="list", cigar_cap=None, ids=None, k=0):
    return bank.align_disjoint_hits(*packed, rounds, min_score=min_score, cigar_cap=cigar_cap,
                                    ids=ids, **_lists(pairs, layout, k))


def _device(bank, bt, pairs, rounds, stride, min_score=1, layout="list", ids=None, k=0, cigar=True,
            stream=0, max_len=None):
    torch = TG._torch()
    n_hits = len(pairs)
    kw = _lists(pairs, layout, k)
    keep = {name: TG._to_dev(kw[name]) for name in ("hits", "hit_queries") if name in kw}
    d_ids = TG._to_dev(np.asarray(ids, np.uint64)) if ids is not None else None
    d_out = TG._filled(n_hits * rounds * REC)
    d_cig = torch.full((max(1, n_hits * rounds * stride),), FILL32, dtype=torch.int32,
                       device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    bank.align_disjoint_hits_device(
        *bt.ptrs(), bt.n, bt.max_len if max_len is None else max_len, rounds, n_hits,
        d_out.data_ptr(), min_score=min_score,
        d_hits=keep["hits"].data_ptr() if "hits" in keep else 0,
        d_hit_queries=keep["hit_queries"].data_ptr() if "hit_queries" in keep else 0,
        hits_per_query=kw.get("hits_per_query", 0),
        d_cigar=d_cig.data_ptr() if cigar else 0, cigar_stride=stride, stream=stream,
        d_ids=d_ids.data_ptr() if d_ids is not None else 0)
    bank.sync()
    rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
    if cigar and stride:
        assert [int(r["cigar_offset"]) for r in rec] == [x * stride for x in range(n_hits * rounds)]
    flat = S.alignments_from(rec, d_cig.cpu().numpy().view(np.uint32))
    return [flat[h * rounds:(h + 1) * rounds] for h in range(n_hits)]


def _stride(want):
    return max([len(ops) for w in want if w is not None for _, ops in w] + [0]) + 1


def _both_forms(bank, bt, pairs, want, rounds, what, min_score=1, stride=None, chunks=1, **kw):
    """The host form's plan and the device form's slots against the model."""
    _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, rounds, min_score, **kw), want, pairs,
           rounds, (what, "host"), kw.get("ids"))
    if chunks is not None:
        assert bank.last_kernel() == f"align-disjoint i32 rounds={rounds} " \
            f"nq={max(bank.query_count(), 1)} hits={len(pairs)} chunks={chunks}"
    _check(_device(bank, bt, pairs, rounds, stride or _stride(want), min_score, **kw), want, pairs,
           rounds, (what, "device"), kw.get("ids"))


# ---- 1. shapes ------------------------------------------------------------------------------------
def _shape_case(name, m):
    """A query of m rows against 18 targets whose lengths walk through TLENS: random codes with up
    to three noisy copies of a query window where they fit."""
    def make():
        matrix, pen = TG.SETS3[name]
        sub = SEAMS.MATRICES[matrix]()
        letters = 4 if sub.shape[0] == 5 else 20
        rng = np.random.default_rng([421, m, letters])
        q = rng.integers(0, letters, m).astype(np.uint8)
        seqs = []
        for x in range(2 * len(TLENS)):
            L = TLENS[x % len(TLENS)]
            t = rng.integers(0, letters, L).astype(np.uint8)
            at = 0
            for c in range(3):
                a = int(rng.integers(0, max(1, m - 8)))
                w = q[a:a + int(rng.integers(8, 90))].copy()
                if c == 1 and len(w) > 4:
                    w[len(w) // 2] = (int(w[len(w) // 2]) + 1) % letters
                if c == 2 and len(w) > 6:
                    w = np.delete(w, len(w) // 3) if x % 2 else np.insert(w, len(w) // 3, w[0])
                at += int(rng.integers(0, 9))
                if x >= len(TLENS) and at + len(w) <= L:
                    t[at:at + len(w)] = w
                    at += len(w)
            seqs.append(t)
        pairs = [(0, k) for k in range(len(seqs))]
        return q, seqs, pairs, _want([q], seqs, pairs, sub, pen, 3)
    return TG._cached(("disjoint-shape", name, m), make)


@POISON
@pytest.mark.parametrize("name", list(TG.SETS3))
def test_query_rows_and_target_edges(name, poison, monkeypatch):
    """Queries of 1, 2 and 3 rows and each side of 256, 512 and 1,024 rows against targets of 0, 1,
    63, 64, 65, 129 and about 300 codes, three rounds; DNA 5 / -4 at -12 / -4 and BLOSUM62 at
    -11 / -1.  Round-0 scores are score_batch's on the same bank, and round-0 ends are
    align_set_hits's."""
    _poison(poison, monkeypatch)
    matrix, pen = TG.SETS3[name]
    depth = set()
    with TG._bank(matrix, pen) as bank:
        for m in QLENS:
            q, seqs, pairs, want = _shape_case(name, m)
            bt = TG._cached(("disjoint-shape-batch", name, m), lambda: TG.Batch(seqs))
            assert set(TLENS) == set(bt.lens.tolist())
            bank.load_query(q)
            _both_forms(bank, bt, pairs, want, 3, (name, m))
            depth |= {sum(1 for rec, _ in w if not rec[1] & D.EMPTY) for w in want}
            sc = bank.score_batch(bt.res, bt.offs, bt.lens)
            assert sc.tolist() == [w[0][0][0] for w in want], (name, m)
            if poison == "plain":
                ends = bank.align_set_hits(bt.res, bt.offs, bt.lens, hits_per_query=len(seqs))
                assert [(a.score, a.q_end, a.t_end) for a in ends] == \
                    [(w[0][0][0], w[0][0][3], w[0][0][5]) for w in want], (name, m)
    assert {0, 3} <= depth  # empty pairs, and pairs three alignments deep


# ---- 2. plants ------------------------------------------------------------------------------------
@POISON
def test_planted_copies_and_an_internal_repeat(poison, monkeypatch):
    """Three copies of a query window between N flanks (exact, a substitution, an indel) come back
    in score order in rounds 0 to 2, and round 3 is empty at a min_score between; a query with an
    internal repeat against a target that holds the unit once reuses the target range with
    another query range in round 1 (asserted on the model in tests/test_disjoint_cases.py)."""
    _poison(poison, monkeypatch)
    q, t, _ = D.copies_case()
    want = _want([q], [t], [(0, 0)], G.dna(), G.DNA_PEN, 4, min_score=200)
    sc = D.scores(want[0])
    assert sc[0] > sc[1] > sc[2] > 200 and want[0][3] == D.EMPTY_REC
    q2, t2 = D.repeat_case()
    want2 = _want([q2], [t2], [(0, 0)], G.dna(), G.DNA_PEN, 2)
    (r0, _), (r1, _) = want2[0]
    assert r0[0] == r1[0] and r0[4:6] == r1[4:6] and r0[2:4] != r1[2:4]
    with TG._bank() as bank:
        bank.load_query(q)
        _both_forms(bank, TG.Batch([t]), [(0, 0)], want, 4, "copies", min_score=200)
        bank.load_query(q2)
        _both_forms(bank, TG.Batch([t2]), [(0, 0)], want2, 2, "repeat")


# ---- 3. seams -------------------------------------------------------------------------------------
@POISON
@pytest.mark.parametrize("K", D.ROWS)
def test_lane_block_row_and_column_seams(K, poison, monkeypatch):
    """disjoint_cases.seam_plants for queries of 64K - 3 rows: a gap run across a lane seam and
    across a 64-step block seam (the model's mutants 1 and 2 lose F and E there), and an island
    whose path crosses row K l or column 64 b (mutants 3 and 4 forget the used cells there and
    find that cell again in round 1).  A plant counts only if its mutant changes a model score;
    at least 3 of 4 count per family (tests/test_disjoint_cases.py states why)."""
    _poison(poison, monkeypatch)
    fams = TG._cached(("disjoint-plants", K), lambda: D.seam_plants(K))
    with TG._bank() as bank:
        for family, plants in fams.items():
            flags = TG._cached(("disjoint-live", K, family),
                               lambda: D.live(plants, G.dna(), *G.DNA_PEN))
            kept = [p for p, f in zip(plants, flags) if f]
            assert len(kept) >= 3, (K, family, flags)
            qs = [p[0] for p in kept]
            seqs = [p[1] for p in kept]
            pairs = [(k, k) for k in range(len(kept))]
            want = TG._cached(("disjoint-seam-want", K, family),
                              lambda: _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, 3))
            assert all(S.lib().swk_glocal_rows(len(q)) == K for q in qs)
            bank.load_queries(qs)
            _both_forms(bank, TG.Batch(seqs), pairs, want, 3, (K, family))


# ---- 4. hit lists and query sets ------------------------------------------------------------------
def _set_case():
    def make():
        rng = np.random.default_rng(431)
        qs = [rng.integers(0, 4, m).astype(np.uint8) for m in (1, 37, 300, 513)]
        seqs = []
        for k in range(40):
            q = qs[1 + k % 3]
            w = q[: int(rng.integers(20, 80))]
            parts = [rng.integers(0, 4, int(rng.integers(0, 12))), w,
                     rng.integers(0, 4, int(rng.integers(1, 9))),
                     np.delete(w, len(w) // 2) if k % 2 else w]
            seqs.append(np.concatenate(parts).astype(np.uint8) if k % 7 != 6 else
                        rng.integers(0, 5, int(rng.integers(0, 60))).astype(np.uint8))
        return qs, seqs
    return TG._cached("disjoint-set", make)


@POISON
@pytest.mark.parametrize("n_hits", [1, 63, 64, 65, 130])
def test_hit_lists(n_hits, poison, monkeypatch):
    """A set with queries of 1, 37, 300 and 513 rows: a scrambled pair list with one pair listed
    twice, whose two slots must be equal (slots do not share a store), and sentinel slots."""
    _poison(poison, monkeypatch)
    qs, seqs = _set_case()
    rng = np.random.default_rng([433, n_hits])
    pairs = [(int(rng.integers(0, 4)), int(rng.integers(0, len(seqs)))) for _ in range(n_hits)]
    if n_hits > 8:
        pairs[7] = pairs[3] = (2, 5)
        pairs[5] = (QUERY_NONE, 2)
        pairs[n_hits - 1] = (1, HIT_NONE)
    ids = np.arange(len(seqs), dtype=np.uint64) * 3 + 100
    want = _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, 3)
    assert n_hits <= 8 or (want[7] == want[3] and sum(s > 0 for s in D.scores(want[3])) >= 2)
    bt = TG._cached("disjoint-set-batch", lambda: TG.Batch(seqs))
    with TG._bank() as bank:
        bank.load_queries(qs)
        _both_forms(bank, bt, pairs, want, 3, n_hits, ids=ids)


@POISON
@pytest.mark.parametrize("layout", ["top", "best"])
def test_pair_layouts(layout, poison, monkeypatch):
    """The nq x k layout of top_hits_device (hits_per_query) with sentinel tails, and the
    one-entry-per-target layout through hit_queries alone."""
    _poison(poison, monkeypatch)
    qs, seqs = _set_case()
    n, k = len(seqs), 4
    rng = np.random.default_rng(439)
    if layout == "top":
        pairs = [(i, int(rng.integers(0, n)) if x < (4, 2, 0, 3)[i] else HIT_NONE)
                 for i in range(4) for x in range(k)]
    else:
        pairs = [(QUERY_NONE if t % 5 == 1 else int(rng.integers(0, 4)), t) for t in range(n)]
    want = _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, 2)
    bt = TG._cached("disjoint-set-batch", lambda: TG.Batch(seqs))
    with TG._bank() as bank:
        bank.load_queries(qs)
        _both_forms(bank, bt, pairs, want, 2, layout, layout=layout, k=k)


@POISON
def test_chain_from_the_score_call_on_one_stream(poison, monkeypatch):
    """score_batch_device -> top_hits_device -> align_disjoint_hits_device on one stream with no
    host step: every round-0 score is the score call's, and the records are the model's."""
    _poison(poison, monkeypatch)
    torch = TG._torch()
    dev = torch.device("cuda", 0)
    qs, seqs = _set_case()
    n, nq, k, rounds, stride = len(seqs), 4, 3, 2, 200
    bt = TG._cached("disjoint-set-batch", lambda: TG.Batch(seqs))
    stream = torch.cuda.Stream()
    with TG._bank() as bank:
        bank.load_queries(qs)
        d_sc = torch.full((nq * n,), FILL32, dtype=torch.int32, device=dev)
        d_hits = TG._filled(nq * k * 8)
        d_out = TG._filled(nq * k * rounds * REC)
        d_cig = torch.full((nq * k * rounds * stride,), FILL32, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_batch_device(*bt.ptrs(), n, bt.max_len, d_sc.data_ptr(), stream=h)
        bank.top_hits_device(d_sc.data_ptr(), n, k, d_hits.data_ptr(), nq=nq, stream=h)
        bank.align_disjoint_hits_device(*bt.ptrs(), n, bt.max_len, rounds, nq * k, d_out.data_ptr(),
                                        d_hits=d_hits.data_ptr(), hits_per_query=k,
                                        d_cigar=d_cig.data_ptr(), cigar_stride=stride, stream=h)
        bank.sync()
        stream.synchronize()
    sc = d_sc.cpu().numpy().reshape(nq, n)
    hits = d_hits.cpu().numpy().view(np.uint64)
    flat = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                             d_cig.cpu().numpy().view(np.uint32))
    got = [flat[x * rounds:(x + 1) * rounds] for x in range(nq * k)]
    pairs = [(x // k, int(hits[x])) for x in range(nq * k)]
    assert all(t < n for _, t in pairs)
    for (i, t), hit in zip(pairs, got):
        assert hit[0].score == int(sc[i, t])
    _check(got, _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, rounds), pairs, rounds, "chain")


# ---- 5. the budget, the CIGAR space, min_score -------------------------------------------------------
@POISON
def test_budget_chunks_and_cigar_space(poison, monkeypatch):
    """SWBANK_ALIGN_MB = 1: both forms run several chunks with the records of the single-chunk
    run.  A slot over the budget is refused and the outputs keep their fill.  A cigar_stride too
    small for round 0 only: that record is SW_ALIGN_NO_PATH and every other record is the
    ample-stride run's.  d_cigar NULL: coordinates only."""
    _poison(poison, monkeypatch)
    q, seqs, pairs, want = _shape_case("dna", 513)
    bt = TG._cached(("disjoint-shape-batch", "dna", 513), lambda: TG.Batch(seqs))
    K, budget = 16, 1 << 18
    with TG._bank() as bank:
        bank.load_query(q)
        monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
        need = [(int(L) + (513 + K - 1) // K - 1) * (K // 4) * 64 if L else 0 for L in bt.lens]
        assert sum(need) > 2 * budget
        _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, 3), want, pairs, 3, "host chunks")
        assert int(bank.last_kernel().split("chunks=")[1]) >= 3
        _check(_device(bank, bt, pairs, 3, _stride(want)), want, pairs, 3, "device chunks")
        per = budget // ((bt.max_len + (513 + K - 1) // K - 1) * (K // 4) * 64)
        assert bank.last_kernel().endswith(f"chunks={-(-len(pairs) // per)}") and per < len(pairs)
        # one slot over the budget
        big = TG.Batch(seqs + [np.zeros(1100, np.uint8)])
        torch = TG._torch()
        d_out = TG._filled(REC * 3)
        one = np.array([len(seqs)], np.uint64)
        hits = TG._to_dev(one)
        hrec = np.full(3 * REC, 0x3C, np.uint8)
        for st in (
            S.lib().sw_align_disjoint_hits_device(
                bank._h, *big.ptrs(), None, big.n, big.max_len, 3, 1, None, 1, hits.data_ptr(), 1,
                d_out.data_ptr(), None, 0, None),
            S.lib().sw_align_disjoint_hits(
                bank._h, G._p(big.res), big.res.size, G._p(big.offs), G._p(big.lens), None, big.n,
                3, 1, None, 1, G._p(one), 1, G._p(hrec), None, 0, None)):
            assert st == S.ERR_UNSUPPORTED and "SWBANK_ALIGN_MB" in _error(bank)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x3C).all() and (hrec == 0x3C).all()
        monkeypatch.delenv("SWBANK_ALIGN_MB")
        # too little CIGAR space for round 0 only
        h = next(h for h, w in enumerate(want) if len(w[0][1]) > max(len(w[1][1]), len(w[2][1]), 1)
                 and w[1][1])
        small = len(want[h][0][1]) - 1
        cut = _want([q], seqs, pairs, G.dna(), G.DNA_PEN, 3, cap=small)
        assert cut[h][0][0][1] == S.ALIGN_NO_PATH and cut[h][1:] == want[h][1:]
        assert cut[h][0][0][:1] + cut[h][0][0][2:6] == want[h][0][0][:1] + want[h][0][0][2:6]
        _check(_device(bank, bt, pairs, 3, small), cut, pairs, 3, "small stride")
        coords = _device(bank, bt, pairs, 3, 0, cigar=False)
        for hit, w in zip(coords, want):
            for a, (rec, _) in zip(hit, w):
                assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == rec[:1] + rec[2:6]
                assert (a.empty or a.flags == S.ALIGN_NO_PATH) and not a.ops
                assert (a.n_columns, a.n_identities) == (0, 0)
        # the host form packs in record order: a cap one short of everything drops the last path
        total = sum(len(ops) for w in want for _, ops in w)
        short = _host(bank, (bt.res, bt.offs, bt.lens), pairs, 3, cigar_cap=total - 1)
        last = max((h, r) for h, w in enumerate(want) for r, (_, ops) in enumerate(w) if ops)
        for h, (hit, w) in enumerate(zip(short, want)):
            for r, (a, (rec, ops)) in enumerate(zip(hit, w)):
                if (h, r) == last:
                    assert a.flags == S.ALIGN_NO_PATH and not a.ops and a.n_columns == 0
                    assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == rec[:1] + rec[2:6]
                else:
                    assert tuple(a.ops) == ops and a.flags == rec[1]


@POISON
def test_min_score_above_the_best_score(poison, monkeypatch):
    """min_score above score_0: every record of every hit is empty."""
    _poison(poison, monkeypatch)
    q, seqs, pairs, want = _shape_case("dna", 257)
    top = max(w[0][0][0] for w in want)
    empty = [[D.EMPTY_REC] * 3 for _ in pairs]
    assert top > 0 and _want([q], seqs, pairs, G.dna(), G.DNA_PEN, 3, min_score=top + 1) == empty
    bt = TG._cached(("disjoint-shape-batch", "dna", 257), lambda: TG.Batch(seqs))
    with TG._bank() as bank:
        bank.load_query(q)
        _both_forms(bank, bt, pairs, empty, 3, "min_score", min_score=top + 1, stride=8)


# ---- 6. one long target, a multi-device bank ----------------------------------------------------------
@POISON
def test_two_copies_at_the_ends_of_a_long_target(poison, monkeypatch):
    """Two copies of a 1,000-row query at the two ends of a 70,000-code target, K = 16, two
    rounds: the exact one at the far end first, the one with a deleted residue second."""
    _poison(poison, monkeypatch)
    rng = np.random.default_rng(443)
    q = rng.integers(0, 4, 1000).astype(np.uint8)
    long = rng.integers(0, 4, 70000).astype(np.uint8)
    long[20:1019] = np.delete(q, 500)
    long[68990:69990] = q
    want = TG._cached("disjoint-long", lambda: _want([q], [long], [(0, 0)], G.dna(), G.DNA_PEN, 2))
    (r0, o0), (r1, o1) = want[0]
    assert r0[:6] == (5000, 0, 0, 999, 68990, 69989) and D.cigar(o0) == "1000M"
    assert r1[0] == 5 * 999 - 16 and r1[4:6] == (20, 1018) and len(o1) == 3
    with TG._bank() as bank:
        bank.load_query(q)
        _both_forms(bank, TG.Batch([long]), [(0, 0)], want, 2, "long")


def test_timing_brackets_and_a_multi_device_bank():
    """Under set_timing the rounds of a chunk are one launch group; a multi-device bank runs the
    call on its root with the same records."""
    qs, seqs = _set_case()
    pairs = [(k % 4, k) for k in range(len(seqs))]
    want = _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, 3)
    bt = TG._cached("disjoint-set-batch", lambda: TG.Batch(seqs))
    with TG._bank() as bank:
        bank.load_queries(qs)
        bank.set_timing(True)
        _check(_device(bank, bt, pairs, 3, _stride(want)), want, pairs, 3, "timed")
        assert bank.last_kernel() == f"align-disjoint i32 rounds=3 nq=4 hits={len(pairs)} chunks=1"
        launches, _, ms = bank.timing()
        assert launches == 1 and ms > 0
    with TG._bank(devices=[0, 0]) as bank:
        bank.load_queries(qs)
        _both_forms(bank, bt, pairs, want, 3, "multi", chunks=None)


# ---- 7. refusals --------------------------------------------------------------------------------------
def test_refusals_in_the_headers_order():
    """Both forms refuse in the header's order and write nothing: the device outputs and the host
    outputs keep their fill, and the bank stays usable."""
    qs, seqs = _set_case()
    qs, seqs = qs[:3], seqs[:8]
    bt = TG.Batch(seqs)
    host = (bt.res, bt.offs, bt.lens)
    torch = TG._torch()
    out = torch.full((1 << 13,), FILL32, dtype=torch.int32, device=torch.device("cuda", 0))
    p = out.data_ptr()
    hq = np.zeros(8, np.uint32)
    hrec = np.full(8 * 2 * REC, 0x3C, np.uint8)
    hcig = np.full(4096, FILL32, np.uint32)
    P = G._p

    def dev(bank, rounds=2, min_score=1, res=None, n_hits=8, hpq=8, hitq=0, stride=64, d_out=p,
            max_len=None):
        b = bt.ptrs() if res is None else res
        return S.lib().sw_align_disjoint_hits_device(
            bank._h, b[0] or None, b[1] or None, b[2] or None, None, bt.n,
            bt.max_len if max_len is None else max_len, rounds, min_score, hitq or None, hpq, None,
            n_hits, d_out or None, p + 16384, stride, None)

    def hst(bank, rounds=2, min_score=1, batch=host, n_hits=8, hpq=0, hitq=hq):
        used = np.zeros(1, np.uint64)
        st = S.lib().sw_align_disjoint_hits(
            bank._h, P(batch[0]), batch[0].size, P(batch[1]), P(batch[2]), None, bt.n, rounds,
            min_score, P(hitq) if hitq is not None else None, hpq, None, n_hits, P(hrec), P(hcig),
            hcig.size, P(used))
        assert st == 0 or ((hrec == 0x3C).all() and (hcig == FILL32).all() and used[0] == 0)
        return st

    def forms(bank, **kw):  # (the device form: hits_per_query = 8; the host form: hit_queries)
        return {dev(bank, **kw), hst(bank, **kw)}

    # 1. the gap model, with nothing loaded and bad arguments behind it
    with S.ScoreBank(gap_model=O.GAP_MERGED) as bank:
        assert forms(bank, rounds=0) == {S.ERR_UNSUPPORTED}
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(qs[1])
        assert forms(bank) == {S.ERR_UNSUPPORTED}
    with S.ScoreBank(gap_model=O.GAP_GOTOH) as bank:
        assert forms(bank, rounds=0) == {S.ERR_STATE}              # 2. the state
        bank.set_penalties(5, -4, -12, -4)
        assert forms(bank) == {S.ERR_STATE}
        rng = np.random.default_rng(449)                           # 3. the query length
        bank.load_query(rng.integers(0, 4, S.DISJOINT_MAX_QUERY + 1).astype(np.uint8))
        assert forms(bank, rounds=0) == {S.ERR_UNSUPPORTED}
        bank.load_queries(qs)
        for bad in (0, S.DISJOINT_MAX_ROUNDS + 1):                 # 4. rounds and min_score
            assert forms(bank, rounds=bad, n_hits=0) == {S.ERR_ARG}
        for bad in (0, -5):
            assert forms(bank, min_score=bad, n_hits=0) == {S.ERR_ARG}
        assert forms(bank, n_hits=0, rounds=S.DISJOINT_MAX_ROUNDS) == {0}   # 7. no hits
        assert dev(bank, res=(0, 0, 0)) == S.ERR_ARG               # 8. NULL buffers
        assert dev(bank, d_out=0) == S.ERR_ARG
        assert S.lib().sw_align_disjoint_hits(bank._h, P(host[0]), host[0].size, P(host[1]),
                                              P(host[2]), None, bt.n, 2, 1, P(hq), 0, None, 8,
                                              None, None, 0, None) == S.ERR_ARG
        # 9. the pair list: both hit_queries and hits_per_query, or neither; too many hits
        d_hq = TG._to_dev(hq)
        assert dev(bank, hitq=d_hq.data_ptr(), hpq=8) == S.ERR_ARG
        assert dev(bank, hpq=0) == S.ERR_ARG
        assert hst(bank, hpq=1) == S.ERR_ARG and hst(bank, hitq=None) == S.ERR_ARG
        assert dev(bank, n_hits=9, hpq=9) == S.ERR_ARG             # no hit list: n_hits > n
        assert hst(bank, hitq=np.full(8, 3, np.uint32)) == S.ERR_ARG   # a query >= nq (host)
        bad = bt.res.copy()                                        # the listed targets (host)
        bad[int(bt.offs[5]) + 1] = 5
        assert hst(bank, batch=(bad, bt.offs, bt.lens)) == S.ERR_ARG
        # 10. n_hits x rounds x cigar_stride
        assert dev(bank, stride=1 << 29) == S.ERR_ARG
        # 11. a slot over the budget
        assert dev(bank, max_len=1 << 20) == S.ERR_UNSUPPORTED
        assert "SWBANK_ALIGN_MB" in _error(bank)
        bank.sync()
        assert (out.cpu().numpy() == FILL32).all()                 # the device outputs keep their fill
        pairs = [(0, k) for k in range(8)]
        _check(_host(bank, host, pairs, 2), _want(qs, seqs, pairs, G.dna(), G.DNA_PEN, 2), pairs, 2,
               "usable")
