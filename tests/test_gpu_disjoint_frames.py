"""Non-intersecting alignments over the six reading frames on the GPU (include/swbank.h
"non-intersecting alignments over reading frames").  Every test compares
sw_align_disjoint_frame_hits[_device] exactly, record fields and ops of every round, with the C
composition of tests/disjoint_frames_cases.py (itself checked against the plain-Python one by
tests/test_disjoint_frames_cases.py), through the host form's plan and through the device form's
slots, plain and with poisoned buffers (outputs, direction store and candidate state): the
kernel's three row counts with exons in three frames, a tie across strands, a frame that wins
twice, the translation's seams under a custom codon table, the min_score cut, hit lists and a
query set, the chain from the six-frame search, the budget and the CIGAR space, the refusals and
the reports.  The CPU references are computed once per process and shared."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import disjoint_cases as D
import disjoint_frames_cases as DF
import frame_cases as FR
import glocal_cases as G
import strand_cases as SC
import test_gpu_disjoint as TD
import test_gpu_glocal as TG

pytestmark = pytest.mark.gpu

HIT_NONE, QUERY_NONE = S.HIT_NONE, S.QUERY_NONE
FILL32 = TG.FILL32
REC = S.ALIGNMENT_DTYPE.itemsize
POISON = TD.POISON
PEN = DF.PEN
ROUNDS, MIN_SCORE = 5, 20


def _bank(**kw):
    return TG._bank("blosum62", PEN, **kw)


def _want(qs, seqs, pairs, rounds, min_score=MIN_SCORE, table=None, cap=None):
    """Per pair (query, target) the model's `rounds` (record, ops); None: the slot names no pair."""
    return [None if i == QUERY_NONE or k == HIT_NONE else
            DF.c_merged(qs[i], seqs[k], O.BLOSUM62, *PEN, rounds, min_score, table, cap=cap)
            for i, k in pairs]


def _host(bank, packed, pairs, rounds, min_score=MIN_SCORE, layout="list", cigar_cap=None,
          ids=None, k=0, table=None):
    return bank.align_disjoint_frame_hits(*packed, rounds, min_score=min_score,
                                          cigar_cap=cigar_cap, ids=ids, codon_table=table,
                                          **TD._lists(pairs, layout, k))


def _device(bank, bt, pairs, rounds, stride, min_score=MIN_SCORE, layout="list", ids=None, k=0,
            cigar=True, stream=0, max_len=None, table=None):
    torch = TG._torch()
    n_hits = len(pairs)
    kw = TD._lists(pairs, layout, k)
    keep = {name: TG._to_dev(kw[name]) for name in ("hits", "hit_queries") if name in kw}
    d_ids = TG._to_dev(np.asarray(ids, np.uint64)) if ids is not None else None
    d_out = TG._filled(n_hits * rounds * REC)
    d_cig = torch.full((max(1, n_hits * rounds * stride),), FILL32, dtype=torch.int32,
                       device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    bank.align_disjoint_frame_hits_device(
        *bt.ptrs(), bt.n, bt.max_len if max_len is None else max_len, rounds, n_hits,
        d_out.data_ptr(), min_score=min_score,
        d_hits=keep["hits"].data_ptr() if "hits" in keep else 0,
        d_hit_queries=keep["hit_queries"].data_ptr() if "hit_queries" in keep else 0,
        hits_per_query=kw.get("hits_per_query", 0),
        d_cigar=d_cig.data_ptr() if cigar else 0, cigar_stride=stride, stream=stream,
        d_ids=d_ids.data_ptr() if d_ids is not None else 0, codon_table=table)
    bank.sync()
    rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
    if cigar and stride:
        assert [int(r["cigar_offset"]) for r in rec] == [x * stride for x in range(n_hits * rounds)]
    flat = S.alignments_from(rec, d_cig.cpu().numpy().view(np.uint32))
    return [flat[h * rounds:(h + 1) * rounds] for h in range(n_hits)]


def _check(got, want, pairs, rounds, what, ids=None):
    """disjoint's comparison, and Alignment.frame; an empty record has no frame bits."""
    TD._check(got, want, pairs, rounds, what, ids)
    for hit, w in zip(got, want):
        for a, x in zip(hit, w or ()):
            assert a.frame == FR.frame_of(x[0][1])
            assert not a.empty or a.flags == S.ALIGN_EMPTY


def _name(bank, rounds, hits, chunks):
    return f"align-disjoint-frames i32 rounds={rounds} nq={max(bank.query_count(), 1)} " \
           f"hits={hits} chunks={chunks}"


def _both_forms(bank, bt, pairs, want, rounds, what, min_score=MIN_SCORE, stride=None, chunks=1,
                **kw):
    """The host form's plan and the device form's slots against the model."""
    _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, rounds, min_score, **kw), want, pairs,
           rounds, (what, "host"), kw.get("ids"))
    if chunks is not None:
        assert bank.last_kernel() == _name(bank, rounds, len(pairs), chunks)
    _check(_device(bank, bt, pairs, rounds, stride or TD._stride(want), min_score, **kw), want,
           pairs, rounds, (what, "device"), kw.get("ids"))
    if chunks is not None:
        assert bank.last_kernel() == _name(bank, rounds, len(pairs), chunks)


# ---- 1. the three row counts: exons in three frames --------------------------------------------------
def _exon_case(m):
    def make():
        q, t = DF.exon_case(m)
        rng = np.random.default_rng([547, m])
        seqs = [t, rng.integers(0, 4, 200).astype(np.uint8), t[:len(t) // 2], t[:4]]
        pairs = [(0, k) for k in range(len(seqs))]
        return q, seqs, pairs, _want([q], seqs, pairs, ROUNDS)
    return TG._cached(("dframes-exons", m), make)


@POISON
@pytest.mark.parametrize("m", [60, 300, 600])
def test_exons_in_three_frames_at_each_row_count(m, poison, monkeypatch):
    """Queries of 60, 300 and 600 residues (4, 8 and 16 rows per lane) whose thirds lie at offsets
    0 and 2 mod 3 and on the reverse strand of one target: the first three records are three
    different frames, one of them reversed; five rounds at min_score 20.  Record 0 has the score
    and the frame of score_frames on the same bank."""
    TD._poison(poison, monkeypatch)
    q, seqs, pairs, want = _exon_case(m)
    fr = DF.frames(want[0])
    assert len(set(fr[:3])) == 3 and max(fr[:3]) >= 3, fr
    assert S.lib().swk_glocal_rows(m) == {60: 4, 300: 8, 600: 16}[m]
    bt = TG._cached(("dframes-exons-batch", m), lambda: TG.Batch(seqs))
    with _bank() as bank:
        bank.load_query(q)
        _both_forms(bank, bt, pairs, want, ROUNDS, m)
        sc, frames = bank.score_frames(bt.res, bt.offs, bt.lens)
        for k, w in enumerate(want):
            rec = w[0][0]
            if sc[k] >= MIN_SCORE:
                assert (rec[0], FR.frame_of(rec[1])) == (int(sc[k]), int(frames[k])), (m, k)
            else:
                assert w[0] == D.EMPTY_REC


# ---- 2. ties and a frame that wins twice ------------------------------------------------------------
@POISON
def test_tie_across_strands_and_the_same_frame_twice(poison, monkeypatch):
    """A peptide on both strands of one target: two equal scores, the lower frame first.  Two
    back-translations of the peptide in one frame: the refreshed candidate of the frame that just
    won wins again."""
    TD._poison(poison, monkeypatch)
    q, t = DF.tie_case()
    want = _want([q], [t], [(0, 0)], 3)
    sc, fr = D.scores(want[0]), DF.frames(want[0])
    assert sc[0] == sc[1] and fr[0] != fr[1] and fr[0] < fr[1]
    q2, t2 = DF.twice_case()
    want2 = _want([q2], [t2], [(0, 0)], 3)
    fr2 = DF.frames(want2[0])
    assert fr2[0] == fr2[1]
    with _bank() as bank:
        bank.load_query(q)
        _both_forms(bank, TG.Batch([t]), [(0, 0)], want, 3, "tie")
        bank.load_query(q2)
        _both_forms(bank, TG.Batch([t2]), [(0, 0)], want2, 3, "twice")


# ---- 3. the translation's seams ---------------------------------------------------------------------
@POISON
def test_translation_seams_under_a_custom_table(poison, monkeypatch):
    """Targets of 0..6 codes and of 3 x 64 + d and 3 x 128 + d codes, d = -1..3, a plant across
    codon 63 | 64 of a forward and of a reverse frame, N inside a codon, under a codon table that
    differs from the standard one in every entry."""
    TD._poison(poison, monkeypatch)
    tab = FR.custom_table()
    q, seqs = TG._cached("dframes-seams", lambda: DF.seam_cases(tab))
    pairs = [(0, k) for k in range(len(seqs))]
    want = TG._cached("dframes-seams-want", lambda: _want([q], seqs, pairs, 3, table=tab))
    std = TG._cached("dframes-seams-std", lambda: _want([q], seqs, pairs, 3))
    assert 2 * sum(a != b for a, b in zip(want, std)) > len(seqs)
    assert {len(t) for t in seqs} >= set(range(7)) | {3 * b + d for b in (64, 128)
                                                       for d in range(-1, 4)}
    bt = TG._cached("dframes-seams-batch", lambda: TG.Batch(seqs))
    with _bank() as bank:
        bank.load_query(q)
        _both_forms(bank, bt, pairs, want, 3, "seams", table=tab)
        _check(_device(bank, bt, pairs, 3, TD._stride(std)), std, pairs, 3, "standard")


# ---- 4. min_score -----------------------------------------------------------------------------------
@POISON
def test_min_score_cuts_the_records(poison, monkeypatch):
    """A min_score between the second and the third record: two records, then empty slots with no
    frame bits; one above the best score: every record is empty."""
    TD._poison(poison, monkeypatch)
    q, seqs, pairs, full = _exon_case(60)
    sc = D.scores(full[0])
    assert sc[1] > sc[2] >= MIN_SCORE
    cut = _want([q], seqs, pairs, ROUNDS, min_score=sc[2] + 1)
    assert cut[0][:2] == full[0][:2] and cut[0][2:] == [D.EMPTY_REC] * 3
    none = _want([q], seqs, pairs, ROUNDS, min_score=sc[0] + 1)
    assert none == [[D.EMPTY_REC] * ROUNDS] * len(pairs)
    bt = TG._cached(("dframes-exons-batch", 60), lambda: TG.Batch(seqs))
    with _bank() as bank:
        bank.load_query(q)
        _both_forms(bank, bt, pairs, cut, ROUNDS, "cut", min_score=sc[2] + 1)
        _both_forms(bank, bt, pairs, none, ROUNDS, "none", min_score=sc[0] + 1, stride=4)


# ---- 5. hit lists and a query set -------------------------------------------------------------------
def _set_case():
    def make():
        q1, t1 = DF.exon_case(60, seed=6)
        q2, t2 = DF.exon_case(300, seed=7)
        rng = np.random.default_rng(557)
        seqs = [t1, t2, DF.tie_case()[1], rng.integers(0, 5, 90).astype(np.uint8), t2[:5],
                np.zeros(0, np.uint8), DF.twice_case()[1], t1[::-1].copy()]
        return [q1, q2], seqs
    return TG._cached("dframes-set", make)


@POISON
@pytest.mark.parametrize("layout", ["list", "top", "best"])
def test_hit_lists_and_a_query_set(layout, poison, monkeypatch):
    """A set of two queries (4 and 8 rows per lane, so 8 for both): a scrambled pair list with one
    pair listed twice and sentinel slots, the nq x k layout of top_hits_device with sentinel tails,
    and the one-entry-per-target layout."""
    TD._poison(poison, monkeypatch)
    qs, seqs = _set_case()
    n, k = len(seqs), 5
    rng = np.random.default_rng([563, len(layout)])
    if layout == "list":
        pairs = [(int(rng.integers(0, 2)), int(rng.integers(0, n))) for _ in range(13)]
        pairs[7] = pairs[3] = (1, 1)
        pairs[5] = (QUERY_NONE, 2)
        pairs[12] = (1, HIT_NONE)
    elif layout == "top":
        pairs = [(i, int(rng.integers(0, n)) if x < (5, 2)[i] else HIT_NONE)
                 for i in range(2) for x in range(k)]
    else:
        pairs = [(QUERY_NONE if t % 5 == 1 else int(rng.integers(0, 2)), t) for t in range(n)]
    ids = np.arange(n, dtype=np.uint64) * 3 + 100
    want = TG._cached(("dframes-set-want", layout), lambda: _want(qs, seqs, pairs, 3))
    assert layout != "list" or (want[7] == want[3] and len(DF.frames(want[3])) >= 2)
    bt = TG._cached("dframes-set-batch", lambda: TG.Batch(seqs))
    with _bank() as bank:
        bank.load_queries(qs)
        _both_forms(bank, bt, pairs, want, 3, layout, layout=layout, k=k, ids=ids)


@POISON
def test_chain_from_the_six_frame_search_on_one_stream(poison, monkeypatch):
    """score_frames_device -> top_hits_device -> align_disjoint_frame_hits_device on one stream
    with no host step: record 0 has the search's score and frame, the records are the model's."""
    TD._poison(poison, monkeypatch)
    torch = TG._torch()
    dev = torch.device("cuda", 0)
    qs, seqs = _set_case()
    n, nq, k, rounds, stride = len(seqs), 2, 3, 3, 64
    bt = TG._cached("dframes-set-batch", lambda: TG.Batch(seqs))
    stream = torch.cuda.Stream()
    with _bank() as bank:
        bank.load_queries(qs)
        d_sc = torch.full((nq * n,), FILL32, dtype=torch.int32, device=dev)
        d_fr = TG._filled(nq * n)
        d_hits = TG._filled(nq * k * 8)
        d_out = TG._filled(nq * k * rounds * REC)
        d_cig = torch.full((nq * k * rounds * stride,), FILL32, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_frames_device(*bt.ptrs(), n, bt.max_len, d_sc.data_ptr(), d_fr.data_ptr(),
                                 stream=h)
        bank.top_hits_device(d_sc.data_ptr(), n, k, d_hits.data_ptr(), nq=nq, stream=h)
        bank.align_disjoint_frame_hits_device(
            *bt.ptrs(), n, bt.max_len, rounds, nq * k, d_out.data_ptr(), min_score=1,
            d_hits=d_hits.data_ptr(), hits_per_query=k, d_cigar=d_cig.data_ptr(),
            cigar_stride=stride, stream=h)
        bank.sync()
        stream.synchronize()
    sc = d_sc.cpu().numpy().reshape(nq, n)
    fr = d_fr.cpu().numpy().reshape(nq, n)
    hits = d_hits.cpu().numpy().view(np.uint64)
    flat = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                             d_cig.cpu().numpy().view(np.uint32))
    got = [flat[x * rounds:(x + 1) * rounds] for x in range(nq * k)]
    pairs = [(x // k, int(hits[x])) for x in range(nq * k)]
    assert all(t < n for _, t in pairs)
    for (i, t), hit in zip(pairs, got):
        assert sc[i, t] > 0 and (hit[0].score, hit[0].frame) == (int(sc[i, t]), int(fr[i, t]))
    _check(got, _want(qs, seqs, pairs, rounds, min_score=1), pairs, rounds, "chain")


# ---- 6. the budget and the CIGAR space --------------------------------------------------------------
def _budget_case():
    def make():
        q = DF.exon_case(60, seed=11)[0]
        rng = np.random.default_rng(569)
        seqs = []
        for s in range(20):
            parts = [rng.integers(0, 4, 6 + s % 4), FR.back_translate(rng, q[:20 + s]),
                     rng.integers(0, 4, 10 + s % 5),
                     SC.revcomp(FR.back_translate(rng, q[25:])), rng.integers(0, 4, 7)]
            seqs.append(np.concatenate(parts).astype(np.uint8))
        pairs = [(0, k) for k in range(len(seqs))]
        return q, seqs, pairs, _want([q], seqs, pairs, 3)
    return TG._cached("dframes-budget", make)


@POISON
def test_budget_chunks_and_cigar_space(poison, monkeypatch):
    """SWBANK_ALIGN_MB = 1: both forms run several chunks with the single-chunk records.  A hit
    whose six stores exceed the budget is refused with the knob named and the outputs keep their
    fill.  A cigar_stride too small for record 0 only: SW_ALIGN_NO_PATH with exact coordinates,
    and every later record is the ample-stride run's."""
    TD._poison(poison, monkeypatch)
    q, seqs, pairs, want = _budget_case()
    bt = TG._cached("dframes-budget-batch", lambda: TG.Batch(seqs))
    K, budget = 4, 1 << 18
    dwords = lambda L: sum(  # noqa: E731
        (FR.frame_len(L, f) + (60 + K - 1) // K - 1) * (K // 4) * 64 if FR.frame_len(L, f) else 0
        for f in range(6))
    with _bank() as bank:
        bank.load_query(q)
        monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
        assert sum(dwords(int(L)) for L in bt.lens) > 2 * budget
        _check(_host(bank, (bt.res, bt.offs, bt.lens), pairs, 3), want, pairs, 3, "host chunks")
        assert int(bank.last_kernel().split("chunks=")[1]) >= 3
        _check(_device(bank, bt, pairs, 3, TD._stride(want)), want, pairs, 3, "device chunks")
        per = budget // (6 * (bt.max_len // 3 + (60 + K - 1) // K - 1) * (K // 4) * 64)
        assert bank.last_kernel() == _name(bank, 3, len(pairs), -(-len(pairs) // per))
        assert per < len(pairs)
        # one hit over the budget
        big = TG.Batch(seqs + [np.zeros(2400, np.uint8)])
        assert dwords(2400) > budget
        torch = TG._torch()
        d_out = TG._filled(REC * 3)
        one = np.array([len(seqs)], np.uint64)
        hits = TG._to_dev(one)
        hrec = np.full(3 * REC, 0x3C, np.uint8)
        for st in (
            S.lib().sw_align_disjoint_frame_hits_device(
                bank._h, *big.ptrs(), None, big.n, big.max_len, None, 3, 1, None, 1,
                hits.data_ptr(), 1, d_out.data_ptr(), None, 0, None),
            S.lib().sw_align_disjoint_frame_hits(
                bank._h, G._p(big.res), big.res.size, G._p(big.offs), G._p(big.lens), None, big.n,
                None, 3, 1, None, 1, G._p(one), 1, G._p(hrec), None, 0, None)):
            assert st == S.ERR_UNSUPPORTED and "SWBANK_ALIGN_MB" in TD._error(bank)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x3C).all() and (hrec == 0x3C).all()
        monkeypatch.delenv("SWBANK_ALIGN_MB")
        # too little CIGAR space for record 0 only
        q2, t2 = DF.indel_case()
        ample = _want([q2], [t2], [(0, 0)], 4)
        assert [len(ops) for _, ops in ample[0]][:3] == [3, 1, 1]
        cut = _want([q2], [t2], [(0, 0)], 4, cap=2)
        r0, a0 = cut[0][0][0], ample[0][0][0]
        assert r0[1] & S.ALIGN_NO_PATH and cut[0][1:] == ample[0][1:]
        assert r0[:1] + r0[2:6] == a0[:1] + a0[2:6] and FR.frame_of(r0[1]) == FR.frame_of(a0[1])
        bank.load_query(q2)
        b2 = TG.Batch([t2])
        _check(_device(bank, b2, [(0, 0)], 4, 2), cut, [(0, 0)], 4, "small stride")
        _both_forms(bank, b2, [(0, 0)], ample, 4, "ample")
        coords = _device(bank, b2, [(0, 0)], 4, 0, cigar=False)
        for a, (rec, _) in zip(coords[0], ample[0]):
            assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == rec[:1] + rec[2:6]
            assert (a.empty or a.flags & ~(S.ALIGN_REVERSE | S.ALIGN_FRAME_MASK) ==
                    S.ALIGN_NO_PATH) and not a.ops
            assert a.frame == FR.frame_of(rec[1]) and (a.n_columns, a.n_identities) == (0, 0)


def test_timing_brackets_and_a_multi_device_bank():
    """Under set_timing the rounds of a chunk are one launch group; a multi-device bank runs the
    call on its root with the same records."""
    qs, seqs = _set_case()
    pairs = [(k % 2, k) for k in range(len(seqs))]
    want = _want(qs, seqs, pairs, 3)
    bt = TG._cached("dframes-set-batch", lambda: TG.Batch(seqs))
    with _bank() as bank:
        bank.load_queries(qs)
        bank.set_timing(True)
        _check(_device(bank, bt, pairs, 3, TD._stride(want)), want, pairs, 3, "timed")
        assert bank.last_kernel() == _name(bank, 3, len(pairs), 1)
        launches, _, ms = bank.timing()
        assert launches == 1 and ms > 0
    with _bank(devices=[0, 0]) as bank:
        bank.load_queries(qs)
        _both_forms(bank, bt, pairs, want, 3, "multi", chunks=None)


# ---- 7. refusals ------------------------------------------------------------------------------------
def test_refusals_in_the_headers_order():
    """Both forms refuse in the header's order and write nothing: the device outputs and the host
    outputs keep their fill, and the bank stays usable."""
    qs, seqs = _set_case()
    bt = TG._cached("dframes-set-batch", lambda: TG.Batch(seqs))
    host = (bt.res, bt.offs, bt.lens)
    n = bt.n
    torch = TG._torch()
    out = torch.full((1 << 13,), FILL32, dtype=torch.int32, device=torch.device("cuda", 0))
    p = out.data_ptr()
    hq = np.zeros(n, np.uint32)
    hrec = np.full(n * 2 * REC, 0x3C, np.uint8)
    hcig = np.full(4096, FILL32, np.uint32)
    bad_tab = FR.standard_table().copy()
    bad_tab[17] = 24
    P = G._p

    def dev(bank, rounds=2, min_score=1, res=None, n_hits=n, hpq=n, hitq=0, stride=64, d_out=p,
            max_len=None, tab=None):
        b = bt.ptrs() if res is None else res
        return S.lib().sw_align_disjoint_frame_hits_device(
            bank._h, b[0] or None, b[1] or None, b[2] or None, None, n,
            bt.max_len if max_len is None else max_len, P(tab) if tab is not None else None,
            rounds, min_score, hitq or None, hpq, None, n_hits, d_out or None, p + 16384, stride,
            None)

    def hst(bank, rounds=2, min_score=1, batch=host, n_hits=n, hpq=0, hitq=hq, tab=None):
        used = np.zeros(1, np.uint64)
        st = S.lib().sw_align_disjoint_frame_hits(
            bank._h, P(batch[0]), batch[0].size, P(batch[1]), P(batch[2]), None, n,
            P(tab) if tab is not None else None, rounds, min_score,
            P(hitq) if hitq is not None else None, hpq, None, n_hits, P(hrec), P(hcig), hcig.size,
            P(used))
        assert st == 0 or ((hrec == 0x3C).all() and (hcig == FILL32).all() and used[0] == 0)
        return st

    def forms(bank, **kw):  # (the device form: hits_per_query = n; the host form: hit_queries)
        return {dev(bank, **kw), hst(bank, **kw)}

    # 1. a DNA bank, with the gap model, nothing loaded and bad arguments behind it
    with S.ScoreBank(gap_model=O.GAP_MERGED) as bank:
        assert forms(bank, rounds=0) == {S.ERR_UNSUPPORTED}
        assert "protein banks only" in TD._error(bank)
    # 2. the gap model
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_MERGED) as bank:
        assert forms(bank, rounds=0) == {S.ERR_UNSUPPORTED}
        assert "Gotoh" in TD._error(bank)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH) as bank:
        assert forms(bank, rounds=0) == {S.ERR_STATE}              # 3. the state
        bank.set_matrix(np.asarray(O.BLOSUM62, np.int8), *PEN)
        assert forms(bank) == {S.ERR_STATE}
        rng = np.random.default_rng(571)                           # 4. the query length
        bank.load_query(rng.integers(0, 20, S.DISJOINT_MAX_QUERY + 1).astype(np.uint8))
        assert forms(bank, rounds=0) == {S.ERR_UNSUPPORTED}
        bank.load_queries(qs)
        for bad in (0, S.DISJOINT_MAX_ROUNDS + 1):                 # 5. rounds, min_score, the table
            assert forms(bank, rounds=bad, n_hits=0, tab=bad_tab) == {S.ERR_ARG}
            assert "rounds" in TD._error(bank)
        for bad in (0, -5):
            assert forms(bank, min_score=bad, n_hits=0) == {S.ERR_ARG}
        assert forms(bank, tab=bad_tab, n_hits=0) == {S.ERR_ARG}
        assert "codon table" in TD._error(bank)
        assert forms(bank, n_hits=0, rounds=S.DISJOINT_MAX_ROUNDS) == {0}   # 8. no hits
        assert dev(bank, res=(0, 0, 0)) == S.ERR_ARG               # 9. NULL buffers
        assert dev(bank, d_out=0) == S.ERR_ARG
        assert S.lib().sw_align_disjoint_frame_hits(
            bank._h, P(host[0]), host[0].size, P(host[1]), P(host[2]), None, n, None, 2, 1, P(hq),
            0, None, n, None, None, 0, None) == S.ERR_ARG
        # 10. the pair list: both hit_queries and hits_per_query, or neither; too many hits
        d_hq = TG._to_dev(hq)
        assert dev(bank, hitq=d_hq.data_ptr(), hpq=n) == S.ERR_ARG
        assert dev(bank, hpq=0) == S.ERR_ARG
        assert hst(bank, hpq=1) == S.ERR_ARG and hst(bank, hitq=None) == S.ERR_ARG
        assert dev(bank, n_hits=n + 1, hpq=n + 1) == S.ERR_ARG     # no hit list: n_hits > n
        assert hst(bank, hitq=np.full(n, 2, np.uint32)) == S.ERR_ARG   # a query >= nq (host)
        bad = bt.res.copy()                                        # the listed targets (host):
        bad[int(bt.offs[2]) + 1] = 5                               # a protein code is no DNA code
        assert hst(bank, batch=(bad, bt.offs, bt.lens)) == S.ERR_ARG
        assert "DNA code" in TD._error(bank)
        # 11. n_hits x rounds x cigar_stride
        assert dev(bank, stride=1 << 29) == S.ERR_ARG
        # 12. a hit over the budget
        assert dev(bank, max_len=1 << 22) == S.ERR_UNSUPPORTED
        assert "SWBANK_ALIGN_MB" in TD._error(bank)
        bank.sync()
        assert (out.cpu().numpy() == FILL32).all()                 # the device outputs keep their fill
        pairs = [(0, k) for k in range(n)]
        _check(_host(bank, host, pairs, 2), _want(qs, seqs, pairs, 2), pairs, 2, "usable")
