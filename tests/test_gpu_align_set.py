"""Alignments against a query set on the GPU (sw_align_set_hits / sw_align_set_hits_device): the
pair lists of tests/set_cases.py against the brute-force coordinates and the reference
traceback, the top-hits layout and the best-query list end to end on one stream, a set of one
against the single-query calls, the direction-store budget, protein, the multi-device bank and
the argument errors.  Every test runs with plain and with poisoned device buffers; the CPU
references are computed once (set_cases) and shared."""
import os

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_cases as AL
import align_check as AC
import matrix_cases as MC
import set_cases as SC

pytestmark = pytest.mark.gpu

REF, ALT = SC.REF, SC.ALT
MODELS = [S.GAP_MERGED, S.GAP_GOTOH]
FILL = 0x3C


@pytest.fixture(params=["plain", "poisoned"], autouse=True)
def buffers(request):
    if request.param == "poisoned":
        request.getfixturevalue("poisoned_buffers")


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


def _dna_bank(model, pen, **kw):
    bank = S.ScoreBank(gap_model=model, **kw)
    bank.set_penalties(*pen)
    return bank


class Batch:
    """A batch on the device."""

    def __init__(self, seqs):
        self.res, self.offs, self.lens = S.pack_targets(seqs)
        self.n = len(seqs)
        self.max_len = max(int(self.lens.max()), 1)
        self.d = [_to_dev(self.res), _to_dev(self.offs), _to_dev(self.lens)]

    def ptrs(self):
        return [t.data_ptr() for t in self.d]


def _device_set(bank, batch, n_hits, stride, hit_queries=None, hits=None, hits_per_query=0,
                max_len=None, n=None, raw=False):
    """sw_align_set_hits_device over 0x3C-filled outputs -> Alignment objects (raw: the record
    bytes and the CIGAR buffer as well)."""
    torch = _torch()
    d_hq = _to_dev(np.asarray(hit_queries, np.uint32)) if hit_queries is not None else None
    d_hits = _to_dev(np.asarray(hits, np.uint64)) if hits is not None else None
    d_out = _filled(n_hits * S.ALIGNMENT_DTYPE.itemsize)
    d_cig = _filled(n_hits * stride * 4)
    torch.cuda.synchronize()
    bank.align_set_hits_device(*batch.ptrs(), batch.n if n is None else n,
                               batch.max_len if max_len is None else max_len, n_hits,
                               d_out.data_ptr(), d_hits=d_hits.data_ptr() if hits is not None else 0,
                               d_hit_queries=d_hq.data_ptr() if hit_queries is not None else 0,
                               hits_per_query=hits_per_query,
                               d_cigar=d_cig.data_ptr() if stride else 0, cigar_stride=stride)
    bank.sync()
    rec = d_out.cpu().numpy()[:n_hits * S.ALIGNMENT_DTYPE.itemsize].view(S.ALIGNMENT_DTYPE)
    cig = d_cig.cpu().numpy().view(np.uint32)
    if stride:
        assert [int(r["cigar_offset"]) for r in rec] == [h * stride for h in range(n_hits)]
    alns = S.alignments_from(rec, cig)
    return (alns, rec.tobytes(), cig.tobytes()) if raw else alns


def _stride(case):
    return 2 * max(len(s) for s in case.seqs) + 1


# ---- 1. set boundaries ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pen", [REF, ALT])
def test_set_boundaries(pen, model, monkeypatch):
    case = SC.set_case()
    sub = O.dna_matrix(pen[0], pen[1])
    refs = SC.pair_refs(case, sub, pen[2], pen[3], model, "set")
    assert sum(1 for (b, _) in refs if b[0] > 0) >= 60
    assert refs[-2][0] != refs[-1][0]  # one target, two queries of one length: two records
    res, offs, lens = S.pack_targets(case.seqs)
    with _dna_bank(model, pen) as bank:
        bank.load_queries(case.queries)
        host = bank.align_set_hits(res, offs, lens, hits=case.hits, hit_queries=case.hit_queries)
        assert bank.last_kernel() == \
            f"align-set i32 nq={len(case.queries)} hits={len(case)} chunks=1"
        SC.check_records(case, host, refs)
        # the device call with scratch rows for 64 waves only: hits 0 (513 rows) and 64 (1 row)
        # go through one wave
        monkeypatch.setenv("SWBANK_EDGE_MB", "1")
        assert AL.i32_waves(len(case), 1024, 1 << 20) == SC.WAVES_SHARED < len(case)
        batch = Batch(case.seqs)
        dev = _device_set(bank, batch, len(case), _stride(case), hit_queries=case.hit_queries,
                          hits=case.hits, max_len=1024)
        SC.check_records(case, dev, refs)
        assert dev == host


# ---- 2. the top-hits layout, end to end ----------------------------------------------------------
def _golden_set():
    def make():
        recs = O.read_fasta(O.golden_fasta("data500.fa"))
        q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
        names = [n for n, _ in recs]
        seqs = [O.encode_dna(s) for _, s in recs]
        rng = np.random.default_rng(12)
        queries = [q, q[20:90].copy(), rng.integers(0, 4, 130).astype(np.uint8)]
        ores, ooffs, olens = O.pack_residues(seqs)
        oracle = np.stack([O.score_batch(x, ores, ooffs, olens, O.dna_matrix(), -12, -4,
                                         O.GAP_MERGED) for x in queries]).astype(np.int32)
        return names, seqs, queries, oracle
    return SC._cached("golden-set", make)


def test_top_hits_layout_chain():
    torch = _torch()
    names, seqs, queries, oracle = _golden_set()
    n, nq, k = len(seqs), 3, 40
    # the largest of the rows' 40th scores: that row is full, a row whose 40th score is lower
    # ends in sentinels
    kth = [int(np.sort(row)[::-1][k - 1]) for row in oracle]
    min_score = max(kth)
    counts = [min(k, int((row >= min_score).sum())) for row in oracle]
    assert max(counts) == k and min(counts) < k and counts[0] >= 2, counts
    batch = Batch(seqs)
    stride = 2 * batch.max_len + 1
    dev = torch.device("cuda", 0)
    d_scores = torch.full((nq * n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_hits, d_out = _filled(nq * k * 8), _filled(nq * k * S.ALIGNMENT_DTYPE.itemsize)
    d_cig = _filled(nq * k * stride * 4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _dna_bank(S.GAP_MERGED, REF) as bank:
        bank.load_queries(queries)
        h = st.cuda_stream
        bank.score_batch_device(*batch.ptrs(), n, batch.max_len, d_scores.data_ptr(), stream=h)
        bank.top_hits_device(d_scores.data_ptr(), n, k, d_hits.data_ptr(), nq=nq,
                             min_score=min_score, stream=h)
        bank.align_set_hits_device(*batch.ptrs(), n, batch.max_len, nq * k, d_out.data_ptr(),
                                   d_hits=d_hits.data_ptr(), hits_per_query=k,
                                   d_cigar=d_cig.data_ptr(), cigar_stride=stride, stream=h)
        assert bank.last_kernel().startswith(f"align-set i32 nq=3 hits={nq * k} chunks=")
        bank.sync()
        st.synchronize()
    assert np.array_equal(d_scores.cpu().numpy().reshape(nq, n), oracle)
    hits = d_hits.cpu().numpy().view(np.uint64).reshape(nq, k)
    alns = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                             d_cig.cpu().numpy().view(np.uint32))
    rows = [ln.rstrip("\n").split("\t")
            for ln in open(os.path.join(O.GOLDEN, "alignments500.tsv"))][1:]
    assert [r[0] for r in rows] == ["db211", "db428"]
    for r in rows:  # row 0 is query100: the ssearch36 report, where the hit ranks
        at = [j for j in range(counts[0]) if names[int(hits[0, j])] == r[0]]
        assert len(at) == 1, r[0]
        a = alns[at[0]]
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns,
                a.n_identities) == tuple(int(x) for x in r[1:8])
        assert a.cigar == r[8] and a.flags == 0
    sub = O.dna_matrix()
    for i in range(nq):
        for j in range(k):
            a = alns[i * k + j]
            if j < counts[i]:
                t = int(hits[i, j])
                assert a.index == t and a.id == t
                AC.check_alignment(O, queries[i], seqs[t], sub, -12, -4, S.GAP_MERGED, a)
            else:
                assert hits[i, j] == SC.HIT_NONE and SC.sentinel_ok(a), (i, j, a)


# ---- 3. a set of one ------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_set_of_one(model):
    torch = _torch()
    q, seqs, hits = AL.boundary_case(300, 88)
    res, offs, lens = S.pack_targets(seqs)
    nh = len(hits)
    stride = 2 * max(len(s) for s in seqs) + 1
    batch = Batch(seqs)
    with _dna_bank(model, ALT) as bank:
        bank.load_query(q)
        d_hits = _to_dev(np.asarray(hits, np.uint64))
        d_out = _filled(nh * S.ALIGNMENT_DTYPE.itemsize)
        d_cig = _filled(nh * stride * 4)
        torch.cuda.synchronize()
        bank.align_hits_device(*batch.ptrs(), batch.n, batch.max_len, d_hits.data_ptr(), nh,
                               d_out.data_ptr(), d_cig.data_ptr(), stride)
        bank.sync()
        want = (d_out.cpu().numpy().tobytes(), d_cig.cpu().numpy().tobytes())
        assert any(len(a.ops) > 1 for a in S.alignments_from(
            d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE), d_cig.cpu().numpy().view(np.uint32)))
        for kw in (dict(hit_queries=np.zeros(nh, np.uint32)), dict(hits_per_query=nh),
                   dict(hits_per_query=nh + 5)):
            _, rec, cig = _device_set(bank, batch, nh, stride, hits=hits, raw=True, **kw)
            assert (rec, cig) == want, kw
        host = bank.align_hits(res, offs, lens, hits)
        assert bank.align_set_hits(res, offs, lens, hits=hits,
                                   hit_queries=np.zeros(nh, np.uint32)) == host
        assert bank.align_set_hits(res, offs, lens, hits=hits, hits_per_query=nh) == host
        assert bank.last_kernel().startswith(f"align-set i32 nq=1 hits={nh} chunks=")


# ---- 4. the direction-store budget ---------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_budget(model, monkeypatch):
    case30 = SC.set_case().head(30)
    sub = O.dna_matrix()
    refs30 = SC.pair_refs(SC.set_case(), sub, -12, -4, model, "set")[:30]
    monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
    with _dna_bank(model, REF) as bank:
        # slots of 513 rows x 200 columns: 3 strips x 263 steps x 256 B, 5 to the MiB
        bank.load_queries(case30.queries)
        batch = Batch(case30.seqs)
        assert batch.max_len == 200 and (1 << 20) // (3 * 263 * 256) == 5
        dev = _device_set(bank, batch, 30, _stride(case30), hit_queries=case30.hit_queries,
                          hits=case30.hits)
        assert bank.last_kernel() == f"align-set i32 nq={len(case30.queries)} hits=30 chunks=6"
        SC.check_records(case30, dev, refs30)
        # a 4,100-row query joins the set: 17 strips x 263 steps x 256 B > 1 MiB per slot
        case = SC.long_case()
        refs = SC.pair_refs(case, sub, -12, -4, model, "long")
        assert (17 * 263 * 256) > (1 << 20) and len(case.queries[-1]) == SC.LONG_QUERY
        bank.load_queries(case.queries)
        res, offs, lens = S.pack_targets(case.seqs)
        host = bank.align_set_hits(res, offs, lens, hits=case.hits, hit_queries=case.hit_queries)
        big = [h for h, (b, _) in enumerate(refs)
               if b[0] > 0 and 256 * ((b[2] - b[1]) // 256 + 1) * (b[4] - b[3] + 64) > (1 << 20)]
        assert big == [len(case) - 1]  # the planted window, and only it
        SC.check_records(case, host, refs, no_path=big)
        assert sum(1 for a in host if a.flags == 0) >= 25
        # the device call's slots are sized for the longest query: no hit gets a path
        short = SC.SetCase(case.queries, case.seqs[:24], case.hit_queries[:31], case.hits[:31])
        assert all(int(t) < 24 for t in short.hits) and SC.LONG_QUERY in \
            [len(case.queries[int(q)]) for q in short.hit_queries]
        dev = _device_set(bank, Batch(short.seqs), 31, _stride(short),
                          hit_queries=short.hit_queries, hits=short.hits)
        assert bank.last_kernel() == f"align-set i32 nq={len(case.queries)} hits=31 chunks=0"
        SC.check_records(short, dev, refs[:31], want_path=False)


# ---- 5. protein ----------------------------------------------------------------------------------
def test_protein_set():
    case = SC.protein_set_case()
    refs = SC.pair_refs(case, O.BLOSUM62, -11, -1, S.GAP_GOTOH, "protein")
    assert sum(1 for (b, _) in refs if b[0] > 0) >= 18
    res, offs, lens = S.pack_targets(case.seqs)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=S.GAP_GOTOH) as bank:
        bank.set_matrix(O.BLOSUM62, -11, -1)
        bank.load_queries(case.queries)
        host = bank.align_set_hits(res, offs, lens, hits=case.hits, hit_queries=case.hit_queries)
        SC.check_records(case, host, refs)
        dev = _device_set(bank, Batch(case.seqs), len(case), _stride(case),
                          hit_queries=case.hit_queries, hits=case.hits)
        SC.check_records(case, dev, refs)
        for a, qi, t in zip(dev, case.hit_queries, case.hits):
            AC.check_alignment(O, case.queries[int(qi)], case.seqs[int(t)], O.BLOSUM62, -11, -1,
                               S.GAP_GOTOH, a)


# ---- 5b. asymmetric matrices ---------------------------------------------------------------------
@pytest.mark.parametrize("name,model", MC.PARAMS)
def test_asymmetric_matrix_set(name, model):
    """The matrix family of tests/matrix_cases.py against a set of three queries (700 rows, its
    rows 100-400, a 40-row piece) that interleave in the hit list, sentinel slots among them:
    the host and the device form agree, and every record is the brute-force record and the
    reference path of its (query, target), op for op.  The SET kernels build their profiles
    per query: one built from the transposed matrix would change most of these scores."""
    P = MC.matrix_param(name, model)
    g = MC.matrix_family(P)
    queries, hq, hv = MC.set_form(g)
    case = SC.SetCase(queries, g.seqs, hq, hv, alpha=P.sub.shape[0])
    refs = SC.pair_refs(case, P.sub, P.go, P.ge, model, f"matrix-{name}")
    assert [h for h, r in enumerate(refs) if r is None] == sorted(MC.SET_NONE)
    assert all(sum(1 for h, r in enumerate(refs) if r and hq[h] == i and r[0][0] > 0) >= 20
               for i in range(3))
    res, offs, lens = S.pack_targets(case.seqs)
    protein = P.sub.shape[0] > 5
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN if protein else S.ALPHABET_DNA,
                     gap_model=model) as bank:
        bank.set_matrix(P.sub, P.go, P.ge)
        bank.load_queries(queries)
        host = bank.align_set_hits(res, offs, lens, hits=hv, hit_queries=hq)
        assert bank.last_kernel() == f"align-set i32 nq=3 hits={len(case)} chunks=1"
        dev = _device_set(bank, Batch(case.seqs), len(case), _stride(case), hit_queries=hq,
                          hits=hv)
    assert dev == host
    seen = set()
    for h, (a, ref) in enumerate(zip(dev, refs)):
        if ref is None:
            assert SC.sentinel_ok(a), (h, a)
            continue
        (s, qs, qe, ts, te), path = ref
        qi, t = int(hq[h]), int(hv[h])
        assert a.index == t and a.id == t
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == (s, qs, qe, ts, te), (h, a)
        if s == 0:
            assert a.flags == SC.ALIGN_EMPTY and not a.ops, (h, a)
        else:
            assert a.flags == 0 and tuple(a.ops) == tuple(path.ops), (h, a.cigar, path)
            assert (a.n_columns, a.n_identities) == (path.n_columns, path.n_identities), (h, a)
        if (qi, t) not in seen:
            AC.check_alignment(O, queries[qi], case.seqs[t], P.sub, P.go, P.ge, model, a)
            seen.add((qi, t))


# ---- 6. read mapping in small ----------------------------------------------------------------------
def test_read_mapping_chain():
    torch = _torch()
    refs, reads, oracle, min_score = SC.readmap_case()
    nq, n = oracle.shape
    want_q, want_s = SC.ref_best(oracle, min_score)
    batch = Batch(reads)
    stride = 2 * batch.max_len + 1
    dev = torch.device("cuda", 0)
    d_scores = torch.full((nq * n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_bq, d_bs = _filled(n * 4), _filled(n * 4)
    d_out, d_cig = _filled(n * S.ALIGNMENT_DTYPE.itemsize), _filled(n * stride * 4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _dna_bank(S.GAP_MERGED, REF) as bank:
        bank.load_queries(refs)
        h = st.cuda_stream
        bank.score_batch_device(*batch.ptrs(), n, batch.max_len, d_scores.data_ptr(), stream=h)
        bank.best_queries_device(d_scores.data_ptr(), n, nq, d_bq.data_ptr(), d_bs.data_ptr(),
                                 min_score=min_score, stream=h)
        assert bank.last_kernel() == f"best-query nq={nq} n={n}"
        bank.align_set_hits_device(*batch.ptrs(), n, batch.max_len, n, d_out.data_ptr(),
                                   d_hit_queries=d_bq.data_ptr(), d_cigar=d_cig.data_ptr(),
                                   cigar_stride=stride, stream=h)
        bank.sync()
        st.synchronize()
    assert np.array_equal(d_scores.cpu().numpy().reshape(nq, n), oracle)
    assert np.array_equal(d_bq.cpu().numpy().view(np.uint32), want_q)
    assert np.array_equal(d_bs.cpu().numpy().view(np.int32), want_s)
    alns = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                             d_cig.cpu().numpy().view(np.uint32))
    sub = O.dna_matrix()
    mapped = 0
    for k, a in enumerate(alns):
        if want_q[k] == SC.QUERY_NONE:
            assert SC.sentinel_ok(a), (k, a)
        else:
            mapped += 1
            assert a.index == k and a.score == int(want_s[k])
            AC.check_alignment(O, refs[int(want_q[k])], reads[k], sub, -12, -4, S.GAP_MERGED, a)
    assert mapped >= 32 and len(alns) - mapped >= 32


# ---- 7. a multi-device bank runs it on its root ------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_multi_device_bank(model):
    case = SC.set_case()
    refs = SC.pair_refs(case, O.dna_matrix(), -12, -4, model, "set")
    res, offs, lens = S.pack_targets(case.seqs)
    got = []
    for kw in ({}, {"devices": [0, 0]}):
        with _dna_bank(model, REF, **kw) as bank:
            bank.load_queries(case.queries)
            got.append(bank.align_set_hits(res, offs, lens, hits=case.hits,
                                           hit_queries=case.hit_queries))
            got.append(_device_set(bank, Batch(case.seqs), len(case), _stride(case),
                                   hit_queries=case.hit_queries, hits=case.hits))
            assert bank.last_kernel() == \
                f"align-set i32 nq={len(case.queries)} hits={len(case)} chunks=1"
    SC.check_records(case, got[0], refs)
    for other in got[1:]:
        assert other == got[0]


# ---- 8. errors ---------------------------------------------------------------------------------------
def test_errors():
    enc = O.encode_dna
    seqs = [enc("ACGTACGT"), enc("TTTT")]
    res, offs, lens = S.pack_targets(seqs)
    batch = Batch(seqs)
    d_out = _filled(8 * S.ALIGNMENT_DTYPE.itemsize)
    d_hits = _to_dev(np.zeros(8, np.uint64))
    d_hq = _to_dev(np.zeros(8, np.uint32))

    def host(bank, **kw):
        return bank.align_set_hits(res, offs, lens, **kw)

    def device(bank, n_hits, **kw):
        bank.align_set_hits_device(*batch.ptrs(), 2, batch.max_len, n_hits, d_out.data_ptr(), **kw)

    def refused(status, call):
        with pytest.raises(S.SwbankError) as e:
            call()
        assert e.value.status == status

    with _dna_bank(S.GAP_MERGED, REF) as bank:
        refused(S.ERR_STATE, lambda: host(bank, hits=[0], hit_queries=[0]))  # no query yet
        refused(S.ERR_STATE, lambda: device(bank, 1, d_hits=d_hits.data_ptr(), hits_per_query=1))
        bank.load_queries([enc("ACGT"), enc("GGGTTT")])
        # both or neither of hit_queries / hits_per_query
        refused(S.ERR_ARG, lambda: host(bank, hits=[0], hit_queries=[0], hits_per_query=1))
        refused(S.ERR_ARG, lambda: host(bank, hits=[0]))
        refused(S.ERR_ARG, lambda: device(bank, 1, d_hits=d_hits.data_ptr(),
                                          d_hit_queries=d_hq.data_ptr(), hits_per_query=1))
        refused(S.ERR_ARG, lambda: device(bank, 1, d_hits=d_hits.data_ptr()))
        # n_hits > nq x hits_per_query
        refused(S.ERR_ARG, lambda: host(bank, hits=[0, 1, 0, 1, 0], hits_per_query=2))
        refused(S.ERR_ARG, lambda: device(bank, 5, d_hits=d_hits.data_ptr(), hits_per_query=2))
        assert len(host(bank, hits=[0, 1, 0, 1], hits_per_query=2)) == 4
        # no hit list: n_hits <= n
        refused(S.ERR_ARG, lambda: host(bank, hit_queries=[0, 1, 0], n_hits=3))
        refused(S.ERR_ARG, lambda: device(bank, 3, d_hit_queries=d_hq.data_ptr()))
        assert len(host(bank, hit_queries=[0, 1])) == 2
        # the host call's lists: a query == nq, a target == n
        refused(S.ERR_ARG, lambda: host(bank, hits=[0], hit_queries=[2]))
        refused(S.ERR_ARG, lambda: host(bank, hits=[2], hit_queries=[0]))
        # no hits: fine
        assert host(bank, hits=[], hit_queries=[]) == []
        device(bank, 0, d_hits=d_hits.data_ptr(), hits_per_query=1)
        # the sentinels, on the host
        alns = host(bank, hits=[0, S.HIT_NONE, 1], hit_queries=[0, 1, S.QUERY_NONE])
        assert alns[0].cigar == "4M" and alns[0].index == 0
        assert SC.sentinel_ok(alns[1]) and SC.sentinel_ok(alns[2])
        # with a set loaded the single-query calls still refuse
        refused(S.ERR_STATE, lambda: bank.align_hits(res, offs, lens, [0]))
        refused(S.ERR_STATE, lambda: bank.align_hits_device(
            *batch.ptrs(), 2, batch.max_len, d_hits.data_ptr(), 1, d_out.data_ptr()))
        bank.sync()
    with S.ScoreBank() as bank:  # merged gaps with max(s) > open + extend: documented refusal
        bank.set_penalties(5, -4, -2, -1)
        bank.load_queries([enc("ACGT"), enc("GGGTTT")])
        refused(S.ERR_UNSUPPORTED, lambda: host(bank, hits=[0], hit_queries=[0]))
        refused(S.ERR_UNSUPPORTED,
                lambda: device(bank, 1, d_hits=d_hits.data_ptr(), hits_per_query=1))
    assert S.QUERY_NONE == int(SC.QUERY_NONE) and S.ALIGN_NO_HIT == SC.ALIGN_NO_HIT == 4
