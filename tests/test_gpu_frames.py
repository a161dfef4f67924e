"""The translated search on the GPU (include/swbank.h "translated search"): the six-frame
translation of a batch byte for byte against the model of tests/frame_cases.py, the frame-merged
scores against the oracle on the model's translations, the frame-aware alignments against what
align_set_hits returns for a batch holding the translation, the chain score_frames -> top_hits ->
align_frame_hits on one stream, and the refusals.  Every test runs with plain and with poisoned
device buffers; the CPU references are computed once per process and shared."""
import ctypes
import dataclasses

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_check as AC
import frame_cases as F
import matrix_cases as MC
import seam_cases as SEAMS

pytestmark = pytest.mark.gpu

FILL = 0x3C
MODELS = [O.GAP_MERGED, O.GAP_GOTOH]
TR_LENS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 62, 63, 64, 65, 66, 191, 192, 193, 194, 195, 1021]


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


class Batch:
    """A packed DNA batch on the device (16 zero bytes behind the last target)."""

    def __init__(self, seqs):
        self.seqs = [np.asarray(s, np.uint8) for s in seqs]
        res, self.offs, self.lens = S.pack_targets(self.seqs)
        self.res = np.concatenate([res, np.zeros(16, np.uint8)])
        self.n = len(self.seqs)
        self.max_len = int(self.lens.max())
        self.min_len = int(self.lens.min())
        self.d_res, self.d_offs, self.d_lens = _to_dev(self.res), _to_dev(self.offs), _to_dev(self.lens)

    def ptrs(self):
        return self.d_res.data_ptr(), self.d_offs.data_ptr(), self.d_lens.data_ptr()


def _bank(model=O.GAP_GOTOH, **kw):
    bank = S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=model, **kw)
    bank.set_matrix(O.BLOSUM62, *F.PEN)
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


# ---- 1. the translation ---------------------------------------------------------------------------
def _gapped_batch(n, pool):
    """n targets whose lengths walk through the pool, at odd byte offsets with 1-3 guard bytes
    between them, N codes included: (residues, offsets, lengths)."""
    rng = np.random.default_rng([n, len(pool)])
    lens = np.array([pool[(5 * k + 3) % len(pool)] for k in range(n)], np.uint32)
    offs = np.zeros(n, np.int64)
    pos = 0
    for k in range(n):
        pos += int(rng.integers(1, 4))
        pos += (pos + 1) % 2  # every start is odd
        offs[k] = pos
        pos += int(lens[k])
    res = rng.integers(0, 5, pos + 5).astype(np.uint8)
    assert (offs % 2 == 1).all() and (res == 4).any()
    return res, offs.astype(np.uint64), lens


@pytest.mark.parametrize("table", ["standard", "custom"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_translation_matches_the_model_byte_for_byte(n, table):
    torch = _torch()
    tab = F.custom_table() if table == "custom" else None
    pool = TR_LENS[16:] + TR_LENS[:16] if n == 1 else TR_LENS  # (n = 1: one 195-code target)
    res, offs, lens = _gapped_batch(n, pool)
    if n >= 63:
        assert set(TR_LENS) <= set(lens.tolist())
    max_len = int(lens.max())
    stride = max(max_len // 3, 1) + (n % 2) * 3  # the least stride, and an odd one past it
    want = np.full(6 * n * stride, FILL, np.uint8)
    want_offs, want_lens = np.zeros(6 * n, np.uint64), np.zeros(6 * n, np.uint32)
    for f in range(6):
        for k in range(n):
            slot = f * n + k
            tr = F.translate(res[int(offs[k]):int(offs[k]) + int(lens[k])], f, tab)
            want[slot * stride:slot * stride + len(tr)] = tr
            want_offs[slot], want_lens[slot] = slot * stride, len(tr)
    d_res, d_offs, d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)
    d_out, d_oo, d_ol = _filled(len(want)), _filled(6 * n * 8), _filled(6 * n * 4)
    torch.cuda.synchronize()
    base = _live()
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN) as bank:  # no query: the call needs none
        bank.translate_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n,
                                    max_len, d_out.data_ptr(), stride, d_oo.data_ptr(),
                                    d_ol.data_ptr(), codon_table=tab)
        assert bank.last_kernel() == f"translate n={n}"
        bank.sync()
    assert _live() == base
    got = d_out.cpu().numpy()
    bad = np.nonzero(got != want)[0]  # (the bytes past every translated length keep the fill)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(d_oo.cpu().numpy().view(np.uint64), want_offs)
    assert np.array_equal(d_ol.cpu().numpy().view(np.uint32), want_lens)
    assert np.array_equal(d_res.cpu().numpy(), res)  # the input is left alone


def test_translation_one_long_target_among_short_ones():
    """The kernel has one path for every length, its 64-codon steps dealt over at most 64 waves
    per 64 targets: a 70,000-code target (365 steps, so every wave takes several) in a wave with
    short and empty ones."""
    torch = _torch()
    res, offs, lens = _gapped_batch(67, [5, 70000, 300, 0] + [33] * 17)
    n, max_len = len(lens), int(lens.max())
    assert max_len == 70000 and (lens == 0).any()
    stride = max_len // 3
    want = np.full(6 * n * stride, FILL, np.uint8)
    want_lens = np.zeros(6 * n, np.uint32)
    for f in range(6):
        for k in range(n):
            tr = F.translate(res[int(offs[k]):int(offs[k]) + int(lens[k])], f)
            want[(f * n + k) * stride:(f * n + k) * stride + len(tr)] = tr
            want_lens[f * n + k] = len(tr)
    d_res, d_offs, d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)
    d_out, d_oo, d_ol = _filled(len(want)), _filled(6 * n * 8), _filled(6 * n * 4)
    torch.cuda.synchronize()
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN) as bank:
        bank.translate_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n,
                                    max_len, d_out.data_ptr(), stride, d_oo.data_ptr(),
                                    d_ol.data_ptr())
        bank.sync()
    assert np.array_equal(d_out.cpu().numpy(), want)
    assert np.array_equal(d_ol.cpu().numpy().view(np.uint32), want_lens)


def test_translated_library_scores_as_a_protein_batch():
    """A library translated once is an ordinary protein batch: score_batch_device over the 6 n
    translations gives the per-frame oracle scores."""
    torch = _torch()
    qs, seqs, _ = _case()[:3]
    per = _case()[3][O.GAP_GOTOH][2]
    bt = Batch(seqs)
    stride = (bt.max_len // 3 + 15) // 16 * 16 + 16
    d_out = torch.zeros(6 * bt.n * stride + 64, dtype=torch.uint8, device=torch.device("cuda", 0))
    d_oo, d_ol = _filled(6 * bt.n * 8), _filled(6 * bt.n * 4)
    d_sc = torch.full((6 * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    with _bank() as bank:
        bank.load_query(qs[0])
        bank.translate_batch_device(*bt.ptrs(), bt.n, bt.max_len, d_out.data_ptr(), stride,
                                    d_oo.data_ptr(), d_ol.data_ptr())
        bank.score_batch_device(d_out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), 6 * bt.n,
                                bt.max_len // 3, d_sc.data_ptr())
        bank.sync()
    assert np.array_equal(d_sc.cpu().numpy().reshape(6, bt.n), per[0])


# ---- 2. scores and frames ---------------------------------------------------------------------------
def _case():
    """The search case of tests/frame_cases.py with the oracle's numbers for both gap models."""
    def make():
        qs, seqs, planted = F.search_case()
        return qs, seqs, planted, {m: F.want_frames(qs, seqs, m) for m in MODELS}
    return _cached("frames-search", make)


def _slices(n, nq, max_len, mb=1):
    """The slices of a call under SWBANK_FRAME_MB=mb: per target six translations at a stride of
    max_len / 3 rounded up to 16, plus 16, six offsets and lengths and 6 nq scores."""
    per = 6 * ((max_len // 3 + 15) // 16 * 16 + 16 + 8 + 4 + 4 * nq)
    span = min(n, max(1, (mb << 20) // per))
    return -(-n // span)


def _score_device(bank, bt, nq, frames=True, table=None, stream=0):
    torch = _torch()
    dev = torch.device("cuda", 0)
    d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_fr = _filled(nq * bt.n)
    torch.cuda.synchronize()
    bank.score_frames_device(*bt.ptrs(), bt.n, bt.max_len, d_sc.data_ptr(),
                             d_frames=d_fr.data_ptr() if frames else 0, min_len=bt.min_len,
                             codon_table=table, stream=stream)
    name = bank.last_kernel()
    bank.sync()
    return (d_sc.cpu().numpy().reshape(nq, bt.n), d_fr.cpu().numpy().reshape(nq, bt.n), name)


@pytest.mark.parametrize("model", MODELS)
def test_scores_and_frames_match_the_oracle(model):
    """Queries of 17 and 130 aa alone and a set of three over 200 targets of 0..400 nt with the
    planted hits among them: exactly the oracle's scores and frames; d_frames NULL; the host form."""
    qs, seqs, planted, want = _case()
    wsc, wfr, _ = want[model]
    assert {len(q) for q in qs[:2]} == {17, 130}
    bt = Batch(seqs)
    base = _live()
    with _bank(model) as bank:
        for i in (0, 1):
            bank.load_query(qs[i])
            got, gfr, name = _score_device(bank, bt, 1)
            assert name == f"frames nq=1 n={bt.n} slices=1"
            assert np.array_equal(got[0], wsc[i]) and np.array_equal(gfr[0], wfr[i])
            got2, gfr2, _ = _score_device(bank, bt, 1, frames=False)  # d_frames NULL
            assert np.array_equal(got2, got) and (gfr2 == FILL).all()
            sc, fr = bank.score_frames(bt.res, bt.offs, bt.lens)
            assert np.array_equal(sc, wsc[i]) and np.array_equal(fr, wfr[i])
        bank.load_queries(qs)
        got, gfr, name = _score_device(bank, bt, 3)
        assert name == f"frames nq=3 n={bt.n} slices=1"
        assert np.array_equal(got, wsc) and np.array_equal(gfr, wfr)
        sc, fr = bank.score_frames(bt.res, bt.offs, bt.lens)
        assert np.array_equal(sc, wsc) and np.array_equal(fr, wfr)
        with pytest.raises(S.SwbankError) as ei:  # no best hit is tracked
            bank.best()
        assert ei.value.status == S.ERR_STATE
    assert _live() == base  # the new scratch frees itself with the bank
    for k, (i, f) in planted.items():
        assert (int(got[i][k]), int(gfr[i][k])) == (F.self_score(qs[i]), f)


def test_custom_table_scores():
    qs, seqs, _, _ = _case()
    tab = F.custom_table()
    wsc, wfr, _ = _cached("frames-custom", lambda: F.want_frames(qs[:1], seqs[:64], table=tab))
    bt = Batch(seqs[:64])
    with _bank() as bank:
        bank.load_query(qs[0])
        got, gfr, _ = _score_device(bank, bt, 1, table=tab)
        assert np.array_equal(got, wsc) and np.array_equal(gfr, wfr)
        sc, fr = bank.score_frames(bt.res, bt.offs, bt.lens, codon_table=tab)
        assert np.array_equal(sc, wsc[0]) and np.array_equal(fr, wfr[0])


@pytest.mark.parametrize("nq", [1, 3])
def test_slices_cannot_change_a_result(nq, monkeypatch):
    """SWBANK_FRAME_MB=1 on 2200 targets: at least three slices, the unsliced numbers bit for bit."""
    qs, seqs, _, want = _case()
    wsc, wfr, _ = want[O.GAP_GOTOH]
    reps = 11
    bt = Batch(seqs * reps)
    with _bank() as bank:
        if nq == 1:
            bank.load_query(qs[1])
        else:
            bank.load_queries(qs)
        got, gfr, name = _score_device(bank, bt, nq)
        assert name == f"frames nq={nq} n={bt.n} slices=1"
        rows = slice(1, 2) if nq == 1 else slice(0, 3)
        assert np.array_equal(got, np.tile(wsc[rows], reps))
        assert np.array_equal(gfr, np.tile(wfr[rows], reps))
        monkeypatch.setenv("SWBANK_FRAME_MB", "1")
        s = _slices(bt.n, nq, bt.max_len)
        assert s >= 3
        got2, gfr2, name = _score_device(bank, bt, nq)
        assert name == f"frames nq={nq} n={bt.n} slices={s}"
        assert np.array_equal(got2, got) and np.array_equal(gfr2, gfr)
        sc, fr = bank.score_frames(bt.res, bt.offs, bt.lens)
        assert np.array_equal(sc.reshape(nq, -1), got) and np.array_equal(fr.reshape(nq, -1), gfr)


@pytest.mark.parametrize("shape", ["equal", "one", "empty"])
def test_small_and_uniform_batches(shape):
    rng = np.random.default_rng(83)
    q = rng.integers(0, 20, 40).astype(np.uint8)
    if shape == "equal":  # min_len == max_len
        seqs = [F.plant(rng, q, 150, k % 3, k % 2 == 1)[0] if k % 4 == 0 else
                rng.integers(0, 4, 150).astype(np.uint8) for k in range(70)]
    elif shape == "one":
        seqs = [F.plant(rng, q, 131, 2, True)[0]]
    else:
        seqs = [np.zeros(0, np.uint8)] * 5
    wsc, wfr, _ = F.want_frames([q], seqs)
    bt = Batch(seqs)
    assert shape != "equal" or bt.min_len == bt.max_len == 150
    with _bank() as bank:
        bank.load_query(q)
        got, gfr, name = _score_device(bank, bt, 1)
        assert name == f"frames nq=1 n={bt.n} slices=1"
        assert np.array_equal(got, wsc) and np.array_equal(gfr, wfr)
        sc, fr = bank.score_frames(bt.res, bt.offs, bt.lens)
        assert np.array_equal(sc, wsc[0]) and np.array_equal(fr, wfr[0])
    if shape == "one":
        assert (int(got[0][0]), int(gfr[0][0])) == (F.self_score(q), 5)
    if shape == "empty":
        assert not got.any() and not gfr.any()


def test_timing_brackets_translation_and_merge():
    qs, seqs, _, _ = _case()
    bt = Batch(seqs)
    with _bank() as bank:
        bank.load_query(qs[1])
        _score_device(bank, bt, 1)
        bank.set_timing(True)
        _score_device(bank, bt, 1)
        launches, _, ms = bank.timing()
    assert launches >= 3 and ms > 0  # the translation, the scoring pass, the merge


# ---- 3. alignments ----------------------------------------------------------------------------------
def _device_align(bank, bt, frames, hits, stride, hit_queries=None, hits_per_query=0, ids=None,
                  stream=0, table=None):
    """sw_align_frame_hits_device on torch buffers -> Alignment objects."""
    torch = _torch()
    n_hits = len(hits) if hits is not None else len(hit_queries)
    d_hits = _to_dev(np.asarray(hits, np.uint64)) if hits is not None else None
    d_hq = _to_dev(np.asarray(hit_queries, np.uint32)) if hit_queries is not None else None
    d_fr = _to_dev(np.asarray(frames, np.uint8).reshape(-1))
    d_ids = _to_dev(np.asarray(ids, np.uint64)) if ids is not None else None
    d_out = _filled(n_hits * S.ALIGNMENT_DTYPE.itemsize)
    d_cig = torch.full((max(1, n_hits * stride),), 0x3C3C3C3C, dtype=torch.int32,
                       device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    bank.align_frame_hits_device(
        *bt.ptrs(), bt.n, bt.max_len, n_hits, d_out.data_ptr(), d_fr.data_ptr(),
        d_hits=d_hits.data_ptr() if d_hits is not None else 0,
        d_hit_queries=d_hq.data_ptr() if d_hq is not None else 0,
        hits_per_query=0 if d_hq is not None else hits_per_query or max(n_hits, 1),
        d_cigar=d_cig.data_ptr() if stride else 0, cigar_stride=stride,
        d_ids=d_ids.data_ptr() if d_ids is not None else 0, stream=stream, codon_table=table)
    bank.sync()
    rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
    cig = d_cig.cpu().numpy().view(np.uint32)
    if stride:
        assert [int(r["cigar_offset"]) for r in rec] == [h * stride for h in range(n_hits)]
    return S.alignments_from(rec, cig)


def _expected(bank, seqs, frames, pairs, ids=None, stride=None, table=None):
    """What the frame call must return for the (query, target) pairs: align_set_hits on a batch
    holding the model's translation of each pair's frame, then the record rules."""
    trans = [F.translate(seqs[k], int(frames[i][k]), table) for i, k in pairs]
    res, offs, lens = S.pack_targets(trans)
    base = bank.align_set_hits(res, offs, lens, hit_queries=[i for i, _ in pairs])
    out = []
    for (i, k), e in zip(pairs, base):
        if stride is not None and len(e.ops) > stride:  # the caller's CIGAR space is too small
            e = dataclasses.replace(e, flags=e.flags | S.ALIGN_NO_PATH, n_columns=0,
                                    n_identities=0, ops=(), cigar="")
        out.append(F.frame_record(e, int(frames[i][k]), len(seqs[k]), k,
                                  int(ids[k]) if ids is not None else k))
    return out, trans


@pytest.mark.parametrize("model", MODELS)
def test_chain_and_alignments_of_the_top_hits(model):
    """score_frames -> top_hits -> align_frame_hits on one stream with no host step; every record
    is the set call's on the model's translation under the record rules, its CIGAR re-scores to
    its score over the translated codes, and the host form agrees."""
    torch = _torch()
    qs, seqs, planted, want = _case()
    wsc, wfr, _ = want[model]
    bt = Batch(seqs)
    ids = np.arange(bt.n, dtype=np.uint64) * 7 + 1000
    k, nq, dev = 8, 3, torch.device("cuda", 0)
    stride = 2 * (bt.max_len // 3) + 1
    stream = torch.cuda.Stream()
    with _bank(model) as bank:
        bank.load_queries(qs)
        d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        d_fr, d_hits, d_ids = _filled(nq * bt.n), _filled(nq * k * 8), _to_dev(ids)
        d_out = _filled(nq * k * S.ALIGNMENT_DTYPE.itemsize)
        d_cig = torch.full((nq * k * stride,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_frames_device(*bt.ptrs(), bt.n, bt.max_len, d_sc.data_ptr(),
                                 d_frames=d_fr.data_ptr(), stream=h)
        bank.top_hits_device(d_sc.data_ptr(), bt.n, k, d_hits.data_ptr(), nq=nq, stream=h)
        bank.align_frame_hits_device(*bt.ptrs(), bt.n, bt.max_len, nq * k, d_out.data_ptr(),
                                     d_fr.data_ptr(), d_hits=d_hits.data_ptr(), hits_per_query=k,
                                     d_cigar=d_cig.data_ptr(), cigar_stride=stride, stream=h,
                                     d_ids=d_ids.data_ptr())
        assert bank.last_kernel() == f"align-frame i32 nq={nq} hits={nq * k} chunks=1"
        bank.sync()
        stream.synchronize()
        frames = d_fr.cpu().numpy().reshape(nq, bt.n)
        hits = d_hits.cpu().numpy().view(np.uint64).reshape(nq, k)
        assert np.array_equal(frames, wfr)
        alns = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                                 d_cig.cpu().numpy().view(np.uint32))
        pairs = [(i, int(hits[i][j])) for i in range(nq) for j in range(k)]
        exp, trans = _expected(bank, seqs, frames, pairs, ids)
        host = bank.align_frame_hits(bt.res, bt.offs, bt.lens, frames, hits=hits.reshape(-1),
                                     hits_per_query=k, ids=ids)
        assert bank.last_kernel().startswith(f"align-frame i32 nq={nq} hits={nq * k} chunks=")
    assert {f for i, t in pairs for f in [int(frames[i][t])]} == set(range(6))
    for (i, t), a, e, hrec, tr in zip(pairs, alns, exp, host, trans):
        f, L = int(frames[i][t]), len(seqs[t])
        assert a == e == hrec, ((i, t), a, e, hrec)
        assert (a.index, a.id, a.score, a.frame) == (t, int(ids[t]), int(wsc[i][t]), f)
        assert a.flags == F.frame_flags(f) and a.has_path and a.reverse == (f >= 3)
        assert 0 <= a.t_start <= a.t_end < L
        # the nucleotide range back to amino positions, and the CIGAR re-scored over them
        o = f % 3
        a_start = (a.t_start - o) // 3 if f < 3 else (L - 1 - a.t_end - o) // 3
        a_end = (a.t_end - o - 2) // 3 if f < 3 else (L - 1 - a.t_start - o - 2) // 3
        assert F.nt_coords(a_start, a_end, f, L) == (a.t_start, a.t_end)
        s, dq, dt, cols, idn = AC.rescore(a.ops, qs[i], tr, a.q_start, a_start, O.BLOSUM62,
                                          *F.PEN, model)
        assert (s, dq, dt) == (a.score, a.q_end - a.q_start + 1, a_end - a_start + 1)
        assert (cols, idn) == (a.n_columns, a.n_identities)
    best = {i: alns[i * k] for i in range(nq)}  # a planted query aligns end to end, no gaps
    for i in range(nq):
        assert best[i].cigar == f"{len(qs[i])}M" and best[i].n_identities == len(qs[i])


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("table", ["standard", "stop-x"])
def test_asymmetric_matrix(table, model):
    """asym-prot at -11 / -1 through the frames (tests/matrix_cases.frame_case: the transposed
    matrix changes the frame score of 25-27 of the 27 planted targets, tests/test_frame_cases.py):
    scores and frames against the oracle on the model's translations, device and host form;
    align_frame_hits, host and device, on each query's 12 best hits against align_set_hits on
    the model's translation under the record rules, the CIGAR re-scored over the translated
    codes under the asymmetric matrix.  The custom table (two more stops, a codon for X; X and
    * in the queries) reads rows and columns 22 / 23 of the matrix."""
    tab = MC.stop_x_table() if table == "stop-x" else None
    sub = SEAMS.MATRICES[MC.PROTEIN]()
    pen = MC.MATRIX_SETS[MC.PROTEIN]
    qs, seqs, planted = MC.frame_case(tab)
    wsc, wfr = MC.frame_oracle(tab, model)
    nq, k = len(qs), 12
    bt = Batch(seqs)
    stride = 2 * (bt.max_len // 3) + 1
    hits = np.stack([np.argsort(-wsc[i].astype(np.int64), kind="stable")[:k] for i in range(nq)])
    pairs = [(i, int(hits[i][j])) for i in range(nq) for j in range(k)]
    hv = hits.reshape(-1).astype(np.uint64)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=model) as bank:
        bank.set_matrix(sub, *pen)
        bank.load_queries(qs)
        got, gfr, name = _score_device(bank, bt, nq, table=tab)
        assert name == f"frames nq={nq} n={bt.n} slices=1"
        bad = np.nonzero(got != wsc)
        assert bad[0].size == 0, (bad, got[bad], wsc[bad])
        assert np.array_equal(gfr, wfr)
        sc, fr = bank.score_frames(bt.res, bt.offs, bt.lens, codon_table=tab)
        assert np.array_equal(sc, wsc) and np.array_equal(fr, wfr)
        exp, trans = _expected(bank, seqs, wfr, pairs, table=tab)
        dev = _device_align(bank, bt, wfr, hv, stride, hits_per_query=k, table=tab)
        assert bank.last_kernel() == f"align-frame i32 nq={nq} hits={nq * k} chunks=1"
        host = bank.align_frame_hits(bt.res, bt.offs, bt.lens, wfr, hits=hv, hits_per_query=k,
                                     codon_table=tab)
    frames = {int(wfr[i][t]) for i, t in pairs}
    assert len(frames) >= 5 and min(frames) < 3 <= max(frames)
    gapped, windows = 0, []
    for (i, t), a, e, hrec, tr in zip(pairs, dev, exp, host, trans):
        f, L = int(wfr[i][t]), len(seqs[t])
        assert a == e == hrec, ((i, t), a, e, hrec)
        assert (a.index, a.score, a.frame) == (t, int(wsc[i][t]), f)
        assert a.flags == F.frame_flags(f) and a.has_path and 0 <= a.t_start <= a.t_end < L
        o = f % 3
        a_start = (a.t_start - o) // 3 if f < 3 else (L - 1 - a.t_end - o) // 3
        a_end = (a.t_end - o - 2) // 3 if f < 3 else (L - 1 - a.t_start - o - 2) // 3
        assert F.nt_coords(a_start, a_end, f, L) == (a.t_start, a.t_end)
        s, dq, dt, cols, idn = AC.rescore(a.ops, qs[i], tr, a.q_start, a_start, sub, *pen, model)
        assert (s, dq, dt) == (a.score, a.q_end - a.q_start + 1, a_end - a_start + 1)
        assert (cols, idn) == (a.n_columns, a.n_identities)
        gapped += len(a.ops) > 1
        windows.append((qs[i][a.q_start:a.q_end + 1], tr[a_start:a_end + 1]))
    assert gapped >= 4
    if tab is not None:  # X and * lie inside the aligned windows, on either side
        for side in (0, 1):
            codes = np.concatenate([w[side] for w in windows])
            assert (codes == F.X).any() and (codes == F.STOP).any()


@pytest.mark.parametrize("form", ["host", "device"])
def test_sentinels_empty_pairs_and_short_cigar_space(form):
    """Sentinel slots of either kind, an empty pair on a frame the caller names (the frame flags
    are set, the coordinates stay 0), repeats, and a cigar_stride of 1: paths of more ops get
    SW_ALIGN_NO_PATH with exact coordinates."""
    qs, seqs, planted, want = _case()
    wsc, wfr, _ = want[O.GAP_GOTOH]
    frames = wfr.copy()
    assert len(seqs[0]) == 0 and len(seqs[3]) == 2 and wsc[1][0] == 0
    frames[1][0], frames[2][3] = 4, 2  # pairs without a codon, on frames of the caller's choice
    # two more targets: query 1 with two codons deleted (a gap in every optimal path), in frame 1
    # of the first and, the second being its reverse complement, in frame 4 of that
    rng = np.random.default_rng(89)
    core = np.delete(F.back_translate(rng, qs[1]), slice(150, 156))
    gapped = np.concatenate([rng.integers(0, 4, 31), core, rng.integers(0, 4, 20)]).astype(np.uint8)
    n0 = len(seqs)
    seqs = seqs + [gapped, F.SC.revcomp(gapped)]
    frames = np.concatenate([frames, np.tile(np.array([1, 4], np.uint8), (3, 1))], axis=1)
    plants = list(planted)[:10]
    pairs = [(planted[k][0], k) for k in plants] + [(1, 0), (2, 3), (0, plants[0]), (1, 17), (2, 40)]
    pairs += [(int(i), int(k)) for i, k in zip(*np.nonzero(wsc > 40))][:12] + [(1, n0), (1, n0 + 1)]
    hq = np.array([i for i, _ in pairs], np.uint32)
    hv = np.array([k for _, k in pairs], np.uint64)
    none = [2, 14, 16]
    hq[none[0]], hv[none[1]], hq[none[2]], hv[none[2]] = S.QUERY_NONE, S.HIT_NONE, S.QUERY_NONE, S.HIT_NONE
    bt = Batch(seqs)
    with _bank() as bank:
        bank.load_queries(qs)
        for stride in (2 * (bt.max_len // 3) + 1, 1):
            exp, _ = _expected(bank, seqs, frames, pairs, stride=stride)
            if form == "device":
                alns = _device_align(bank, bt, frames, hv, stride, hit_queries=hq)
            elif stride > 1:
                alns = bank.align_frame_hits(bt.res, bt.offs, bt.lens, frames, hits=hv,
                                             hit_queries=hq)
            else:
                continue  # (the host form packs its CIGARs: it has no stride)
            assert bank.last_kernel().startswith(f"align-frame i32 nq=3 hits={len(pairs)} chunks=")
            for h, (a, e) in enumerate(zip(alns, exp)):
                if h in none:
                    assert (a.index, a.id, a.score, a.flags) == \
                        (S.HIT_NONE, S.HIT_NONE, 0, S.ALIGN_EMPTY | S.ALIGN_NO_HIT), (h, a)
                else:
                    assert a == e, (h, pairs[h], a, e)
            assert alns[10].flags == S.ALIGN_EMPTY | F.frame_flags(4) and alns[10].frame == 4
            assert alns[11].flags == S.ALIGN_EMPTY | F.frame_flags(2)
            assert (alns[10].t_start, alns[10].t_end, alns[10].index) == (0, 0, 0)
            kinds = {a.flags & S.ALIGN_NO_PATH for h, a in enumerate(alns)
                     if h not in none and a.score > 0}
            assert kinds == ({0} if stride > 1 else {0, S.ALIGN_NO_PATH})
        # coordinates only
        if form == "host":
            alns = bank.align_frame_hits(bt.res, bt.offs, bt.lens, frames, hits=hv, hit_queries=hq,
                                         cigar_cap=0)
        else:
            alns = _device_align(bank, bt, frames, hv, 0, hit_queries=hq)
        exp, _ = _expected(bank, seqs, frames, pairs, stride=0)
        for h, (a, e) in enumerate(zip(alns, exp)):
            assert h in none or a == e, (h, a, e)


def test_multi_device_bank():
    qs, seqs, _, want = _case()
    wsc, wfr, _ = want[O.GAP_GOTOH]
    bt = Batch(seqs)
    with _bank(devices=[0, 0]) as bank:
        bank.load_query(qs[1])
        got, gfr, name = _score_device(bank, bt, 1)
        assert name.startswith("frames nq=1")
        assert np.array_equal(got[0], wsc[1]) and np.array_equal(gfr[0], wfr[1])
        hv = np.argsort(-wsc[1].astype(np.int64), kind="stable")[:4].astype(np.uint64)
        alns = _device_align(bank, bt, wfr[1:2], hv, 2 * (bt.max_len // 3) + 1, hits_per_query=4)
        assert bank.last_kernel().startswith("align-frame i32 nq=1 hits=4")
    with _bank() as bank:
        bank.load_query(qs[1])
        assert alns == _device_align(bank, bt, wfr[1:2], hv, 2 * (bt.max_len // 3) + 1,
                                     hits_per_query=4)


# ---- 4. refusals ------------------------------------------------------------------------------------
def test_refusals():
    qs, seqs, _, want = _case()
    bt = Batch(seqs[:8])
    res, offs, lens = S.pack_targets(seqs[:8])
    buf = _filled(1 << 16)
    hv = np.arange(4, dtype=np.uint64)
    fr = np.zeros(8, np.uint8)
    p = buf.data_ptr()

    def status(fn, *a, **kw):
        with pytest.raises(S.SwbankError) as ei:
            fn(*a, **kw)
        return ei.value.status

    # a DNA bank: every new call
    with S.ScoreBank() as bank:
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(np.arange(20, dtype=np.uint8) % 4)
        assert status(bank.translate_batch_device, *bt.ptrs(), bt.n, bt.max_len, p, 200, p,
                      p) == S.ERR_UNSUPPORTED
        assert status(bank.score_frames_device, *bt.ptrs(), bt.n, bt.max_len, p) == S.ERR_UNSUPPORTED
        assert status(bank.score_frames, res, offs, lens) == S.ERR_UNSUPPORTED
        assert status(bank.align_frame_hits, res, offs, lens, fr, hits=hv,
                      hits_per_query=4) == S.ERR_UNSUPPORTED
        assert status(bank.align_frame_hits_device, *bt.ptrs(), bt.n, bt.max_len, 4, p, p,
                      d_hits=p, hits_per_query=4) == S.ERR_UNSUPPORTED
    # state: no query (a protein bank starts with BLOSUM62 penalties)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN) as bank:
        assert status(bank.score_frames_device, *bt.ptrs(), bt.n, bt.max_len, p) == S.ERR_STATE
        assert status(bank.score_frames, res, offs, lens) == S.ERR_STATE
        assert status(bank.align_frame_hits, res, offs, lens, fr, hits=hv,
                      hits_per_query=4) == S.ERR_STATE
        assert status(bank.align_frame_hits_device, *bt.ptrs(), bt.n, bt.max_len, 4, p, p,
                      d_hits=p, hits_per_query=4) == S.ERR_STATE
        bank.load_query(qs[0])
        # argument errors
        bad_tab = F.standard_table()
        bad_tab[63] = 24
        assert status(bank.translate_batch_device, *bt.ptrs(), bt.n, bt.max_len, p, 200, p, p,
                      codon_table=bad_tab) == S.ERR_ARG
        assert status(bank.translate_batch_device, *bt.ptrs(), bt.n, bt.max_len, p,
                      bt.max_len // 3 - 1, p, p) == S.ERR_ARG  # out_stride too small
        assert status(bank.translate_batch_device, *bt.ptrs(), 0, bt.max_len, p, 200, p,
                      p) == S.ERR_ARG
        assert status(bank.translate_batch_device, 0, bt.d_offs.data_ptr(), bt.d_lens.data_ptr(),
                      bt.n, bt.max_len, p, 200, p, p) == S.ERR_ARG
        assert status(bank.score_frames_device, *bt.ptrs(), bt.n, bt.max_len, p,
                      codon_table=bad_tab) == S.ERR_ARG
        assert status(bank.score_frames, res, offs, lens, codon_table=bad_tab) == S.ERR_ARG
        assert status(bank.score_frames_device, *bt.ptrs(), bt.n, bt.max_len, 0) == S.ERR_ARG
        assert status(bank.score_frames_device, *bt.ptrs(), bt.n, 4, p, min_len=5) == S.ERR_ARG
        bad = res.copy()
        bad[int(offs[5]) + 1] = 5  # a host code of 5 or more (23 would be a protein code)
        assert status(bank.score_frames, bad, offs, lens) == S.ERR_ARG
        assert status(bank.align_frame_hits, bad, offs, lens, fr, hits=[5],
                      hits_per_query=1) == S.ERR_ARG
        assert len(bank.align_frame_hits(bad, offs, lens, fr, hits=[4], hits_per_query=1)) == 1
        assert status(bank.align_frame_hits, res, offs, lens, None, hits=hv,
                      hits_per_query=4) == S.ERR_ARG  # frames NULL
        assert status(bank.align_frame_hits_device, *bt.ptrs(), bt.n, bt.max_len, 4, p, 0,
                      d_hits=p, hits_per_query=4) == S.ERR_ARG
        fr6 = fr.copy()
        fr6[2] = 6
        assert status(bank.align_frame_hits, res, offs, lens, fr6, hits=hv,
                      hits_per_query=4) == S.ERR_ARG  # a host frame above 5
        assert len(bank.align_frame_hits(res, offs, lens, fr6, hits=[0, 1, 3],
                                         hits_per_query=3)) == 3  # (not a listed pair's)
        assert status(bank.align_frame_hits, res, offs, lens, fr, hits=hv, hit_queries=[0] * 4,
                      hits_per_query=4) == S.ERR_ARG
        assert status(bank.align_frame_hits, res, offs, lens, fr, hits=[99],
                      hits_per_query=1) == S.ERR_ARG
        assert status(bank.align_frame_hits, res, offs, lens, fr, hits=hv, codon_table=bad_tab,
                      hits_per_query=4) == S.ERR_ARG
        bank.score_frames_device(*bt.ptrs(), 0, bt.max_len, 0)  # an empty batch is fine
        bank.sync()
        # the device form takes a frame above 5 as a target without codons
        d6 = _device_align(bank, bt, fr6, hv, 9, hits_per_query=4)
        assert (d6[2].flags, d6[2].score, d6[2].index) == (S.ALIGN_EMPTY, 0, 2)
