"""Both DNA strands on the GPU (include/swbank.h "both DNA strands"): the reverse complement of a
batch against numpy, the strand-merged scores against the oracle on rc(target), the strand-aware
alignments against the forward expectations of tests/align_cases.py with the batch holding
rc(target), the chain score_strands -> top_hits -> hit_significance -> align_strand_hits on one
stream, and the refusals.  Every test runs with plain and with poisoned device buffers; the CPU
references are computed once per process and shared."""
import dataclasses

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_cases as C
import align_check as AC
import matrix_cases as MC
import strand_cases as SC

pytestmark = pytest.mark.gpu

FILL = 0x3C
ABC = [(tag, model) for tag in C.DNA_SETS for model in C.MODELS]
MODES = ["plan", "slot"]
RC_LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1021]


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
    """A packed batch on the device (16 zero bytes behind the last target)."""

    def __init__(self, seqs):
        self.seqs = [np.asarray(s, np.uint8) for s in seqs]
        res, self.offs, self.lens = S.pack_targets(self.seqs)
        self.res = np.concatenate([res, np.zeros(16, np.uint8)])
        self.n = len(self.seqs)
        self.max_len = max(int(self.lens.max()), 1)
        self.min_len = int(self.lens.min())
        self.d_res, self.d_offs, self.d_lens = _to_dev(self.res), _to_dev(self.offs), _to_dev(self.lens)

    def ptrs(self):
        return self.d_res.data_ptr(), self.d_offs.data_ptr(), self.d_lens.data_ptr()


def _bank(pen=SC.REF, model=O.GAP_MERGED, **kw):
    bank = S.ScoreBank(gap_model=model, **kw)
    bank.set_penalties(*pen)
    return bank


# ---- 1. the reverse complement --------------------------------------------------------------------
def _gapped_batch(n, lens_pool):
    """n targets whose lengths walk through lens_pool, at odd byte offsets with 1-3 guard bytes
    between them, N codes included: (residues, offsets, lengths, the mask of the targets' bytes)."""
    rng = np.random.default_rng([n, len(lens_pool)])
    lens = np.array([lens_pool[(7 * k + 3) % len(lens_pool)] for k in range(n)], np.uint32)
    offs = np.zeros(n, np.int64)
    pos = 0
    for k in range(n):
        pos += int(rng.integers(1, 4))
        pos += (pos + 1) % 2  # every start is odd
        offs[k] = pos
        pos += int(lens[k])
    res = rng.integers(0, 5, pos + 5).astype(np.uint8)
    mask = np.zeros(len(res), bool)
    for k in range(n):
        mask[offs[k]:offs[k] + int(lens[k])] = True
    assert (offs % 2 == 1).all() and (res == 4).any()
    return res, offs.astype(np.uint64), lens, mask


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_revcomp_matches_numpy_byte_for_byte(n):
    torch = _torch()
    pool = RC_LENS[9:] + RC_LENS[:9] if n == 1 else RC_LENS  # (n = 1: one 127-code target)
    res, offs, lens, mask = _gapped_batch(n, pool)
    if n >= 63:
        assert set(RC_LENS) <= set(lens.tolist())
    want = np.full(len(res), FILL, np.uint8)
    for k in range(n):
        a, b = int(offs[k]), int(offs[k]) + int(lens[k])
        want[a:b] = SC.revcomp(res[a:b])
    d_res, d_offs, d_lens, d_out = _to_dev(res), _to_dev(offs), _to_dev(lens), _filled(len(res))
    torch.cuda.synchronize()
    with S.ScoreBank() as bank:  # neither penalties nor a query: the call needs none
        bank.revcomp_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n,
                                  d_out.data_ptr())
        assert bank.last_kernel() == f"revcomp n={n}"
        bank.sync()
        got = d_out.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
        assert (got[~mask] == FILL).all()            # the guard bytes survive
        assert np.array_equal(d_res.cpu().numpy(), res)  # the input is left alone
        # twice is the identity
        d_back = _filled(len(res))
        torch.cuda.synchronize()
        bank.revcomp_batch_device(d_out.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n,
                                  d_back.data_ptr())
        bank.sync()
        assert np.array_equal(d_back.cpu().numpy()[mask], res[mask])


def test_revcomp_one_long_target_among_short_ones():
    """The kernel has one path for every length (a wave runs until its longest target is done):
    a 70,000-code target in a wave with short and empty ones."""
    torch = _torch()
    res, offs, lens, mask = _gapped_batch(67, [70000, 5, 0, 300] + [33] * 63)
    assert lens.max() == 70000 and (lens == 0).any()
    want = np.full(len(res), FILL, np.uint8)
    for k in range(len(lens)):
        a, b = int(offs[k]), int(offs[k]) + int(lens[k])
        want[a:b] = SC.revcomp(res[a:b])
    d_res, d_offs, d_lens, d_out = _to_dev(res), _to_dev(offs), _to_dev(lens), _filled(len(res))
    torch.cuda.synchronize()
    with S.ScoreBank() as bank:
        bank.revcomp_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), len(lens),
                                  d_out.data_ptr())
        bank.sync()
    assert np.array_equal(d_out.cpu().numpy(), want)


# ---- 2. the strand-merged scores ---------------------------------------------------------------
def _want(qs, seqs, pen, model):
    """(merged [nq, n], strands [nq, n], forward, reverse) by the oracle."""
    pairs = [SC.oracle_strands(q, seqs, pen, model) for q in qs]
    fwd, rev = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return (*SC.merge(fwd, rev), fwd, rev)


def _slices(n, nq, max_len, resident, mb=1):
    """The slices of a call under SWBANK_STRAND_MB=mb: per target nq scores and, without a
    resident rc, its codes at a stride of max_len rounded up to 16, plus 16, and an offset."""
    per = 4 * nq + (0 if resident else (max_len + 15) // 16 * 16 + 16 + 8)
    span = min(n, max(1, (mb << 20) // per))
    return -(-n // span)


def _score_device(bank, bt, nq, d_rc=0, strands=True):
    torch = _torch()
    dev = torch.device("cuda", 0)
    d_sc = torch.full((nq * bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_st = _filled(nq * bt.n)
    torch.cuda.synchronize()
    bank.score_strands_device(*bt.ptrs(), bt.n, bt.max_len, d_sc.data_ptr(),
                              d_strands=d_st.data_ptr() if strands else 0, d_rc=d_rc,
                              min_len=bt.min_len)
    name = bank.last_kernel()
    bank.sync()
    return (d_sc.cpu().numpy().reshape(nq, bt.n), d_st.cpu().numpy().reshape(nq, bt.n), name)


def _resident_rc(bank, bt):
    d_rc = _filled(len(bt.res))
    d_rc.zero_()
    _torch().cuda.synchronize()
    bank.revcomp_batch_device(*bt.ptrs(), bt.n, d_rc.data_ptr())
    bank.sync()
    return d_rc


@pytest.mark.parametrize("model", C.MODELS)
def test_score_data500(model):
    """The reference's library: the fixture's forward / reverse / strand columns, the host and
    the device form, d_rc given and NULL bitwise equal."""
    names, q, seqs = SC.data500()
    rows = SC.load_strands500()
    want_sc = np.array([max(r[1], r[2]) for r in rows], np.int32)
    want_st = np.array([r[3] for r in rows], np.uint8)
    bt = Batch(seqs)
    with _bank(model=model) as bank:
        bank.load_query(q)
        sc, st = bank.score_strands(bt.res, bt.offs, bt.lens)
        assert np.array_equal(sc, want_sc) and np.array_equal(st, want_st)
        got, gst, name = _score_device(bank, bt, 1)
        assert name == f"strands nq=1 n={bt.n} slices=1"
        assert np.array_equal(got[0], want_sc) and np.array_equal(gst[0], want_st)
        d_rc = _resident_rc(bank, bt)
        got2, gst2, _ = _score_device(bank, bt, 1, d_rc=d_rc.data_ptr())
        assert np.array_equal(got2, got) and np.array_equal(gst2, gst)
        got3, gst3, _ = _score_device(bank, bt, 1, strands=False)  # d_strands NULL
        assert np.array_equal(got3, got) and (gst3 == FILL).all()
    order = np.argsort(-got[0].astype(np.int64), kind="stable")[:3]
    assert [(names[k], "fr"[gst[0][k]], int(got[0][k])) for k in order] == \
        [("db35", "r", 83), ("db198", "r", 79), ("db211", "f", 78)]


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(41)
    q = rng.integers(0, 4, 100).astype(np.uint8)
    seqs = [C.planted(rng, q, int(L)) if k % 3 == 0 else rng.integers(0, 5, int(L)).astype(np.uint8)
            for k, L in enumerate(rng.integers(64, 151, 4097))]
    seqs[5] = SC.revcomp(C.planted(rng, q, 120))
    return q, seqs, {m: _want([q], seqs, SC.REF, m) for m in C.MODELS}


@pytest.mark.parametrize("model", C.MODELS)
def test_score_ragged_and_slices(ragged, model, monkeypatch):
    """Ragged 64-150 bp, n = 4097 (N codes included): the oracle's numbers, with and without a
    resident rc, bitwise equal (4097 such targets fit 1 MiB of scratch: the sliced runs are
    test_score_slices)."""
    q, seqs, want = ragged
    wsc, wst, fwd, rev = want[model]
    assert wst.any() and not wst.all()
    bt = Batch(seqs)
    with _bank(model=model) as bank:
        bank.load_query(q)
        got, gst, name = _score_device(bank, bt, 1)
        assert name == f"strands nq=1 n={bt.n} slices=1"
        assert np.array_equal(got, wsc) and np.array_equal(gst, wst)
        monkeypatch.setenv("SWBANK_STRAND_MB", "1")
        d_rc = _resident_rc(bank, bt)
        for rc in (0, d_rc.data_ptr()):
            got2, gst2, name = _score_device(bank, bt, 1, d_rc=rc)
            assert name == f"strands nq=1 n={bt.n} slices={_slices(bt.n, 1, bt.max_len, rc != 0)}"
            assert np.array_equal(got2, got) and np.array_equal(gst2, gst)


def test_score_slices(monkeypatch):
    """A set of three queries of different lengths, and one query, over 9001 targets at
    SWBANK_STRAND_MB=1: several slices (a slice's reverse scores are nq rows of its own width),
    the same numbers bit for bit."""
    rng = np.random.default_rng(43)
    qs = [rng.integers(0, 4, n).astype(np.uint8) for n in (37, 100, 300)]
    seqs = [C.planted(rng, qs[k % 3], int(L)) if k % 2 else rng.integers(0, 4, int(L)).astype(np.uint8)
            for k, L in enumerate(rng.integers(90, 141, 9001))]
    for k in range(0, 9001, 7):
        seqs[k] = SC.revcomp(seqs[k])
    wsc, wst, _, _ = _want(qs, seqs, SC.REF, O.GAP_MERGED)
    bt = Batch(seqs)
    with _bank() as bank:
        bank.load_queries(qs)
        got, gst, name = _score_device(bank, bt, 3)
        assert name == f"strands nq=3 n={bt.n} slices=1"
        assert np.array_equal(got, wsc) and np.array_equal(gst, wst)
        monkeypatch.setenv("SWBANK_STRAND_MB", "1")
        got2, gst2, name = _score_device(bank, bt, 3)
        # per target: 144 + 16 rc bytes, an offset and three scores = 180 bytes -> 5825 a slice
        assert _slices(bt.n, 3, bt.max_len, False) == 2
        assert name == f"strands nq=3 n={bt.n} slices=2"
        assert np.array_equal(got2, got) and np.array_equal(gst2, gst)
        sc, st = bank.score_strands(bt.res, bt.offs, bt.lens)
        assert np.array_equal(sc, got) and np.array_equal(st, gst)
        bank.load_query(qs[1])
        one, ost, name = _score_device(bank, bt, 1)
        assert name == f"strands nq=1 n={bt.n} slices=2"
        assert np.array_equal(one[0], wsc[1]) and np.array_equal(ost[0], wst[1])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_score_small_batches(n):
    rng = np.random.default_rng(n)
    q = rng.integers(0, 4, 64).astype(np.uint8)
    seqs = [C.planted(rng, q, 128) for _ in range(n)]
    seqs = [SC.revcomp(s) if k % 2 else s for k, s in enumerate(seqs)]
    wsc, wst, _, _ = _want([q], seqs, SC.REF, O.GAP_MERGED)
    bt = Batch(seqs)
    with _bank() as bank:
        bank.load_query(q)
        got, gst, _ = _score_device(bank, bt, 1)
    assert np.array_equal(got, wsc) and np.array_equal(gst, wst)


def test_score_ties_empty_and_rescore():
    """Palindromic targets (ACGT repeated: rc(t) == t) tie and stay forward; an empty target
    scores 0 on strand 0; a 600-base query against its own reverse complement scores 3000 on the
    reverse strand, past the 16-bit lanes' f16 bound, so that pass alone re-scores."""
    rng = np.random.default_rng(47)
    q = rng.integers(0, 4, 600).astype(np.uint8)
    pal = np.tile(S.encode("ACGT"), 32)
    assert np.array_equal(SC.revcomp(pal), pal)
    seqs = [pal, np.zeros(0, np.uint8), SC.revcomp(q), pal[:60], rng.integers(0, 4, 600).astype(np.uint8)]
    for model in C.MODELS:
        wsc, wst, fwd, rev = _want([q], seqs, SC.REF, model)
        assert rev[0][2] == 3000 and fwd[0][2] < 2048 and wst[0].tolist()[:4] == [0, 0, 1, 0]
        assert fwd[0][0] == rev[0][0] and wsc[0][1] == 0
        bt = Batch(seqs)
        with _bank(model=model) as bank:
            bank.load_query(q)
            got, gst, _ = _score_device(bank, bt, 1)
            assert np.array_equal(got, wsc) and np.array_equal(gst, wst)
            sc, st = bank.score_strands(bt.res, bt.offs, bt.lens)
            assert np.array_equal(sc, wsc[0]) and np.array_equal(st, wst[0])


def test_score_multi_device_bank(ragged):
    q, seqs, want = ragged
    wsc, wst, _, _ = want[O.GAP_MERGED]
    bt = Batch(seqs)
    with _bank(devices=[0, 0]) as bank:
        bank.load_query(q)
        got, gst, name = _score_device(bank, bt, 1)
        assert name.startswith("strands nq=1")
        assert np.array_equal(got, wsc) and np.array_equal(gst, wst)


def test_score_timing_brackets_rc_and_merge():
    names, q, seqs = SC.data500()
    bt = Batch(seqs)
    with _bank() as bank:
        bank.load_query(q)
        _score_device(bank, bt, 1)
        bank.set_timing(True)
        _score_device(bank, bt, 1)
        with_rc, _, ms = bank.timing()
        d_rc = _resident_rc(bank, bt)
        bank.timing()
        _score_device(bank, bt, 1, d_rc=d_rc.data_ptr())
        resident, _, _ = bank.timing()
    assert with_rc == resident + 1 and resident >= 3 and ms > 0  # two passes, the merge (+ the rc)


# ---- 3. strand-aware alignments ----------------------------------------------------------------
def _device_align(bank, seqs, hits, strands, stride, hit_queries=None, hits_per_query=0):
    """sw_align_strand_hits_device on torch buffers -> Alignment objects."""
    torch = _torch()
    bt = Batch(seqs)
    n_hits = len(hits) if hits is not None else len(hit_queries)
    d_hits = _to_dev(np.asarray(hits, np.uint64)) if hits is not None else None
    d_hq = _to_dev(np.asarray(hit_queries, np.uint32)) if hit_queries is not None else None
    d_st = _to_dev(np.asarray(strands, np.uint8).reshape(-1)) if strands is not None else None
    d_out = _filled(n_hits * S.ALIGNMENT_DTYPE.itemsize)
    d_cig = torch.full((max(1, n_hits * stride),), 0x3C3C3C3C, dtype=torch.int32,
                       device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    bank.align_strand_hits_device(
        *bt.ptrs(), bt.n, bt.max_len, n_hits, d_out.data_ptr(),
        d_strands=d_st.data_ptr() if d_st is not None else 0,
        d_hits=d_hits.data_ptr() if d_hits is not None else 0,
        d_hit_queries=d_hq.data_ptr() if d_hq is not None else 0,
        hits_per_query=0 if d_hq is not None else hits_per_query or max(n_hits, 1),
        d_cigar=d_cig.data_ptr() if stride else 0, cigar_stride=stride)
    bank.sync()
    rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
    cig = d_cig.cpu().numpy().view(np.uint32)
    if stride:
        assert [int(r["cigar_offset"]) for r in rec] == [h * stride for h in range(n_hits)]
    return S.alignments_from(rec, cig), rec, cig


def _align(bank, mode, seqs, hits, strands):
    if mode == "plan":
        res, offs, lens = S.pack_targets(seqs)
        alns = bank.align_strand_hits(res, offs, lens, strands=strands, hits=hits,
                                      hits_per_query=max(len(hits), 1))
    else:
        alns = _device_align(bank, seqs, hits, strands, 2 * max(len(s) for s in seqs) + 1)[0]
    assert bank.last_kernel().startswith(f"align-strand i32 nq=1 hits={len(hits)} chunks="), \
        bank.last_kernel()
    return alns


def _expect(g, h):
    """The forward expectation of the family's target h as an Alignment (no cigar text)."""
    s, qs, qe, ts, te = g.brute[h]
    r = g.refs[h]
    if r is None:
        return S.Alignment(h, h, 0, S.ALIGN_EMPTY, 0, 0, 0, 0, 0, 0)
    return S.Alignment(h, h, s, 0, qs, qe, ts, te, r.n_columns, r.n_identities, tuple(r.ops),
                       S.cigar_string(r.ops))


def _run_group(P, g, mode):
    """The family with the batch holding rc(t) and strand 1: flip_record of its forward
    expectation, op for op (rc(rc(t)) = t: the strand path crosses every seam the forward path
    is tested at)."""
    seqs = [SC.revcomp(t) for t in g.seqs]
    with _bank((int(P.sub[0][0]), int(P.sub[0][1]), P.go, P.ge), P.model) as bank:
        bank.load_query(g.q)
        alns = _align(bank, mode, seqs, g.hits, np.ones(len(seqs), np.uint8))
        chunks = int(bank.last_kernel().split("chunks=")[1])
    assert len(alns) == len(g.hits)
    for h, a in zip(g.hits, alns):
        want = SC.flip_record(_expect(g, h), len(g.seqs[h]))
        assert a == want, (g.name, h, a, want)
        assert a.reverse and a.t_start <= a.t_end
    return chunks


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_pass_seams_on_the_reverse_strand(tag, model, mode):
    P = C.dna_param(tag, model)
    assert _run_group(P, C.seam_family(P), mode) == 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_pass_seams_chunked_on_the_reverse_strand(tag, model, mode, monkeypatch):
    """The budget path: a direction store of 1 MiB, several chunks, by plan and by slot."""
    monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
    P = C.dna_param(tag, model)
    assert _run_group(P, C.seam_family(P), mode) > 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_window_edges_on_the_reverse_strand(tag, model, mode):
    P = C.dna_param(tag, model)
    _run_group(P, C.edge_family(P), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_ties_on_the_reverse_strand(tag, model, mode):
    P = C.dna_param(tag, model)
    for g in C.tie_family(P):
        _run_group(P, g, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", C.MODELS)
def test_tie_rich_paths_on_the_reverse_strand(model, mode):
    for g, tag in zip(C.tie_rich_family(model), C.TIE_SETS):
        _run_group(C.dna_param(tag, model, C.TIE_SETS), g, mode)


def _matrix_bank(P):
    bank = S.ScoreBank(gap_model=P.model)
    bank.set_matrix(P.sub, P.go, P.ge)
    return bank


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,model", MC.DNA_PARAMS)
def test_asymmetric_matrices_on_alternating_strands(name, model, mode):
    """The matrix family of tests/matrix_cases.py, forward hits on t and reverse hits on the
    stored rc(t) by turns.  A reverse hit is walked under smat'[q][c] = smat[q][comp c]: built
    from the uncomplemented matrix, with the rows complemented, from the transposed matrix or
    with both sides complemented it would change 94-100 % of these scores
    (tests/test_strand_cases.py), which no match / mismatch table shows for the second and
    third.  Records equal the flipped references op for op, and a reverse hit's counts are
    recomputed from its ops on the reverse complement of the stored target."""
    P = MC.matrix_param(name, model)
    g = MC.matrix_family(P)
    stored, strands = MC.strand_form(g)
    with _matrix_bank(P) as bank:
        bank.load_query(g.q)
        alns = _align(bank, mode, stored, g.hits, strands)
    assert len(alns) == len(g.hits)
    gapped = 0
    for h, a in zip(g.hits, alns):
        want, L = _expect(g, h), len(stored[h])
        if strands[h]:
            want = SC.flip_record(want, L)
        assert a == want, (g.name, h, a, want)
        assert a.reverse == bool(strands[h])
        if strands[h] and a.score > 0:
            s, dq, dt, cols, idn = AC.rescore(a.ops, g.q, SC.revcomp(stored[h]), a.q_start,
                                              L - 1 - a.t_end, P.sub, P.go, P.ge, P.model)
            assert (s, dq, dt) == (a.score, a.q_end - a.q_start + 1, a.t_end - a.t_start + 1)
            assert (cols, idn) == (a.n_columns, a.n_identities), (h, a)
            gapped += len(a.ops) > 1
    assert gapped >= 6


def _set_case():
    """Three queries, 40 targets (every third one reverse-complemented, N codes, an empty one),
    the oracle's strand matrix, and per (query, target) the forward call's expectation on the
    strand's own target."""
    def make():
        rng = np.random.default_rng(53)
        qs = [rng.integers(0, 4, n).astype(np.uint8) for n in (60, 130, 300)]
        seqs = [C.planted(rng, qs[k % 3], int(L)) for k, L in enumerate(rng.integers(40, 200, 40))]
        seqs = [SC.revcomp(s) if k % 3 == 1 else s for k, s in enumerate(seqs)]
        seqs[7] = np.zeros(0, np.uint8)
        seqs[9][::5] = 4
        out = {}
        for model in C.MODELS:
            P = C.dna_param("ref", model)
            _, strands, _, _ = _want(qs, seqs, SC.REF, model)
            exp = {}
            for i, q in enumerate(qs):
                tt = [SC.revcomp(s) if strands[i][k] else s for k, s in enumerate(seqs)]
                brute, refs = C.prepare(q, tt, P)
                g = C.Group("set", q, tt, None, brute, refs, None)
                for k in range(len(seqs)):
                    e = _expect(g, k)
                    exp[(i, k)] = SC.flip_record(e, len(seqs[k])) if strands[i][k] else e
            out[model] = (strands, exp)
        return qs, seqs, out
    return C._cached("strand-set", make)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", C.MODELS)
def test_alternating_strands_and_sentinels(model, mode, monkeypatch):
    """A set: hits of both strands by turns in one hit list (with SWBANK_EDGE_MB=1 a wave takes
    several hits in turn, so one wave's list alternates too), sentinel slots of either kind,
    repeats; hit_queries and the [nq, k] layout."""
    qs, seqs, out = _set_case()
    strands, exp = out[model]
    n = len(seqs)
    rng = np.random.default_rng(59)
    pairs = [(int(i), int(k)) for i, k in zip(rng.integers(0, 3, 90), rng.integers(0, n, 90))]
    hq = np.array([i for i, _ in pairs], np.uint32)
    hv = np.array([k for _, k in pairs], np.uint64)
    hq[[4, 50]] = S.QUERY_NONE
    hv[[11, 50, 77]] = S.HIT_NONE
    kinds = [int(strands[i][k]) for (i, k), a, b in zip(pairs, hq, hv)
             if a != S.QUERY_NONE and b != S.HIT_NONE]
    assert 0 in kinds and 1 in kinds and any(x != y for x, y in zip(kinds, kinds[1:]))
    monkeypatch.setenv("SWBANK_EDGE_MB", "1")
    assert C.i32_waves(90, 200, 1 << 20) >= 4
    with _bank(model=model) as bank:
        bank.load_queries(qs)
        if mode == "plan":
            res, offs, lens = S.pack_targets(seqs)
            alns = bank.align_strand_hits(res, offs, lens, strands=strands, hits=hv, hit_queries=hq)
        else:
            alns = _device_align(bank, seqs, hv, strands, 2 * 200 + 1, hit_queries=hq)[0]
        assert bank.last_kernel().startswith("align-strand i32 nq=3 hits=90 chunks=")
        # the [nq, k] layout: row i = targets 0..k of query i
        k = 12
        grid = np.tile(np.arange(k, dtype=np.uint64), 3)
        if mode == "plan":
            alns2 = bank.align_strand_hits(res, offs, lens, strands=strands, hits=grid,
                                           hits_per_query=k)
        else:
            alns2 = _device_align(bank, seqs, grid, strands, 401, hits_per_query=k)[0]
    for h, a in enumerate(alns):
        if hq[h] == S.QUERY_NONE or hv[h] == S.HIT_NONE:
            assert (a.index, a.id, a.score, a.flags) == \
                (S.HIT_NONE, S.HIT_NONE, 0, S.ALIGN_EMPTY | S.ALIGN_NO_HIT), (h, a)
            assert not a.reverse
        else:
            assert a == exp[pairs[h]], (h, pairs[h], a, exp[pairs[h]])
    for h, a in enumerate(alns2):
        assert a == exp[(h // k, h % k)], (h, a)


@pytest.mark.parametrize("model", C.MODELS)
def test_null_strands_equal_the_set_call_byte_for_byte(model):
    torch = _torch()
    qs, seqs, out = _set_case()
    n = len(seqs)
    hv = np.tile(np.arange(n, dtype=np.uint64), 3)
    hv[5] = S.HIT_NONE
    stride = 401
    with _bank(model=model) as bank:
        bank.load_queries(qs)
        _, rec, cig = _device_align(bank, seqs, hv, None, stride, hits_per_query=n)
        assert bank.last_kernel().startswith("align-strand i32 nq=3")
        bt = Batch(seqs)
        d_hits = _to_dev(hv)
        d_out = _filled(len(hv) * S.ALIGNMENT_DTYPE.itemsize)
        d_cig = torch.full((len(hv) * stride,), 0x3C3C3C3C, dtype=torch.int32,
                           device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        bank.align_set_hits_device(*bt.ptrs(), bt.n, bt.max_len, len(hv), d_out.data_ptr(),
                                   d_hits=d_hits.data_ptr(), hits_per_query=n,
                                   d_cigar=d_cig.data_ptr(), cigar_stride=stride)
        bank.sync()
        assert d_out.cpu().numpy().tobytes() == rec.tobytes()
        assert d_cig.cpu().numpy().tobytes() == cig.tobytes()
        res, offs, lens = S.pack_targets(seqs)
        assert bank.align_strand_hits(res, offs, lens, hits=hv, hits_per_query=n) == \
            bank.align_set_hits(res, offs, lens, hits=hv, hits_per_query=n)
    # all-zero strands: the strand kernels on the forward strand give the same records
    with _bank(model=model) as bank:
        bank.load_queries(qs)
        _, rec0, cig0 = _device_align(bank, seqs, hv, np.zeros((3, n), np.uint8), stride,
                                      hits_per_query=n)
    assert rec0.tobytes() == rec.tobytes() and cig0.tobytes() == cig.tobytes()


@pytest.mark.parametrize("model", C.MODELS)
def test_null_strands_equal_the_set_call_under_an_asymmetric_matrix(model):
    """asym-ncol (a non-uniform N column, a positive N x N score): the matrix family against a
    set of three queries in the [nq, k] layout, a sentinel among the hits."""
    torch = _torch()
    P = MC.matrix_param("asym-ncol", model)
    g = MC.matrix_family(P)
    qs = MC.set_form(g)[0]
    n = len(g.seqs)
    hv = np.tile(np.arange(n, dtype=np.uint64), 3)
    hv[5] = S.HIT_NONE
    stride = 2 * MC.MAX_TLEN + 1
    with _matrix_bank(P) as bank:
        bank.load_queries(qs)
        alns, rec, cig = _device_align(bank, g.seqs, hv, None, stride, hits_per_query=n)
        assert bank.last_kernel().startswith("align-strand i32 nq=3")
        bt = Batch(g.seqs)
        d_hits = _to_dev(hv)
        d_out = _filled(len(hv) * S.ALIGNMENT_DTYPE.itemsize)
        d_cig = torch.full((len(hv) * stride,), 0x3C3C3C3C, dtype=torch.int32,
                           device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        bank.align_set_hits_device(*bt.ptrs(), bt.n, bt.max_len, len(hv), d_out.data_ptr(),
                                   d_hits=d_hits.data_ptr(), hits_per_query=n,
                                   d_cigar=d_cig.data_ptr(), cigar_stride=stride)
        bank.sync()
        assert d_out.cpu().numpy().tobytes() == rec.tobytes()
        assert d_cig.cpu().numpy().tobytes() == cig.tobytes()
        res, offs, lens = S.pack_targets(g.seqs)
        assert bank.align_strand_hits(res, offs, lens, hits=hv, hits_per_query=n) == \
            bank.align_set_hits(res, offs, lens, hits=hv, hits_per_query=n)
    for h in g.hits:  # row 0 is the family's own query: its records are the family's
        assert h == 5 or alns[h] == _expect(g, h), (h, alns[h])
    assert sum(1 for a in alns if len(a.ops) > 1) >= 30


# ---- 3b. the first-column rule on the reverse strand ----------------------------------------------
def test_first_column_rule_on_the_reverse_strand():
    """Merged 3 / -3 / -1 / -1 (max(s) > open + extend): the one rule that is not
    reversal-symmetric.  On a reverse hit the first column is the stored target's last code; on
    7 of the 24 reverse hits of tests/matrix_cases.col0_family the rule applied at the other end
    gives another score (tests/test_strand_cases.py).  Scores and strands against the oracle on
    rc(target): the device form with the bank's own complement and with a resident one, and
    the host form.  The alignment entries refuse these penalties (include/swbank.h: the start
    rule has no reversed problem), so the strand alignments have nothing to return."""
    g = MC.col0_family()
    P = MC.col0_param()
    pen = (3, -3, P.go, P.ge)
    stored, strands = MC.strand_form(g)
    wsc, wst, fwd, rev = _want([g.q], stored, pen, P.model)
    assert int(wst[0][strands == 1].sum()) >= 18
    bt = Batch(stored)
    with _bank(pen, P.model) as bank:
        bank.load_query(g.q)
        got, gst, name = _score_device(bank, bt, 1)
        assert name == f"strands nq=1 n={bt.n} slices=1"
        bad = np.nonzero(got[0] != wsc[0])[0]
        assert bad.size == 0, (bad, got[0][bad], wsc[0][bad], fwd[0][bad], rev[0][bad])
        assert np.array_equal(gst, wst)
        d_rc = _resident_rc(bank, bt)
        got2, gst2, _ = _score_device(bank, bt, 1, d_rc=d_rc.data_ptr())
        assert np.array_equal(got2, wsc) and np.array_equal(gst2, wst)
        sc, st = bank.score_strands(bt.res, bt.offs, bt.lens)
        assert np.array_equal(sc, wsc[0]) and np.array_equal(st, wst[0])
        hv = np.arange(bt.n, dtype=np.uint64)
        with pytest.raises(S.SwbankError) as ei:
            bank.align_strand_hits(bt.res, bt.offs, bt.lens, strands=wst, hits=hv,
                                   hits_per_query=bt.n)
        assert ei.value.status == S.ERR_UNSUPPORTED


def test_coordinates_only_and_short_cigar_space():
    """No CIGAR buffer: the flipped coordinates with SW_ALIGN_NO_PATH | SW_ALIGN_REVERSE."""
    qs, seqs, out = _set_case()
    strands, exp = out[O.GAP_MERGED]
    hv = np.arange(len(seqs), dtype=np.uint64)
    with _bank() as bank:
        bank.load_queries(qs)
        res, offs, lens = S.pack_targets(seqs)
        for alns in (bank.align_strand_hits(res, offs, lens, strands=strands, hits=hv,
                                            hits_per_query=len(hv), cigar_cap=0),
                     _device_align(bank, seqs, hv, strands, 0, hits_per_query=len(hv))[0]):
            for k, a in enumerate(alns):
                e = exp[(0, k)]
                want = e if e.empty else dataclasses.replace(
                    e, flags=e.flags | S.ALIGN_NO_PATH, n_columns=0, n_identities=0, ops=(),
                    cigar="")
                assert a == want, (k, a, want)


# ---- 4. the chain ---------------------------------------------------------------------------------
def test_chain_on_one_stream_db35_first():
    """score_strands -> top_hits -> hit_significance -> align_strand_hits on one stream with no
    host step: db35 [r] 83 25M2I10M comes first, as the fixture records it."""
    torch = _torch()
    names, q, seqs = SC.data500()
    gold = SC.load_strand_alignments500()
    bt = Batch(seqs)
    k, dev = 6, torch.device("cuda", 0)
    st = S.make_statistics(0.1840, 0.1293, len(q))
    stride = 2 * bt.max_len + 1
    stream = torch.cuda.Stream()
    with _bank() as bank:
        bank.load_query(q)
        d_sc = torch.full((bt.n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        d_st, d_hits, d_hsc = _filled(bt.n), _filled(k * 8), _filled(k * 4)
        d_bits, d_ev = _filled(k * 8), _filled(k * 8)
        d_out = _filled(k * S.ALIGNMENT_DTYPE.itemsize)
        d_cig = torch.full((k * stride,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        h = stream.cuda_stream
        bank.score_strands_device(*bt.ptrs(), bt.n, bt.max_len, d_sc.data_ptr(),
                                  d_strands=d_st.data_ptr(), stream=h)
        bank.top_hits_device(d_sc.data_ptr(), bt.n, k, d_hits.data_ptr(),
                             d_hit_scores=d_hsc.data_ptr(), stream=h)
        bank.hit_significance_device(st, d_hsc.data_ptr(), d_hits.data_ptr(), bt.d_lens.data_ptr(),
                                     k, 2 * bt.n, d_bits=d_bits.data_ptr(),
                                     d_evalues=d_ev.data_ptr(), stream=h)
        bank.align_strand_hits_device(*bt.ptrs(), bt.n, bt.max_len, k, d_out.data_ptr(),
                                      d_strands=d_st.data_ptr(), d_hits=d_hits.data_ptr(),
                                      hits_per_query=k, d_cigar=d_cig.data_ptr(),
                                      cigar_stride=stride, stream=h)
        assert bank.last_kernel() == f"align-strand i32 nq=1 hits={k} chunks=1"
        bank.sync()
        stream.synchronize()
    alns = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                             d_cig.cpu().numpy().view(np.uint32))
    got = [(names[a.index], "fr"[a.reverse], a.score) for a in alns]
    assert got == [("db35", "r", 83), ("db198", "r", 79), ("db211", "f", 78), ("db428", "f", 72),
                   ("db41", "r", 70), ("db454", "f", 70)]
    assert alns[0].cigar == "25M2I10M" and (alns[0].n_columns, alns[0].n_identities) == (37, 27)
    rev = [a for a in alns if a.reverse]
    assert len(rev) == len(gold)
    for a, r in zip(rev, gold):
        assert (names[a.index], a.index, a.score, a.q_start, a.q_end, a.t_start, a.t_end,
                a.n_columns, a.n_identities, a.cigar) == \
            (r["name"], r["index"], r["score"], r["q_start"], r["q_end"], r["t_start"], r["t_end"],
             r["n_columns"], r["n_identities"], r["cigar"])
    ev = d_ev.cpu().numpy().view(np.float64)
    want_ev = S.hit_significance(st, [a.score for a in alns], bt.lens[[a.index for a in alns]],
                                 2 * bt.n)[1]
    assert np.allclose(ev, want_ev, rtol=1e-10, atol=0)  # db_size: two strands, twice the library


# ---- 5. refusals ----------------------------------------------------------------------------------
def test_refusals():
    names, q, seqs = SC.data500()
    bt = Batch(seqs[:8])
    res, offs, lens = S.pack_targets(seqs[:8])
    buf = _filled(4096)
    hv = np.arange(4, dtype=np.uint64)

    def status(fn, *a, **kw):
        with pytest.raises(S.SwbankError) as ei:
            fn(*a, **kw)
        return ei.value.status

    # a protein bank: every new call
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=S.GAP_GOTOH) as bank:
        bank.set_matrix(O.BLOSUM62, -11, -1)
        bank.load_query(np.arange(20, dtype=np.uint8))
        assert status(bank.revcomp_batch_device, *bt.ptrs(), bt.n, buf.data_ptr()) == S.ERR_UNSUPPORTED
        assert status(bank.score_strands_device, *bt.ptrs(), bt.n, bt.max_len,
                      buf.data_ptr()) == S.ERR_UNSUPPORTED
        assert status(bank.score_strands, res, offs, lens) == S.ERR_UNSUPPORTED
        assert status(bank.align_strand_hits, res, offs, lens, hits=hv,
                      hits_per_query=4) == S.ERR_UNSUPPORTED
        assert status(bank.align_strand_hits_device, *bt.ptrs(), bt.n, bt.max_len, 4,
                      buf.data_ptr(), d_hits=buf.data_ptr(), hits_per_query=4) == S.ERR_UNSUPPORTED
    # state: no penalties, no query
    with S.ScoreBank() as bank:
        assert status(bank.score_strands_device, *bt.ptrs(), bt.n, bt.max_len,
                      buf.data_ptr()) == S.ERR_STATE
        bank.set_penalties(*SC.REF)
        assert status(bank.score_strands, res, offs, lens) == S.ERR_STATE
        assert status(bank.align_strand_hits, res, offs, lens, hits=hv,
                      hits_per_query=4) == S.ERR_STATE
        bank.load_query(q)
        # argument errors
        assert status(bank.revcomp_batch_device, 0, bt.d_offs.data_ptr(), bt.d_lens.data_ptr(),
                      bt.n, buf.data_ptr()) == S.ERR_ARG
        assert status(bank.revcomp_batch_device, *bt.ptrs(), 0, buf.data_ptr()) == S.ERR_ARG
        assert status(bank.score_strands_device, *bt.ptrs(), bt.n, bt.max_len, 0) == S.ERR_ARG
        assert status(bank.score_strands_device, *bt.ptrs(), bt.n, 4, buf.data_ptr(),
                      min_len=5) == S.ERR_ARG
        bad = res.copy()
        bad[3] = 9
        assert status(bank.score_strands, bad, offs, lens) == S.ERR_ARG
        assert status(bank.align_strand_hits, res, offs, lens, hits=hv, hit_queries=[0] * 4,
                      hits_per_query=4) == S.ERR_ARG
        assert status(bank.align_strand_hits, res, offs, lens, hits=[99], hits_per_query=1,
                      strands=np.zeros(8, np.uint8)) == S.ERR_ARG
        bank.score_strands_device(*bt.ptrs(), 0, bt.max_len, 0)  # an empty batch is fine
        bank.sync()
        assert status(bank.best) == S.ERR_STATE  # no best hit is tracked
    # merged gaps with max(s) > open + extend: refused as the align calls refuse it today
    with _bank((5, -4, -2, -1)) as bank:
        bank.load_query(q)
        assert status(bank.align_strand_hits, res, offs, lens, hits=hv, hits_per_query=4,
                      strands=np.zeros(8, np.uint8)) == S.ERR_UNSUPPORTED
        assert status(bank.align_strand_hits_device, *bt.ptrs(), bt.n, bt.max_len, 4,
                      buf.data_ptr(), d_hits=buf.data_ptr(), hits_per_query=4) == S.ERR_UNSUPPORTED
        sc, st = bank.score_strands(res, offs, lens)  # the scoring call takes them
        wsc, wst, _, _ = _want([q], seqs[:8], (5, -4, -2, -1), O.GAP_MERGED)
        assert np.array_equal(sc, wsc[0]) and np.array_equal(st, wst[0])
