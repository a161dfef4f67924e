"""The frameshift search, its aligner and its statistics across the accepted scoring envelope
(include/swbank.h "frameshift-tolerant translated search": 0 >= gap_open, gap_extend >= -32767,
any int8 matrix of span <= 254, exact int32), on the GPU.  Every comparison is exact equality with
the C models of tests/fshift_cases.py and tests/fsalign_cases.py over the inputs of
tests/fshift_envelope_cases.py (tests/test_fshift_envelope_cases.py checks those on the CPU: the
models against the plain-Python restatements under every case, the seam plants' liveness, the
transposed matrix): zero and four-digit gap penalties, matrices with no positive entry, +-127 and
-128 entries (the kernels' own pad score), the gap state across the score walk's lane and block
seams, pad rows and pad columns beside a hit, the CIGAR tie rules at go = 0, a seeded fuzz, the
two SW_ERR_RANGE refusals and the statistics of a degenerate and of a free-gap search.  The CPU
references are computed once per process and shared."""
import ctypes
import os

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import fsalign_cases as A
import fshift_cases as FS
import fshift_envelope_cases as E
import test_gpu_fsalign as TA
import test_gpu_fshift as TG

pytestmark = pytest.mark.gpu

CASE_K = [(c.name, K) for c in E.CASES for K in E.ROWS]


def _bank(case):
    bank = S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH)
    bank.set_matrix(E.matrix(case.matrix), case.go, case.ge)
    return bank


def _align_fs(case):
    return (-15, -32767) + ((0,) if case.go == 0 else ())


def _batches(name, K):
    """[(what, q, seqs)]: the noise batch, and the case's seam family where it has one (a batch of
    its own: its targets are up to eight times as long)."""
    def make():
        case = E.BY_NAME[name]
        out = [("noise",) + E.noise_batch(name, K)]
        if case in E.SEAM_CASES:
            q, plants, _ = E.seam_family(name, K)
            out.append(("seams", q, [p.target for p in plants]))
        return out
    return TG._cached(("env-batches", name, K), make)


def _want_scores(name, K, what, q, seqs, fs):
    case = E.BY_NAME[name]
    return TG._cached(("env-scores", name, K, what, fs),
                      lambda: FS.c_search(q, seqs, E.matrix(case.matrix), case.go, case.ge, fs))


def _want_aligned(name, K, what, q, seqs, pairs, fs):
    case = E.BY_NAME[name]
    return TG._cached(("env-aligned", name, K, what, fs),
                      lambda: TA._want([q], seqs, pairs, E.matrix(case.matrix), E.pen(case), fs))


def _score_both_forms(bank, bt, seqs, fs, want, what, table=None):
    got, gsd, _ = TG._score_device(bank, bt, 1, fs, table=table)
    TG._same(got[0], want[0], what + ("device scores",))
    TG._same(gsd[0], want[1], what + ("device strands",))
    sc, sd = bank.score_frameshift((bt.res, bt.offs, bt.lens), fs, codon_table=table)
    TG._same(sc, want[0], what + ("host scores",))
    TG._same(sd, want[1], what + ("host strands",))
    return got[0]


def _align_device(bank, bt, seqs, pairs, fs, want, scores, what, table=None):
    """The device form's records and ops against the model; every score is the score call's."""
    stride = max(len(w[1]) for w in want) + 1
    got = TA._device(bank, bt, pairs, fs, stride, table)
    TA._check(got, want, pairs, what)
    assert [a.score for a in got] == [int(scores[k]) for _, k in pairs], what


# ---- 1. scores and strands ------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", CASE_K)
def test_scores_across_the_envelope(name, K, poisoned_buffers):
    """Every case of the table at the kernel's three row counts, fs in {0, -1, -15, -32767}, the
    device and the host form, over the noise batch and the seam family, with poisoned device
    buffers."""
    case = E.BY_NAME[name]
    with _bank(case) as bank:
        for what, q, seqs in _batches(name, K):
            if not seqs:
                continue
            assert K == (4 if len(q) <= 256 else 8 if len(q) <= 512 else 16)
            bt = TG.Batch(seqs)
            bank.load_query(q)
            for fs in E.FS_VALUES:
                want = _want_scores(name, K, what, q, seqs, fs)
                _score_both_forms(bank, bt, seqs, fs, want, (name, K, what, fs))
                assert "nopos" not in case.tags or not want[0].any()
    if "nopos" in case.tags:
        return
    if "limit" not in case.tags:
        free = _want_scores(name, K, "noise", *E.noise_batch(name, K), 0)[0]
        dear = _want_scores(name, K, "noise", *E.noise_batch(name, K), -32767)[0]
        assert (free > dear).sum() >= 10  # the shifts are alive


# ---- 2. the aligner --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", CASE_K)
def test_alignments_across_the_envelope(name, K, poisoned_buffers):
    """align_frameshift_hits_device over every non-empty target of the same batches at
    fs = -15 and -32767, and at fs = 0 where go = 0: every record field and every op is the C
    model's, every score the score call's.  The go = 0 cases are the tie-rule cases (M, then E,
    then F; a gap opens rather than extends; the smallest column, then the smallest row): at
    fs = 0 at least 10 targets of their noise batch have an I or D op in the model's CIGAR and at
    least 10 reach their best value at more than one cell."""
    case = E.BY_NAME[name]
    sub = E.matrix(case.matrix)
    with _bank(case) as bank:
        for what, q, seqs in _batches(name, K):
            pairs = [(0, k) for k, t in enumerate(seqs) if len(t)]
            if not pairs:
                continue
            bt = TG.Batch(seqs)
            bank.load_query(q)
            for fs in _align_fs(case):
                want = _want_aligned(name, K, what, q, seqs, pairs, fs)
                scores, _, _ = TG._score_device(bank, bt, 1, fs)
                _align_device(bank, bt, seqs, pairs, fs, want, scores[0], f"{name} {K} {what} {fs}")
    if case.go == 0:
        q, seqs = E.noise_batch(name, K)
        pairs = [(0, k) for k, t in enumerate(seqs) if len(t)]
        want = _want_aligned(name, K, "noise", q, seqs, pairs, 0)
        gapped = sum(any(op & 15 in (A.OP_I, A.OP_D) for op in w[1]) for w in want)
        tied = TG._cached(("env-tied", name, K), lambda: sum(
            E.best_cells(q, t, sub, case.go, case.ge, 0) > 1 for t in seqs))
        print(name, K, "gapped", gapped, "tied", tied)
        assert gapped >= 10 and tied >= 10


# ---- 3. pad rows and pad columns beside a hit ---------------------------------------------------------
@pytest.mark.parametrize("m", E.EDGE_QLENS)
@pytest.mark.parametrize("go,ge", [(0, 0), (-8, 0)])
@pytest.mark.parametrize("mat", ["pad-prot", "wide-prot"])
def test_pad_rows_and_pad_columns(mat, go, ge, m, poisoned_buffers):
    """Queries of 255, 256, 257, 1,023 and 1,024 rows against windows of their last rows at the
    very end of a strand, L mod 3 in {0, 1, 2}: the rows past the query and the frames of the last
    codon index past the strand read the pad score -128, which under pad-prot is also a matrix
    entry (the whole X column), and with a free gap a pad cell equals the real cell it extends.
    Scores, strands, records and ops at every frameshift value."""
    case = E.BY_NAME[f"{mat}{go}/{ge}"]
    sub = E.matrix(mat)
    q, seqs = E.edge_batch(m)
    assert {len(t) % 3 for t in seqs} == {0, 1, 2}
    pairs = [(0, k) for k in range(len(seqs))]
    bt = TG.Batch(seqs)
    with _bank(case) as bank:
        bank.load_query(q)
        for fs in E.FS_VALUES:
            want = TG._cached(("env-edge-scores", mat, go, m, fs),
                              lambda: FS.c_search(q, seqs, sub, go, ge, fs))
            scores = _score_both_forms(bank, bt, seqs, fs, want, (mat, go, m, fs))
            if fs in _align_fs(case):
                recs = TG._cached(("env-edge-aligned", mat, go, m, fs),
                                  lambda: TA._want([q], seqs, pairs, sub, (go, ge), fs))
                _align_device(bank, bt, seqs, pairs, fs, recs, scores, f"{mat} {go} {m} {fs}")
    # the hits do end at the matrix's far corner (the query's last row, the strand's last codon),
    # right beside the pad cells; with free gaps a best value reached earlier runs on into every
    # later cell instead, the pad cells among them, and the tie rule alone keeps the end on a real
    # cell: one or the other holds for the batch
    recs = TG._cached(("env-edge-aligned", mat, go, m, -32767), None)
    at_edge = sum(w[0][3] == m - 1 and
                  (w[0][4] <= 2 if w[0][1] & S.ALIGN_REVERSE else w[0][5] >= len(t) - 3)
                  for w, t in zip(recs, seqs))
    tied = TG._cached(("env-edge-tied", mat, go, m), lambda: sum(
        E.best_cells(q, t, sub, go, ge, -32767) > 1 for t in seqs))
    print(mat, go, m, "hits at the far corner", at_edge, "tied", tied)
    assert at_edge >= 6 or (go == 0 and tied >= 10)


# ---- 4. seeded fuzz ----------------------------------------------------------------------------------
#  SWBANK_FSFUZZ_SEEDS=n (default 48) / SWBANK_FSFUZZ_BASE=b: seeds b .. b+n-1, eight to a test
_BASE = int(os.environ.get("SWBANK_FSFUZZ_BASE", "0"))
_SEEDS = int(os.environ.get("SWBANK_FSFUZZ_SEEDS", "48"))


@pytest.mark.parametrize("first", range(_BASE, _BASE + _SEEDS, 8))
def test_fuzz_against_the_models(first, poisoned_buffers):
    for seed in range(first, min(first + 8, _BASE + _SEEDS)):
        sub, go, ge, fs, table, q, seqs = E.fuzz_case(seed)
        want = FS.c_search(q, seqs, sub, go, ge, fs, table)
        bt = TG.Batch(seqs) if sum(len(t) for t in seqs) else None
        with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=O.GAP_GOTOH) as bank:
            bank.set_matrix(sub, go, ge)
            bank.load_query(q)
            if bt is None:  # (nothing to upload: the host form alone)
                sc, sd = bank.score_frameshift(seqs, fs, codon_table=table)
                assert not sc.any() and not sd.any() and not want[0].any()
                continue
            scores = _score_both_forms(bank, bt, seqs, fs, want, (seed, go, ge, fs, len(q)), table)
            top = [int(k) for k in np.argsort(-want[0], kind="stable")[:4] if want[0][k] > 0]
            if top:
                pairs = [(0, k) for k in top]
                recs = TA._want([q], seqs, pairs, sub, (go, ge), fs, table)
                _align_device(bank, bt, seqs, pairs, fs, recs, scores, f"seed {seed}", table)


# ---- 5. the two refusals -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_range_refusals_write_nothing(which):
    """A matrix of span 255 and Gotoh penalties with o + e + S = 65536 are refused by every
    frameshift entry with SW_ERR_RANGE (the query tables every entry prepares are built for the
    16-bit kernels), after the opening checks and before anything is written; the bank stays
    usable."""
    torch = TG._torch()
    case = E.REFUSED[which]
    q, seqs = E.noise_batch(E.CASES[0].name, 4)
    seqs = seqs[:8]
    bt = TG.Batch(seqs)
    host = (bt.res, bt.offs, bt.lens)
    n, dev = bt.n, torch.device("cuda", 0)
    rec = S.ALIGNMENT_DTYPE.itemsize

    def status(fn, *a, **kw):
        with pytest.raises(S.SwbankError) as ei:
            fn(*a, **kw)
        return ei.value.status

    with _bank(case) as bank:  # (loading the matrix and the query is accepted)
        bank.load_query(q)
        d_sc = torch.full((n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        d_sd, d_out = TG._filled(n), TG._filled(n * rec)
        d_cig = torch.full((n * 64,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert status(bank.score_frameshift_device, *bt.ptrs(), n, bt.max_len, -15,
                      d_sc.data_ptr(), d_strands=d_sd.data_ptr()) == S.ERR_RANGE
        assert status(bank.align_frameshift_hits_device, *bt.ptrs(), n, bt.max_len, -15, n,
                      d_out.data_ptr(), hits_per_query=n, d_cigar=d_cig.data_ptr(),
                      cigar_stride=64) == S.ERR_RANGE
        assert status(bank.estimate_frameshift_statistics_device, *bt.ptrs(), n, bt.max_len,
                      -15) == S.ERR_RANGE
        assert status(bank.score_frameshift, host, -15) == S.ERR_RANGE
        assert status(bank.align_frameshift_hits, *host, -15, hits=np.arange(n, dtype=np.uint64),
                      hits_per_query=n) == S.ERR_RANGE
        assert status(bank.estimate_frameshift_statistics, host, -15) == S.ERR_RANGE
        # the opening checks come first
        assert status(bank.score_frameshift, host, 1) == S.ERR_ARG
        assert status(bank.align_frameshift_hits_device, *bt.ptrs(), n, bt.max_len, -32768, n,
                      d_out.data_ptr(), hits_per_query=n) == S.ERR_ARG
        # the host forms' outputs, through the C entries themselves
        L, P = S.lib(), FS._p
        sc, sd = np.full(n, 0x3C3C3C3C, np.int32), np.full(n, TG.FILL, np.uint8)
        assert L.sw_score_fshift(bank._h, P(bt.res), bt.res.size, P(bt.offs), P(bt.lens), n, None,
                                 -15, P(sc), P(sd)) == S.ERR_RANGE
        out = np.full(n * rec, TG.FILL, np.uint8)
        cig = np.full(n * 64, 0x3C3C3C3C, np.uint32)
        used = ctypes.c_size_t(77)
        hv = np.arange(n, dtype=np.uint64)
        assert L.sw_align_fshift_hits(bank._h, P(bt.res), bt.res.size, P(bt.offs), P(bt.lens), None,
                                      n, None, -15, None, n, P(hv), n, P(out), P(cig), cig.size,
                                      ctypes.byref(used)) == S.ERR_RANGE
        st = np.full(ctypes.sizeof(S.Statistics), TG.FILL, np.uint8)
        assert L.sw_estimate_fshift_statistics(bank._h, P(bt.res), bt.res.size, P(bt.offs),
                                               P(bt.lens), n, None, -15, 1, 1, P(st)) == S.ERR_RANGE
        bank.sync()
        torch.cuda.synchronize()
        assert (d_sc.cpu().numpy() == 0x3C3C3C3C).all() and (d_sd.cpu().numpy() == TG.FILL).all()
        assert (d_out.cpu().numpy() == TG.FILL).all() and (d_cig.cpu().numpy() == 0x3C3C3C3C).all()
        assert (sc == 0x3C3C3C3C).all() and (sd == TG.FILL).all() and (out == TG.FILL).all()
        assert (cig == 0x3C3C3C3C).all() and (st == TG.FILL).all()
        assert used.value == 0  # (cigar_used is cleared on entry, as the header says)
        assert np.array_equal(bt.d_res.cpu().numpy(), bt.res)
        # an accepted matrix and the bank scores again
        ok = E.CASES[0]
        bank.set_matrix(E.matrix(ok.matrix), ok.go, ok.ge)
        want = _want_scores(ok.name, 4, "noise", *E.noise_batch(ok.name, 4), -15)
        sc, sd = bank.score_frameshift(seqs, -15)
        TG._same(sc, want[0][:8], "scores after a refusal")
        TG._same(sd, want[1][:8], "strands after a refusal")


# ---- 6. statistics -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nopos0-prot-11/-1", "blosum620/0"])
def test_statistics_at_the_envelopes_ends(name):
    """estimate_frameshift_statistics over 64 targets of 300 nt, a 33-row query, 2 rounds, against
    the reference pipeline (stat_cases.shuffle -> the C model -> histogram -> fit): a matrix with
    no positive entry (every score 0, one occupied bin: whatever the reference's fit returns for
    it, SW_STAT_DEGENERATE and lambda = K = 0), and free gaps."""
    case = E.BY_NAME[name]
    q, res, offs, lens = E.stats_batch()
    lam, K, degenerate, ns, lo, hi, clamped = TG._cached(
        ("env-stats", name), lambda: E.stats_reference(E.matrix(case.matrix), case.go, case.ge,
                                                       -15, 3))
    assert degenerate == ("nopos" in case.tags) and ns == 2 * 64
    with _bank(case) as bank:
        bank.load_query(q)
        (host,) = bank.estimate_frameshift_statistics((res, offs, lens), -15, seed=3,
                                                      rounds=E.STATS_ROUNDS)
        bt = TG.Batch(packed=(res, offs, lens))
        (dev,) = bank.estimate_frameshift_statistics_device(*bt.ptrs(), bt.n, bt.max_len, -15,
                                                            seed=3, rounds=E.STATS_ROUNDS)
    assert bytes(host) == bytes(dev)
    st = host
    assert (st.n_samples, st.min_score, st.max_score, st.n_clamped, st.query_len) == \
        (ns, lo, hi, clamped, len(q))
    if degenerate:
        assert (lo, hi) == (0, 0)
        assert st.flags == S.STAT_DEGENERATE and (st.lambda_, st.K) == (lam, K) == (0.0, 0.0)
    else:
        assert st.flags == 0 and hi > lo
        assert abs(st.lambda_ - lam) <= 1e-9 * lam and abs(st.K - K) <= 1e-6 * K
