"""The models of the alignments of global-local hits (tests/glalign_cases.py) against each other,
against the search's model, against the local aligner's model and against their own mutants; no
GPU.  What the GPU tests (tests/test_gpu_glalign.py) compare the library with is the C model; this
module is what says the C model is the definition of include/swbank.h."""
import numpy as np
import pytest

from oracle import oracle as O

import align_cases as AL
import align_check as AC
import glalign_cases as A
import glocal_cases as G
import seam_cases as SEAMS
import strand_cases as SC

MATRICES = {"dna": G.dna, "asym": SEAMS.MATRICES[G.ASYM]}


def _tiny_pairs(seed, n):
    rng = np.random.default_rng(seed)
    for it in range(n):
        m, L = int(rng.integers(1, 10)), int(rng.integers(0, 12))
        q = rng.integers(0, 4, m).astype(np.uint8)
        t = rng.integers(0, 5 if it % 7 == 0 else 4, L).astype(np.uint8)
        if it % 3 == 0 and L > 3:      # a piece of the query, on either strand
            w = q[int(rng.integers(0, m)):][:L]
            t[:len(w)] = w
            t = SC.revcomp(t) if it % 2 else t
        yield q, t


@pytest.mark.parametrize("matrix", list(MATRICES))
@pytest.mark.parametrize("pen", list(G.ENVELOPE), ids=str)
def test_c_model_is_the_python_restatement(pen, matrix):
    """50 random tiny pairs (m <= 9, L <= 11) per penalty pair and matrix, in all three modes on
    one strand and on both -- 3,000 records in all: the C model equals the plain-Python
    restatement (brute-force start, documented preference) field for field and op for op, and
    every record passes the preference-free checks."""
    sub = MATRICES[matrix]()
    kinds = set()
    for q, t in _tiny_pairs([331, abs(pen[0]), abs(pen[1])], 50):
        for ends in G.MODES:
            for both in (False, True):
                want = A.py_align(q, t, sub, *pen, ends, both)
                got = A.c_align(q, t, sub, *pen, ends, both)
                assert got == want, (q, t, pen, ends, both, got, want)
                A.check_record(*got, q, t, sub, *pen, ends, both)
                if got[1]:
                    kinds.add((ends, got[1][0] & 15, got[1][-1] & 15))
    # the first and the last op need not be M (where a gap is cheap enough to occur at all)
    if pen[0] > -100:
        assert {(A.QUERY, A.OP_I, A.OP_M), (A.QUERY, A.OP_M, A.OP_I)} <= kinds


def test_records_at_the_reference_penalties():
    """5 / -4 at -12 / -4, 300 tiny pairs: the same comparison, and the share of end cells that
    are not M-sourced (a query tail against a gap) is what the definition says to expect."""
    sub, pen = G.dna(), G.DNA_PEN
    last, n = 0, 0
    for q, t in _tiny_pairs(337, 300):
        for ends in G.MODES:
            for both in (False, True):
                want = A.py_align(q, t, sub, *pen, ends, both)
                got = A.c_align(q, t, sub, *pen, ends, both)
                assert got == want, (q, t, ends, both, got, want)
                A.check_record(*got, q, t, sub, *pen, ends, both)
                if got[1]:
                    n += 1
                    last += (got[1][-1] & 15) != A.OP_M
    print(f"{last} of {n} paths end in a gap")
    assert last * 20 > n   # more than one in twenty


def test_query_mode_is_the_local_alignment_when_the_query_aligns_whole():
    """A query copied whole into N flanks with substitutions in its interior only: where the
    local reference (align_cases.ref_path over the brute-force coordinates) aligns the query end
    to end, the QUERY record is the local record field for field and op for op."""
    rng = np.random.default_rng(347)
    sub, (go, ge) = G.dna(), G.DNA_PEN
    kept = 0
    for k in range(24):
        m = int(rng.integers(30, 90))
        q = rng.integers(0, 4, m).astype(np.uint8)
        core = q.copy()
        at = rng.integers(8, m - 8, 3)
        core[at] = (core[at] + 1 + rng.integers(0, 3, 3)) % 4
        if k % 3 == 1:
            core = np.delete(core, m // 2)
        elif k % 3 == 2:
            core = np.insert(core, m // 2, rng.integers(0, 4, 2))
        t = np.concatenate([np.full(int(rng.integers(1, 9)), 4), core,
                            np.full(int(rng.integers(1, 9)), 4)]).astype(np.uint8)
        score, qs, qe, ts, te = AC.brute_ends(O, q, t, sub, go, ge, AL.GAP_GOTOH)
        assert (qs, qe) == (0, m - 1), "the local alignment spans the query"
        ref = AL.ref_path(q, t, sub, go, ge, AL.GAP_GOTOH, (score, qs, qe, ts, te))
        rec, ops = A.c_align(q, t, sub, go, ge, A.QUERY)
        assert rec == (score, 0, qs, qe, ts, te, ref.n_columns, ref.n_identities), (k, rec)
        assert ops == tuple(ref.ops), (k, A.cigar(ops), A.cigar(ref.ops))
        kept += 1
    assert kept == 24


@pytest.mark.parametrize("matrix", list(MATRICES))
def test_target_mode_is_query_mode_transposed(matrix):
    """TARGET(q, t, S) scores what QUERY(t, q, S^T) scores, and its coordinates are those with q
    and t exchanged.  (The ops are not compared: D before I is not symmetric.)"""
    sub = MATRICES[matrix]()
    subT = np.ascontiguousarray(np.asarray(sub).T)
    for pen in G.ENVELOPE + (G.DNA_PEN,):
        for q, t in _tiny_pairs([349, abs(pen[0])], 40):
            if len(t) == 0:
                continue
            a, _ = A.c_align(q, t, sub, *pen, A.TARGET)
            b, _ = A.c_align(t, q, subT, *pen, A.QUERY)
            assert (a[0], a[1]) == (b[0], b[1]) and a[2:6] == (b[4], b[5], b[2], b[3]), \
                (q, t, pen, a, b)
            assert a[6] == b[6] or a[1] & A.EMPTY == 0


@pytest.mark.parametrize("K", G.ROWS)
def test_seam_plants_are_live_per_pass(K):
    """Per pass and rows-per-lane count, the C model's mutant that loses F at the plant's lane
    seam, or E at its block seam, in THAT pass's rows and columns changes the record or the ops
    of at least 3 of the family's 4 plants; the GPU test runs the live ones."""
    for family, plants in A.pass_plants(K).items():
        flags = A.live(plants, G.dna(), *G.DNA_PEN, A.ENDS_OF[family])
        print(K, family, flags)
        assert len(flags) == 4 and sum(flags) >= 3, (K, family, flags)
        for q, _, _ in plants:
            assert G.ROWS[(len(q) > 256) + (len(q) > 512)] == K


def test_asymmetric_matrix_moves_the_records():
    """glocal_cases.asym_case on both strands: the transposed matrix changes a majority of the
    model's records in every mode, so a kernel reading s(t, q) cannot pass."""
    q, seqs = G.asym_case()
    sub = SEAMS.MATRICES[G.ASYM]()
    subT = np.ascontiguousarray(np.asarray(sub).T)
    for ends in G.MODES:
        moved = sum(A.c_align(q, t, sub, *G.ASYM_PEN, ends, True) !=
                    A.c_align(q, t, subT, *G.ASYM_PEN, ends, True) for t in seqs)
        assert 2 * moved > len(seqs), (ends, moved)
        for t in seqs[:12]:
            A.check_record(*A.c_align(q, t, sub, *G.ASYM_PEN, ends, True), q, t, sub,
                           *G.ASYM_PEN, ends, True)


@pytest.mark.parametrize("pen", [(0, 0), (0, -3)], ids=str)
def test_tie_pairs_are_rich_in_ties(pen):
    """The low-complexity pairs at (0, 0) and (0, -3): path cells with a co-optimal diagonal/gap,
    left/up and open/extend alternative all occur, and the C model still equals the Python
    restatement on the smaller ones."""
    sub = G.dna()
    for ends in G.MODES:
        total = np.zeros(3, np.int64)
        for k, (q, t) in enumerate(A.tie_pairs()):
            rec, ops, ties = A.c_align(q, t, sub, *pen, ends, True, ties=True)
            total += ties
            A.check_record(rec, ops, q, t, sub, *pen, ends, True)
            if k < 4:
                assert (rec, ops) == A.py_align(q, t, sub, *pen, ends, True)
        print(pen, ends, total)
        assert (total > 0).all(), (pen, ends, total)
