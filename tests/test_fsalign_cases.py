"""The model of the alignments of frameshift hits (tests/fsalign_cases.py, tests/c/fsalign_model.c)
against the contract of include/swbank.h "alignments of frameshift hits": the C model against the
plain-Python restatement with its brute-force start, the six-frame anchor at fs = -32767, the
planted shifts, the op texts, the edges.  No GPU."""
import collections
import os

import numpy as np

import swbank as S
from oracle import oracle as O

import align_cases as ALC
import align_check as AC
import frame_cases as F
import fsalign_cases as A
import fshift_cases as FS
import strand_cases as SC

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "swbank.h")


def test_c_model_equals_the_python_restatement():
    """264 tiny pairs (m <= 7, L <= 25, 2- and 4-letter DNA, queries read off the target with
    steps of 2, 3 and 4 bases, planted one- and two-codon gaps; fs in {0, -1, -4, -15}; penalties
    (-11,-1), (-2,-1), (-1,0), (-4,-4)): the C model (reversed pass, direction bytes) equals the
    Python restatement (brute-force start, walk over values) in every field and op, every CIGAR
    re-scores to its score and spans its window, the score is the search's, and every op kind
    occurs at least 10 times."""
    cases = A.tiny_cases()
    assert len(cases) >= 150
    kinds = collections.Counter()
    for q, t, go, ge, fs in cases:
        assert len(q) <= 7 and len(t) <= 25
        got = A.c_align(q, t, O.BLOSUM62, go, ge, fs)
        assert got == A.py_align(q, t, O.BLOSUM62, go, ge, fs), (q, t, go, ge, fs)
        A.check_record(*got, q, t, O.BLOSUM62, go, ge, fs)
        score, strand = FS.py_search(q, t, O.BLOSUM62, go, ge, fs)
        assert got[0][0] == score and bool(got[0][1] & F.ALIGN_REVERSE) == bool(strand and score)
        kinds.update(A.OP_TEXT[op & 15] for op in got[1])
    print(dict(kinds))
    assert all(kinds[c] >= 10 for c in A.OP_TEXT), kinds


def anchor_pairs(cap=80):
    """(qs, seqs, [(i, k, f, per-frame scores)]) of frame_cases.search_case(): the 50 pairs
    scoring at least half the query's self score, then the other positive pairs in (query,
    target) order up to `cap` pairs in all; f the strictly best frame, None for a tied pair."""
    qs, seqs, _ = F.search_case()
    per = np.stack([F.oracle_frames(q, seqs) for q in qs])  # [nq, 6, n]
    best = per.max(axis=1)
    strong = [(i, k) for i in range(len(qs)) for k in range(len(seqs))
              if 2 * best[i, k] >= F.self_score(qs[i])]
    rest = [(i, k) for i in range(len(qs)) for k in range(len(seqs))
            if best[i, k] > 0 and (i, k) not in set(strong)]
    assert len(strong) == 50 and len(strong) + len(rest) == 591
    pairs = []
    for i, k in (strong + rest)[:cap]:
        top = np.nonzero(per[i, :, k] == best[i, k])[0]
        pairs.append((i, k, int(top[0]) if len(top) == 1 else None, per[i, :, k]))
    return qs, seqs, pairs


def frame_reference(q, t, f):
    """What sw_align_frame_hits returns for frame f: (record, ops) by brute force and ref_path."""
    prot = F.translate(t, f)
    ends = AC.brute_ends(O, q, prot, O.BLOSUM62, *F.PEN, O.GAP_GOTOH)
    ref = ALC.ref_path(q, prot, O.BLOSUM62, *F.PEN, O.GAP_GOTOH, ends)
    ts, te = F.nt_coords(ends[3], ends[4], f, len(t))
    return (ends[0], F.frame_flags(f), ends[1], ends[2], ts, te, ref.n_columns, ref.n_identities), \
        tuple(ref.ops)


def test_anchor_equals_the_frame_alignment_of_the_strictly_best_frame():
    """At fs = -32767 a pair with a strictly best frame has the record sw_align_frame_hits
    specifies for that frame (brute-force ends, align_cases.ref_path on the translation), field
    for field and op for op.  80 of the 591 positive pairs of search_case() (seed 71): the 50
    strong pairs, then the next 30 positive pairs in (query, target) order; the 2 tied pairs are
    skipped, none of the 50 strong pairs is: 78 pairs."""
    qs, seqs, pairs = anchor_pairs()
    untied = [p for p in pairs if p[2] is not None]
    print(f"{len(untied)} untied of {len(pairs)}")
    assert all(f is not None for _, _, f, _ in pairs[:50]) and len(untied) == 78
    for i, k, f, _ in untied:
        got = A.c_align(qs[i], seqs[k], O.BLOSUM62, *F.PEN, -32767)
        assert got == frame_reference(qs[i], seqs[k], f), (i, k, f)


def test_planted_shifts_read_one_shift_op():
    """fshift_cases.shift_cases() at fs = -15: the hit lies on the planted strand, spans query
    rows 0..39 and holds exactly one shift op: 20M1/20M for an inserted base, aM1\\bM with
    a + b = 40 and a in {19, 20, 21} for a deleted one."""
    cases = FS.shift_cases()
    assert len(cases) == 40
    for kind, rev, q, t, _, _ in cases:
        rec, ops = A.c_align(q, t, O.BLOSUM62, *F.PEN, FS.SHIFT_FS)
        A.check_record(rec, ops, q, t, O.BLOSUM62, *F.PEN, FS.SHIFT_FS)
        assert bool(rec[1] & F.ALIGN_REVERSE) == rev and rec[2:4] == (0, 39)
        assert sum(op & 15 >= A.OP_SKIP for op in ops) == 1 and len(ops) == 3
        text = S.cigar_string(ops)
        if kind == "ins":
            assert text == "20M1/20M"
        else:
            a, b = ops[0] >> 4, ops[2] >> 4
            assert text == f"{a}M1\\{b}M" and a + b == 40 and a in (19, 20, 21)


def test_cigar_string_prints_the_shift_ops():
    """Codes 3 and 4 print '/' and '\\', every other code past D still '?'; the header carries the
    new macro and the op codes, and the ABI version stays 6."""
    assert (S.CIGAR_FS_SKIP, S.CIGAR_FS_BACK) == (3, 4) == (A.OP_SKIP, A.OP_BACK)
    assert S.cigar_string([20 << 4, 1 << 4 | 3, 20 << 4]) == "20M1/20M"
    assert S.cigar_string([19 << 4, 1 << 4 | 4, 21 << 4 | 0, 2 << 4 | 2]) == "19M1\\21M2D"
    assert S.cigar_string([3 << 4 | 9]) == "3?"
    for code in range(5, 16):
        assert S.cigar_string([1 << 4 | code]) == "1?"
    text = open(HEADER).read()
    assert "#define SWBANK_HAS_FSHIFT_ALIGN 1" in text
    assert "SW_CIGAR_FS_SKIP = 3, SW_CIGAR_FS_BACK = 4" in text
    assert "#define SWBANK_ABI_VERSION 6\n" in text and S.ABI_VERSION == 6
    assert hasattr(S.ScoreBank, "align_frameshift_hits")
    assert hasattr(S.ScoreBank, "align_frameshift_hits_device")


def test_edges():
    """A self-complementary target gives the forward strand; L < 3 and a pair scoring 0 are the
    empty record."""
    rng = np.random.default_rng(3)
    q = rng.integers(0, 20, 12).astype(np.uint8)
    half = F.back_translate(rng, q)
    t = np.concatenate([half, SC.revcomp(half)])
    assert np.array_equal(SC.revcomp(t), t)
    for model in (A.c_align, A.py_align):
        rec, ops = model(q, t, O.BLOSUM62, *F.PEN, -15)
        assert rec[0] == F.self_score(q) and not rec[1] & F.ALIGN_REVERSE
        assert rec[4:6] == (0, 35) and S.cigar_string(ops) == "12M"
        for L in range(3):
            assert model(q, t[:L], O.BLOSUM62, *F.PEN, -15) == A.EMPTY
        d = np.array([O.PROT_LETTERS.index("D")], np.uint8)  # D scores below 0 with F and with K
        assert model(d, np.zeros(9, np.uint8), O.BLOSUM62, *F.PEN, 0) == A.EMPTY


def test_seam_family_is_live():
    """The targets of the GPU seam tests: for K = 4, 8, 16 and each of passes A, B and C an I run
    across the lane seam 5K - 1 | 5K and a D run across the codon indices 63 | 64, in that pass's
    own numbering, in windows whose first row is no multiple of K.  A target is kept only if the C
    model that drops the gap state there, in that pass, returns another record: 34 of 36."""
    total = 0
    for K in (4, 8, 16):
        q, kept, tried = A.seam_family(K, O.BLOSUM62, F.PEN)
        assert tried == 12 and {(p, k) for _, p, k, _, _ in kept} == \
            {(p, k) for p in "ABC" for k in "ID"}
        for t, pas, kind, mrow, mcol in kept:
            rec, ops = A.c_align(q, t, O.BLOSUM62, *F.PEN, -15)
            A.check_record(rec, ops, q, t, O.BLOSUM62, *F.PEN, -15)
            assert rec[2] % K and S.cigar_string(ops).count("2" + kind) == 1
        total += len(kept)
    print(total, "of 36 kept")
    assert total >= 30
