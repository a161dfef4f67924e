"""The inputs and references of the frameshift envelope (tests/fshift_envelope_cases.py, what
tests/test_gpu_fshift_envelope.py compares the kernels with): the two restatements of the
definition agree under every matrix and penalty pair of the table, the seam plants are live by the
C model's own mutant, a kernel reading s(a, q) could not pass, the no-positive matrices score
nothing, the limit case is the gap-free model.  No GPU."""
import collections

import numpy as np

import frame_cases as F
import fsalign_cases as A
import fshift_cases as FS
import fshift_envelope_cases as E


def test_the_table_holds_what_it_says():
    names = {c.name for c in E.CASES}
    assert len(names) == len(E.CASES)
    for go, ge in E.PAIRS:
        assert f"blosum62{go}/{ge}" in names
    for go, ge in ((0, 0), (-8, 0), (-100, -10)):
        assert f"asym-prot{go}/{ge}" in names
    m0, m1 = E.matrix("nopos0-prot"), E.matrix("nopos1-prot")
    assert m0.max() == 0 and (m0 == 0).sum() >= 24 and m1.max() == -1
    wide, pad, s255 = E.matrix("wide-prot"), E.matrix("pad-prot"), E.matrix("span255-prot")
    assert set(np.unique(wide).tolist()) == {-127, 127}
    assert (pad.min(), pad.max()) == (-128, 12) and (pad[:, F.X] == -128).all()
    assert (s255.min(), s255.max()) == (-128, 127)
    (limit,) = [c for c in E.CASES if "limit" in c.tags]
    S = int(E.matrix(limit.matrix).max())
    assert -limit.go - limit.ge + S == 65535
    span, gotoh = E.REFUSED
    assert -gotoh.go - gotoh.ge + int(E.matrix(gotoh.matrix).max()) == 65536
    assert int(E.matrix(span.matrix).max()) - int(E.matrix(span.matrix).min()) == 255
    for K in E.ROWS:
        q, seqs = E.noise_batch(E.CASES[0].name, K)
        assert len(q) == E.NOISE_QLEN[K] and len(seqs) == 64
        assert len(seqs[3]) == 0 and len(seqs[11]) == 2 and any((t == 4).any() for t in seqs)


def test_c_models_equal_the_python_restatements_under_every_case():
    """24 tiny pairs (m <= 7, L <= 25) per case of the table, 17 cases: both C models against the
    plain-Python restatements of the definition (fshift_cases.py_search; fsalign_cases.py_align
    with its brute-force start) in score, strand, every record field and op; every CIGAR
    re-scores to its score.  Under pad-prot the pairs read -128 entries in the X column and in
    rows of real residues; the go = 0 cases produce I and D ops (the tie rules are the Python
    walk's, over values, against the C model's direction bits)."""
    kinds = collections.Counter()
    pad_x = pad_real = 0
    for case in E.CASES:
        sub = E.matrix(case.matrix)
        for q, t, fs in E.tiny_pairs(case):
            assert len(q) <= 7 and len(t) <= 25
            what = (case.name, q.tolist(), t.tolist(), fs)
            score, strand = FS.py_search(q, t, sub, case.go, case.ge, fs)
            csc, csd = FS.c_search(q, [t], sub, case.go, case.ge, fs)
            assert (int(csc[0]), int(csd[0])) == (score, strand), what
            got = A.c_align(q, t, sub, case.go, case.ge, fs)
            assert got == A.py_align(q, t, sub, case.go, case.ge, fs), what
            A.check_record(*got, q, t, sub, case.go, case.ge, fs)
            assert got[0][0] == score
            assert bool(got[0][1] & F.ALIGN_REVERSE) == bool(strand and score)
            if case.go == 0:
                kinds.update(A.OP_TEXT[op & 15] for op in got[1])
            if case.matrix == "pad-prot" and len(t) >= 3:
                a = A.aminos(t) + A.aminos(E.SC.revcomp(t))
                cells = sub[np.asarray(q, np.intp)][:, np.asarray(a, np.intp)]
                pad_x += int((np.asarray(a) == F.X).any())
                pad_real += int((cells[:, np.asarray(a) != F.X] == -128).any())
    print(dict(kinds), pad_x, pad_real)
    assert kinds["I"] >= 10 and kinds["D"] >= 10, kinds
    assert pad_x >= 24 and pad_real >= 12


def test_seam_plants_are_live():
    """The gap-state seam families of the score walk, over the 8 cases with go < 0 that have one
    (fshift_envelope_cases.SEAM_CASES): at least 3 of every 4 plants tried are live (the C model
    that drops F into the row after a lane seam, or E into the codon index after a block seam,
    scores differently), at K = 16 every (kind, strand) cell of every case holds a live plant,
    and every plant kept lies on the strand it was planted on.

    Measured: 178 live of 200 tried, every plant on its strand.  Per case over K = 4 / 8 / 16 (live
    of tried): blosum62 -8/0 7/10 10/10 10/10; -1/-30 10/10 7/10 10/10; -100/-10 6/6 8/10 10/10;
    -300/-40 2/2 5/6 10/10; -1000/-1 0/2 2/2 6/6; asym-prot -8/0 8/10 7/10 10/10; -100/-10 6/6
    10/10 7/10; pad-prot -8/0 7/10 10/10 10/10.  The dead ones are the K = 4 plants at -1000 / -1
    (a 256-row query cannot pay the gap twice) and plants whose run slides off its seam."""
    live = E.liveness()
    tried = sum(v[0] for v in live.values())
    alive = sum(v[1] for v in live.values())
    print({k: v[:2] for k, v in live.items()}, alive, tried)
    assert len(E.SEAM_CASES) >= 8 and 4 * alive >= 3 * tried, (alive, tried)
    for case in E.SEAM_CASES:
        assert live[case.name, 16][2] == {(k, r) for k in "ID" for r in (False, True)}, case.name
        for K in E.ROWS:
            q, plants, _ = E.seam_family(case.name, K)
            assert len(q) == E.SEAM_QLEN[K]
            for p in plants:  # (the family checks the strand by the aligner: here by the score)
                sc, sd = FS.c_search(q, [p.target], E.matrix(case.matrix), case.go, case.ge,
                                     E.live_fs(case))
                assert sc[0] > 0 and bool(sd[0]) == p.reverse, (case.name, K, p.kind, p.seam)
    # the seams are the kernels': F into row K * l, E into codon index 64 * j
    for case in E.SEAM_CASES:
        for K in E.ROWS:
            for p in E.seam_family(case.name, K)[1]:
                assert (p.mrow % K == 0 and p.mcol == -1) if p.kind == "I" else \
                    (p.mcol % 64 == 0 and p.mrow == -1)


def test_a_mutant_off_the_seam_or_a_transposed_matrix_is_told_apart():
    """What the GPU comparisons rest on, shown once with the models alone: on the live plants the
    mutant at the seam scores differently (so a kernel losing F or E there fails), and the
    transposed pad-prot changes at least half of the scores of every noise batch (so a kernel
    reading s(a, q) fails)."""
    case = E.BY_NAME["blosum62-100/-10"]
    sub = E.matrix(case.matrix)
    q, plants, _ = E.seam_family(case.name, 16)
    for p in plants:
        if p.live:
            want = A.c_align(q, p.target, sub, *E.pen(case), E.live_fs(case), ops_cap=0)[0][0]
            mut = A.c_mutant(q, p.target, sub, *E.pen(case), E.live_fs(case), "A", p.mrow, p.mcol)
            assert mut[0][0] != want
    for name in ("pad-prot0/0", "pad-prot-8/0"):
        case = E.BY_NAME[name]
        sub = E.matrix(case.matrix)
        for K in E.ROWS:
            q, seqs = E.noise_batch(name, K)
            want = FS.c_search(q, seqs, sub, *E.pen(case), -15)[0]
            wrong = FS.c_search(q, seqs, np.ascontiguousarray(sub.T), *E.pen(case), -15)[0]
            print(name, K, int((want != wrong).sum()))
            assert 2 * int((want != wrong).sum()) >= len(seqs), (name, K)


def test_no_positive_entry_scores_nothing():
    for name in ("nopos0-prot-11/-1", "nopos1-prot-11/-1"):
        case = E.BY_NAME[name]
        sub = E.matrix(case.matrix)
        for K in E.ROWS:
            q, seqs = E.noise_batch(name, K)
            for fs in E.FS_VALUES:
                sc, sd = FS.c_search(q, seqs, sub, *E.pen(case), fs)
                assert not sc.any() and not sd.any()
            assert all(A.c_align(q, t, sub, *E.pen(case), 0) == A.EMPTY for t in seqs)


def test_the_limit_case_is_the_gap_free_model():
    (case,) = [c for c in E.CASES if "limit" in c.tags]
    sub = E.matrix(case.matrix)
    for K in E.ROWS:
        q, seqs = E.noise_batch(case.name, K)
        for fs in E.FS_VALUES:
            want = FS.c_search(q, seqs, sub, *E.pen(case), fs)
            free = FS.c_search(q, seqs, sub, -32767, -32767, fs)
            assert np.array_equal(want[0], free[0]) and np.array_equal(want[1], free[1])
            assert (want[0] > 0).sum() >= 32


def test_tie_cases_are_not_vacuous():
    """The go = 0 cases: in every noise batch at least 10 targets have an I or a D op in the
    model's CIGAR at fs = 0, and at least 10 reach their best value at more than one cell."""
    for case in E.TIE_CASES:
        sub = E.matrix(case.matrix)
        for K in E.ROWS:
            q, seqs = E.noise_batch(case.name, K)
            gapped = sum(any(op & 15 in (A.OP_I, A.OP_D) for op in
                             A.c_align(q, t, sub, *E.pen(case), 0)[1]) for t in seqs)
            tied = sum(E.best_cells(q, t, sub, *E.pen(case), 0) > 1 for t in seqs)
            print(case.name, K, gapped, tied)
            assert gapped >= 10 and tied >= 10, (case.name, K, gapped, tied)
