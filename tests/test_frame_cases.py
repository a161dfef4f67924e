"""The translated-search model (tests/frame_cases.py) against the definitions of include/swbank.h
"translated search", the oracle over six frames on planted proteins, and the library's host
translation against the model.  No GPU."""
import itertools

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import matrix_cases as MC
import seam_cases as SEAMS
import strand_cases as SC


def test_atg_gcc_taa_is_ma_stop():
    got = F.translate(O.encode_dna("ATGGCCTAANN"), 0)
    assert "".join(O.PROT_LETTERS[c] for c in got) == "MA*"
    assert got[2] == F.STOP == 23


def test_all_64_codons_give_the_standard_table():
    codons = np.array(list(itertools.product(range(4), repeat=3)), np.uint8).reshape(-1)
    got = F.translate(codons, 0)
    assert "".join(O.PROT_LETTERS[c] for c in got) == F.STANDARD_CODE == S.STANDARD_CODE
    assert np.array_equal(got, F.standard_table())


def test_any_n_gives_x():
    for pos in range(3):
        for base in itertools.product(range(4), repeat=3):
            c = np.array(base, np.uint8)
            c[pos] = 4
            assert F.translate(c, 0).tolist() == [F.X] == [22]
    assert F.translate(np.array([0, 0, 9], np.uint8), 0).tolist() == [F.X]  # and anything past N


def test_short_targets_have_empty_frames():
    for L in range(0, 9):
        t = np.arange(L, dtype=np.uint8) % 4
        for f in range(6):
            want = (L - f % 3) // 3 if L >= f % 3 + 3 else 0
            assert len(F.translate(t, f)) == want == F.frame_len(L, f)
            if L < f % 3 + 3:
                assert want == 0


def test_reverse_frames_are_forward_frames_of_the_reverse_complement():
    rng = np.random.default_rng(5)
    for L in (0, 1, 2, 3, 4, 5, 6, 7, 100, 101, 102):
        t = rng.integers(0, 5, L).astype(np.uint8)
        for f in range(3):
            assert np.array_equal(F.translate(t, 3 + f), F.translate(SC.revcomp(t), f))


def test_custom_table_is_honoured():
    tab = F.custom_table()
    assert (tab != F.standard_table()).all() and tab.max() < O.PROT_ALPHA
    t = np.random.default_rng(6).integers(0, 4, 300).astype(np.uint8)
    for f in range(6):
        std, cus = F.translate(t, f), F.translate(t, f, tab)
        assert np.array_equal(cus, (std.astype(np.int64) + 1) % O.PROT_ALPHA)
    assert F.translate(np.array([4, 0, 0], np.uint8), 0, tab).tolist() == [F.X]  # N is X in any code


def test_merge6_ties_go_to_the_lowest_frame():
    s = np.array([[0, 3, 5, 1], [0, 7, 5, 1], [0, 7, 2, 1], [0, 1, 5, 9], [0, 0, 0, 9], [0, 7, 0, 0]])
    sc, fr = F.merge6(s)
    assert sc.tolist() == [0, 7, 5, 9] and fr.tolist() == [0, 1, 0, 3]


def test_nt_coords_ranges():
    for L in range(3, 40):
        for f in range(6):
            n = F.frame_len(L, f)
            for a in range(n):
                for e in range(a, n):
                    ts, te = F.nt_coords(a, e, f, L)
                    assert 0 <= ts <= te < L and te - ts + 1 == 3 * (e - a + 1)
    # the range holds the codons: reading it on its strand gives the aligned amino acids
    rng = np.random.default_rng(7)
    t = rng.integers(0, 4, 61).astype(np.uint8)
    for f in range(6):
        ts, te = F.nt_coords(2, 9, f, len(t))
        piece = t[ts:te + 1]
        assert np.array_equal(F.translate(piece, 0 if f < 3 else 3), F.translate(t, f)[2:10])


def test_frame_flags_round_trip():
    for f in range(6):
        assert F.frame_of(F.frame_flags(f)) == f
        assert F.frame_of(F.frame_flags(f) | F.ALIGN_NO_PATH) == f
        a = S.Alignment(0, 0, 5, F.frame_flags(f), 0, 0, 0, 0, 0, 0)
        assert a.frame == f and a.reverse == (f >= 3) and a.has_path
    assert (S.ALIGN_FRAME_SHIFT, S.ALIGN_FRAME_MASK) == (F.ALIGN_FRAME_SHIFT, F.ALIGN_FRAME_MASK)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("o", [0, 1, 2])
def test_oracle_finds_the_planted_frame_with_the_self_score(o, reverse):
    """A 40-aa query, back-translated and planted at offset residue o on either strand of random
    200-nt targets: the oracle over six frames finds the planted frame with the self-score."""
    rng = np.random.default_rng([11, o, int(reverse)])
    q = rng.integers(0, 20, 40).astype(np.uint8)
    made = [F.plant(rng, q, 200, o, reverse) for _ in range(6)]
    seqs = [t for t, _ in made]
    assert {f for _, f in made} == {o + (3 if reverse else 0)}
    sc, fr = F.merge6(F.oracle_frames(q, seqs))
    assert sc.tolist() == [F.self_score(q)] * 6
    assert fr.tolist() == [f for _, f in made]


def test_search_case_has_every_planted_frame():
    qs, seqs, planted = F.search_case()
    assert set(planted.values()) == set(itertools.product(range(3), range(6)))
    sc, fr, _ = F.want_frames(qs, seqs)
    for k, (i, f) in planted.items():  # every query in every frame, found with its self-score
        assert (sc[i][k], fr[i][k]) == (F.self_score(qs[i]), f)
    assert {len(seqs[k]) for k in (0, 2, 3, 6)} == {0, 1, 2, 4}
    assert any((s == 4).any() for s in seqs) and max(len(s) for s in seqs) <= 400


# ---- the library's host translation (no device) -----------------------------------------------------
@pytest.mark.parametrize("table", [None, "custom"])
def test_translate_codes_matches_the_model(table):
    tab = F.custom_table() if table else None
    rng = np.random.default_rng(13)
    for L in list(range(0, 12)) + [191, 192, 193, 1021]:
        t = rng.integers(0, 5, L).astype(np.uint8)
        for f in range(6):
            assert np.array_equal(S.translate_codes(t, f, tab), F.translate(t, f, tab)), (L, f)
    assert np.array_equal(S.translate_codes(O.encode_dna("ATGGCCTAANN"), 0),
                          O.encode_protein("MA*"))
    if tab is not None:  # the table as letters
        letters = "".join(O.PROT_LETTERS[c] for c in tab)
        assert np.array_equal(S.translate_codes(t, 4, letters), F.translate(t, 4, tab))


def test_translate_codes_refuses_bad_arguments():
    t = np.zeros(9, np.uint8)
    bad = F.standard_table()
    bad[17] = 24
    with pytest.raises(ValueError):
        S.translate_codes(t, 6)
    with pytest.raises(ValueError):
        S.translate_codes(t, 0, bad)
    out = np.zeros(3, np.uint8)
    L = S.lib()
    assert L.sw_translate_codes(S._p(t), 9, 6, None, S._p(out)) == 0
    assert L.sw_translate_codes(S._p(t), 9, 0, S._p(bad), S._p(out)) == 0
    assert L.sw_translate_codes(None, 9, 0, None, S._p(out)) == 0
    assert L.sw_translate_codes(S._p(t), 9, 0, None, S._p(out)) == 3


# ---- the asymmetric protein matrix through the frames ---------------------------------------------
@pytest.mark.parametrize("model", [O.GAP_MERGED, O.GAP_GOTOH])
@pytest.mark.parametrize("table", ["standard", "stop-x"])
def test_asymmetric_matrix_frames(table, model):
    """tests/matrix_cases.frame_case: every planted target scores best in its planted frame, and
    the transposed matrix changes the frame score of >= 80 % of them (measured: 27 of 27
    standard, 25 and 27 of 27 with the custom table); the custom table puts X and * in the
    queries and the translations, so rows and columns 22 / 23 are read."""
    tab = MC.stop_x_table() if table == "stop-x" else None
    qs, seqs, planted = MC.frame_case(tab)
    sub = SEAMS.MATRICES[MC.PROTEIN]()
    assert max(len(t) for t in seqs) <= MC.FRAME_MAX and len(planted) >= 24
    sc, fr = MC.frame_oracle(tab, model)
    sc2, _ = MC.frame_oracle(tab, model, np.ascontiguousarray(sub.T))
    changed = 0
    for k, (i, f) in planted.items():
        assert int(fr[i][k]) == f, (k, i, f)
        changed += int(sc[i][k]) != int(sc2[i][k])
    print(f"\n    frames {table} model {model}: {changed} of {len(planted)}", end="")
    assert changed >= 0.8 * len(planted)
    if tab is not None:
        assert sorted(np.nonzero(tab != F.standard_table())[0]) == [19, 34, 63]
        assert int((tab == F.STOP).sum()) == 5 and int((tab == F.X).sum()) == 1
        assert all((q == F.X).any() and (q == F.STOP).any() for q in qs)
        tr = np.concatenate([F.translate(seqs[k], f, tab) for k, (_, f) in planted.items()])
        assert (tr == F.X).any() and (tr == F.STOP).any()
