"""The both-strand definitions on the CPU (no GPU): the host helper against the numpy model, the
facts of the reference's data500 library under the unchanged oracle, the equivalence of the
bank's definition (query against rc(target)) with ssearch36's (rc(query) against target), and
the two fixtures the GPU tests compare with (tests/golden/make_strands.py)."""
import os

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_cases as C
import align_check as AC
import matrix_cases as MC
import strand_cases as SC
from test_align_cases import check_mutant

SUB = O.dna_matrix(SC.REF[0], SC.REF[1])
MODELS = [O.GAP_MERGED, O.GAP_GOTOH]


@pytest.fixture(scope="module")
def data500():
    names, q, seqs = SC.data500()
    return names, q, seqs, {m: SC.oracle_strands(q, seqs, model=m) for m in MODELS}


def test_header_symbols():
    assert S.ALIGN_REVERSE == SC.ALIGN_REVERSE == 8
    hdr = open(os.path.join(O.REPO, "include", "swbank.h")).read()
    assert "#define SWBANK_HAS_STRANDS 1" in hdr and "SW_ALIGN_REVERSE = 8" in hdr
    assert "#define SWBANK_ABI_VERSION 6" in hdr


def test_revcomp_is_an_involution_and_matches_the_library():
    rng = np.random.default_rng(5)
    assert S.revcomp([]).size == 0
    assert S.revcomp([0, 1, 2, 3, 4]).tolist() == [4, 1, 0, 3, 2]  # TCAGN -> NCTGA
    assert S.revcomp(S.encode("AACGTN")).tolist() == S.encode("NACGTT").tolist()
    for n in (1, 2, 3, 4, 5, 64, 127, 1021):
        t = rng.integers(0, 5, n).astype(np.uint8)
        assert (S.revcomp(t) == SC.revcomp(t)).all()
        assert (SC.revcomp(SC.revcomp(t)) == t).all()
        assert (S.revcomp(S.revcomp(t)) == t).all()
    # codes past N stay, and the helper works in place
    t = np.array([7, 0, 255, 3, 4, 1], np.uint8)
    assert S.revcomp(t).tolist() == [3, 4, 1, 255, 2, 7]
    buf = rng.integers(0, 5, 9).astype(np.uint8)
    want = SC.revcomp(buf)
    S.lib().sw_revcomp_codes(S._p(buf), buf.size, S._p(buf))
    assert (buf == want).all()


def test_merge_ties_are_forward():
    sc, st = SC.merge([3, 5, 7, 0], [3, 6, 2, 0])
    assert sc.tolist() == [3, 6, 7, 0] and st.tolist() == [0, 1, 0, 0]


@pytest.mark.parametrize("model", MODELS)
def test_data500_facts(data500, model):
    """The table of the issue: the search documented as matching ssearch36 misses the two best
    hits of its own fixture.  The figures are the same under both gap models."""
    names, q, seqs, sc = data500
    fwd, rev = sc[model]
    assert len(names) == 499
    assert int((rev > fwd).sum()) == 232 and int((rev == fwd).sum()) == 22
    assert (names[int(np.argmax(fwd))], int(fwd.max())) == ("db211", 78)
    best, strand = SC.merge(fwd, rev)
    order = np.argsort(-best.astype(np.int64), kind="stable")[:6]
    assert [(names[k], "fr"[strand[k]], int(best[k])) for k in order] == [
        ("db35", "r", 83), ("db198", "r", 79), ("db211", "f", 78), ("db428", "f", 72),
        ("db41", "r", 70), ("db454", "f", 70)]


@pytest.mark.parametrize("model", MODELS)
def test_rc_query_equivalence(data500, model):
    """ssearch36 scores the reverse strand as (rc(query), target); the bank as (query,
    rc(target)).  Under these penalties (no first-column case, a complement-symmetric matrix)
    0 of 499 differ."""
    names, q, seqs, sc = data500
    assert SC.REF[0] <= -(SC.REF[2] + SC.REF[3])  # max(s) <= open + extend
    assert all(SUB[a][b] == SUB[a ^ 2][b ^ 2] for a in range(4) for b in range(4))
    theirs = O.score_batch(SC.revcomp(q), *O.pack_residues(seqs), SUB, SC.REF[2], SC.REF[3], model)
    assert int((theirs != sc[model][1]).sum()) == 0


def test_strands500_fixture(data500):
    names, q, seqs, sc = data500
    rows = SC.load_strands500()
    for model in MODELS:  # one fixture serves both models
        fwd, rev = sc[model]
        best, strand = SC.merge(fwd, rev)
        assert rows == [(n, int(f), int(r), int(s)) for n, f, r, s in zip(names, fwd, rev, strand)]


@pytest.mark.parametrize("model", MODELS)
def test_db35_reverse_alignment(data500, model):
    names, q, seqs, _ = data500
    k = names.index("db35")
    t = SC.revcomp(seqs[k])
    ends = AC.brute_ends(O, q, t, SUB, SC.REF[2], SC.REF[3], model)
    ref = C.ref_path(q, t, SUB, SC.REF[2], SC.REF[3], model, ends)
    assert ends[0] == 83
    assert S.cigar_string(ref.ops) == "25M2I10M"
    assert (ref.n_columns, ref.n_identities) == (37, 27)


def test_strand_alignments500_fixture(data500):
    names, q, seqs, _ = data500
    rows = SC.load_strand_alignments500()
    assert [(r["name"], r["score"]) for r in rows] == [("db35", 83), ("db198", 79), ("db41", 70)]
    for r in rows:
        k = r["index"]
        assert names[k] == r["name"] and len(seqs[k]) == r["length"]
        t = SC.revcomp(seqs[k])
        ends = AC.brute_ends(O, q, t, SUB, SC.REF[2], SC.REF[3], O.GAP_MERGED)
        ref = C.ref_path(q, t, SUB, SC.REF[2], SC.REF[3], O.GAP_MERGED, ends)
        assert SC.flip_ends(ends, len(t)) == (r["score"], r["q_start"], r["q_end"], r["t_start"],
                                              r["t_end"])
        assert r["t_start"] <= r["t_end"]
        assert tuple(AC.parse_cigar(r["cigar"])) == tuple(ref.ops)
        assert (ref.n_columns, ref.n_identities) == (r["n_columns"], r["n_identities"])


def test_flip_record():
    a = S.Alignment(3, 3, 83, 0, 30, 66, 47, 81, 37, 27, (25 << 4, 2 << 4 | 1, 10 << 4), "25M2I10M")
    b = SC.flip_record(a, 128)
    assert (b.t_start, b.t_end, b.flags, b.reverse, b.has_path) == (46, 80, 8, True, True)
    assert (b.q_start, b.q_end, b.ops, b.score) == (a.q_start, a.q_end, a.ops, a.score)
    e = S.Alignment(0, 0, 0, S.ALIGN_EMPTY, 0, 0, 0, 0, 0, 0)
    f = SC.flip_record(e, 0)
    assert (f.flags, f.t_start, f.t_end, f.empty, f.reverse) == (S.ALIGN_EMPTY | 8, 0, 0, True, True)


# ---- asymmetric matrices and the first-column rule on the reverse strand --------------------------
def test_reverse_mutants_are_what_they_say():
    """On a stored code c = comp(t) the right smat'[q][c] = sub[q][comp c] gives sub[q][t]; the
    four wrong ones are different matrices under every asymmetric DNA matrix; under a match /
    mismatch table the complemented rows and the transposed matrix are the right matrix (no test
    built on set_penalties can see them), the other two amount to a missing complement."""
    for name in ("asym-pair", "asym-ncol", "asym-odd"):
        sub = MC.matrix_param(name, O.GAP_GOTOH).sub
        muts = MC.reverse_mutants(sub)
        assert sorted(muts) == ["both-sides", "no-complement", "rows", "transposed"]
        assert all((m != sub).any() for m in muts.values())
        assert np.array_equal(muts["transposed"], sub.T)
        assert np.array_equal(muts["no-complement"], sub[:, MC.COMP])
    hidden = MC.reverse_mutants(SUB)
    assert all(np.array_equal(hidden[k], SUB) for k in ("rows", "transposed"))
    assert np.array_equal(hidden["both-sides"], hidden["no-complement"])
    assert (hidden["no-complement"] != SUB).any()


@pytest.mark.parametrize("name,model", MC.DNA_PARAMS)
def test_matrix_family_reverse_mutants(name, model):
    """A strand kernel that built smat' from the matrix uncomplemented, with the rows
    complemented, from the transposed matrix or with both sides complemented: each changes the
    score of >= 80 % of the family's positive hits and at least one record (the table of
    tests/matrix_cases.py records the figures)."""
    P = MC.matrix_param(name, model)
    g = MC.matrix_family(P)
    for mutant, sub2 in MC.reverse_mutants(P.sub).items():
        check_mutant(g, P, "reverse " + mutant, sub2)


def test_strand_form_alternates_and_flips_back():
    g = MC.matrix_family(MC.matrix_param("asym-ncol", O.GAP_MERGED))
    stored, strands = MC.strand_form(g)
    assert strands.tolist() == [k % 2 for k in range(len(g.seqs))]
    assert any((t == 4).any() for t, s in zip(stored, strands) if s)
    for t, s, st in zip(g.seqs, stored, strands):
        assert np.array_equal(SC.revcomp(s) if st else s, t)
    rev = [h for h in MC.positive(g) if strands[h]]
    assert len(rev) >= 20
    for h in rev:  # the flipped coordinates are those of brute force on the stored target's rc
        e = SC.flip_ends(g.brute[h], len(stored[h]))
        assert (e[3], e[4]) == (len(stored[h]) - 1 - g.brute[h][4], len(stored[h]) - 1 - g.brute[h][3])


def test_col0_family():
    """Merged 3 / -3 / -1 / -1 (max(s) > open + extend): of the reverse hits of the strand form
    at least a quarter have an alignment that must use the reverse target's first column (the
    stored target's last code: leaving it out lowers the score), and on at least a quarter the
    first-column rule is alive: applying it at the other end of the target (which is what
    scoring rc(query) against the stored target amounts to) gives another score."""
    g = MC.col0_family()
    P = MC.col0_param()
    assert P.model == O.GAP_MERGED and int(P.sub.max()) > -(P.go + P.ge)
    kinds, want, mirror, touches = g.meta
    lens = [len(t) for t in g.seqs]
    assert max(lens) <= 200 and set(MC.BOUNDARY_LENS) <= set(lens) and len(g.seqs) == 48
    stored, strands = MC.strand_form(g)
    fwd, rev = SC.oracle_strands(g.q, stored, (3, -3, P.go, P.ge), P.model)
    best, strand = SC.merge(fwd, rev)
    hits = strands == 1
    assert np.array_equal(rev[hits], want[hits]) and np.array_equal(fwd[~hits], want[~hits])
    n = int(hits.sum())
    assert n == 24 and int(strand[hits].sum()) >= 18  # the reverse strand wins where it should
    alive = hits & (want != mirror)
    print(f"\n    col0: {int((touches & hits).sum())} of {n} reverse hits need the first column, "
          f"the rule is alive on {int(alive.sum())}", end="")
    assert 4 * int((touches & hits).sum()) >= n and 4 * int(alive.sum()) >= n


def test_col0_has_no_reversed_start():
    """Why the col0 family carries scores only: include/swbank.h defines an alignment's start by
    the end rule on the reversed prefixes, and under the first-column rule the reversed
    prefixes of some pairs do not score what the pair scores (brute_ends_batch asserts that
    they do).  The alignment entries refuse these penalties (SW_ERR_UNSUPPORTED; the GPU
    tests' refusals), so there is no record to expect."""
    g = MC.col0_family()
    with pytest.raises(AssertionError, match="reversed prefixes"):
        C.brute_batch(g.q, g.seqs, MC.col0_param())
