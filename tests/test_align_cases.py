"""The reference traceback and the inputs of tests/test_gpu_align_seams.py, on the CPU.

The GPU tests compare the alignment kernels' CIGARs with align_cases.ref_path on inputs built
by tests/align_cases.py.  That proves something only if (1) the reference is right where the
answer is known, and (2) the inputs put a live gap, a tie or a window edge where they claim to.
Building a family checks (2) (it raises otherwise); this module builds every one and checks its
shape, and checks (1) on the ssearch36 fixture, the corner-turning pair and random pairs.  The
matrix family of tests/matrix_cases.py (asymmetric matrices) is live by matrix mutants: section 3."""
import collections
import os

import numpy as np
import pytest

from oracle import oracle as O

import align_cases as C
import align_check as AC
import matrix_cases as MC

ABC = [(tag, model) for tag in C.DNA_SETS for model in C.MODELS]


# ---- 1. the reference traceback --------------------------------------------------------------
@pytest.mark.parametrize("model", C.MODELS)
def test_ref_path_reproduces_ssearch36(model):
    """Both hits of tests/golden/alignments500.tsv, field for field."""
    recs = dict(O.read_fasta(O.golden_fasta("data500.fa")))
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    rows = [ln.rstrip("\n").split("\t")
            for ln in open(os.path.join(O.GOLDEN, "alignments500.tsv"))][1:]
    assert [r[0] for r in rows] == ["db211", "db428"]
    for r in rows:
        t = O.encode_dna(recs[r[0]])
        ends = AC.brute_ends(O, q, t, O.dna_matrix(), -12, -4, model)
        ref = C.ref_path(q, t, O.dna_matrix(), -12, -4, model, ends)
        assert ends + (ref.n_columns, ref.n_identities) == tuple(int(x) for x in r[1:8])
        assert ref.ops == AC.parse_cigar(r[8])


def test_ref_path_turns_the_corner():
    """The pair of test_gpu_align.test_corner_turning_gap: merged 20M3I2D20M (the gap from the
    left comes first walking back, so the I ops precede the D ops), a left / up tie on the way;
    Gotoh takes one gap and two mismatches."""
    enc = O.encode_dna
    a, b = "ACGTTGCAAGCTTAGCATCA", "TTAGGCATCGATCCGATTAC"
    q, t = enc(a + "CCC" + b), enc(a + "GG" + b)
    m = C.ref_path(q, t, O.dna_matrix(), -10, -1, C.GAP_MERGED)
    assert m.ops == AC.parse_cigar("20M3I2D20M") and (m.n_columns, m.n_identities) == (45, 40)
    assert m.ties["lu"] >= 1
    g = C.ref_path(q, t, O.dna_matrix(), -10, -1, C.GAP_GOTOH)
    assert sorted(op & 15 for op in g.ops) == [0, 0, 1]


def test_ref_path_of_an_empty_pair():
    enc = O.encode_dna
    assert C.ref_path(enc("AAAA"), enc("CCCC"), O.dna_matrix(), -12, -4, C.GAP_MERGED) is None
    assert C.ref_paths(enc("AAAA"), [np.zeros(0, np.uint8)], [(0, 0, 0, 0, 0)], O.dna_matrix(),
                       -12, -4, C.GAP_GOTOH) == [None]


@pytest.mark.parametrize("model", C.MODELS)
def test_ref_path_rescores(model):
    """50 random planted pairs (DNA REF and ALT, protein for Gotoh): the ops span the window
    and re-score to the brute-force score under the model's gap-run rule; the first and last op
    are M."""
    rng = np.random.default_rng(50 + model)
    sets = [C.dna_param("ref", model), C.dna_param("alt", model)]
    if model == C.GAP_GOTOH:
        sets.append(C.protein_param())
    gapped = 0
    for P in sets:
        q = rng.integers(0, P.letters, 300).astype(np.uint8)
        seqs = [C.planted(rng, q, int(rng.integers(20, 280)), P.letters)
                for _ in range(50 // len(sets) + 1)]
        brute, refs = C.prepare(q, seqs, P)
        for t, b, r in zip(seqs, brute, refs):
            assert b[0] > 0
            s, dq, dt, cols, idn = AC.rescore(r.ops, q, t, b[1], b[3], P.sub, P.go, P.ge, P.model)
            assert (s, dq, dt) == (b[0], b[2] - b[1] + 1, b[4] - b[3] + 1)
            assert (cols, idn) == (r.n_columns, r.n_identities)
            assert r.ops[0] & 15 == AC.M and r.ops[-1] & 15 == AC.M
            gapped += len(r.ops) > 1
    assert gapped >= 25


# ---- 2. the families ---------------------------------------------------------------------------
def _check_seams(g):
    count = collections.Counter((pas, seam, "short" if run <= 6 else run)
                                for pas, seam, run in g.meta)
    for pas, seam in C.seam_rows():
        assert count[(pas, seam, "short")] >= (2 if pas == "A" else 4), (g.name, pas, seam)
        for run in C.SEAM_RUNS if pas != "A" else ():
            assert count[(pas, seam, run)] >= 1, (g.name, pas, seam, run)
    for pas, seam in C.tight_rows():  # pass B shows only in the start: see align_cases.tight_rows
        assert count[(pas, seam, "short")] >= 2, (g.name, pas, seam)
    assert len(g.seqs) == len(g.brute) == len(g.refs) == sum(count.values())
    assert all(r is not None and len(r.ops) >= 3 for r in g.refs)


@pytest.mark.parametrize("tag,model", ABC)
def test_seam_family(tag, model):
    """Family a: >= 4 live targets per (pass B | C, seam), a 9- and a 13-row run at each, and
    forward-seam targets in the same batch (building the family asserts that the pass's
    gap-dropping mutant changes each score and that the reference path runs an I over the seam).
    The three seam sets are different rows: the window starts off a lane boundary."""
    rows = C.seam_rows()
    assert len(set(rows.values())) == 6 and C.SEAM_WINDOW[0] % 4
    _check_seams(C.seam_family(C.dna_param(tag, model)))


def test_seam_family_protein():
    _check_seams(C.seam_family(C.protein_param()))


def test_free_extension_is_the_only_omission():
    """Families a-c run REF and ALT under both models; the free-extension set is left out by
    name (align_cases.FREE_EXTENSION_LEFT_OUT) and nothing else is."""
    assert C.FREE_EXTENSION_LEFT_OUT[1][3] == 0
    assert C.DNA_SETS == {"ref": (5, -4, -12, -4), "alt": (5, -4, -10, -1)}


@pytest.mark.parametrize("tag,model", ABC)
def test_edge_family(tag, model):
    """Family b: windows of exactly 255 .. 513 rows and of exactly 63 .. 129 columns (from
    brute_ends), the indel's last cell 7 cells from the window's last row or column."""
    g = C.edge_family(C.dna_param(tag, model))
    assert [m for m in g.meta] == [("rows", h) for h in (255, 256, 257, 511, 512, 513)] + \
        [("cols", w) for w in (63, 64, 65, 127, 128, 129)]
    for (kind, size), b, r in zip(g.meta, g.brute, g.refs):
        assert (b[2] - b[1] + 1 if kind == "rows" else b[4] - b[3] + 1) == size and b[1] % 4
        run = C.runs_of(r.ops, AC.I if kind == "rows" else AC.D)
        assert len(run) == 1 and size - run[0][1] == 7


@pytest.mark.parametrize("tag,model", ABC)
def test_tie_family(tag, model):
    """Family c: every case has two maximal cells where it says (building asserts it on the
    model's H) and the record the tie rule asks for; the cells lie in different lanes of one
    strip, or in different strips."""
    groups = C.tie_family(C.dna_param(tag, model))
    assert [g.meta[0].name for g in groups] == list(C.TIE_CASES)
    for g in groups:
        tie = g.meta[0]
        (r1, c1), (r2, c2) = tie.cells
        assert g.brute[0][1:] == tie.want
        if "lanes" in tie.name:
            assert r1 // 256 == r2 // 256 and r1 // 4 != r2 // 4
        elif "columns" in tie.name:
            assert r1 == r2 and c1 // 64 != c2 // 64
        else:
            assert r1 // 256 != r2 // 256
        if tie.name == "end-strips-same-lane":
            assert (r1 % 256) // 4 == (r2 % 256) // 4
        if tie.name == "end-mixed":
            assert r1 > r2 and c1 < c2 and (tie.want[1], tie.want[3]) == (r1, c1)


@pytest.mark.parametrize("model", C.MODELS)
def test_tie_rich_family(model):
    """Family d: over the model's batch every kind of co-optimal move occurs on >= 20 path
    cells and >= a quarter of the pairs have another co-optimal path (building asserts it);
    paths cross the strip seam.  Prints the counts (pytest -s)."""
    groups = C.tie_rich_family(model)
    total = collections.Counter()
    for g in groups:
        total.update(g.meta[0])
        assert any(b[1] < 256 <= b[2] for b in g.brute)
    other, n = sum(g.meta[1] for g in groups), sum(len(g.seqs) for g in groups)
    assert min(total.values()) >= 20 and len(total) == 3 and 4 * other >= n
    print(f"\n    model {model}: {dict(total)}, {other} of {n} pairs with another path", end="")


@pytest.mark.parametrize("model", C.MODELS)
def test_reuse_case(model):
    """The scratch-reuse hit lists: >= 300 hits, more than swk_i32_waves gives waves at a
    1 MiB scratch budget, long (three-strip) and short or empty hits alternating."""
    g, order2 = C.reuse_case(C.dna_param("ref", model))
    longest = max(len(s) for s in g.seqs)
    assert C.i32_waves(len(g.hits), 700, 1 << 20) == 96
    waves = C.i32_waves(len(g.hits), longest, 1 << 20)
    assert len(g.hits) >= 300 and len(g.hits) > 2 * waves and len(order2) > 2 * waves
    lens = [len(g.seqs[h]) for h in g.hits]
    for w in range(waves):  # every wave takes a long and a short hit by turns
        mine = [a > 600 for a in lens[w::waves]]
        assert len(mine) >= 3 and all(x != y for x, y in zip(mine, mine[1:])), w
    assert all(a > 600 or a <= 40 for a in lens)
    assert 0 in lens and sorted(order2[1:-1]) == sorted(g.hits) and order2[1:-1] != g.hits
    assert len(set(g.hits)) < len(g.hits)


# ---- 3. asymmetric matrices ----------------------------------------------------------------------
def check_mutant(g, P, name, sub2):
    """A matrix mutant changes the score of >= 80 % of the group's positive hits, and the
    coordinates or the ops of at least one record.  Prints the figures (pytest -s)."""
    share, moved = MC.mutant_share(g, P, sub2), MC.mutant_moved(g, P, sub2)
    print(f"\n    {g.name} {name}: {100 * share:.0f} % ({moved})", end="")
    assert share >= 0.8, (g.name, name, share)
    assert moved >= 1, (g.name, name)


@pytest.mark.parametrize("name,model", MC.PARAMS)
def test_matrix_family(name, model):
    """The family builds for all eight sets: 48 targets of at most 760 codes with the boundary
    lengths among them, N in the DNA query and targets, an asymmetric matrix; every positive
    hit's reference path spans the window and re-scores to the brute-force score; >= 12 paths
    have an I or a D run; >= 8 windows span two or more 256-row strips, and one, two and three
    strips all occur."""
    P = MC.matrix_param(name, model)
    g = MC.matrix_family(P)
    assert len(MC.PARAMS) == 8 and (P.sub != P.sub.T).any() and P.sub.shape[0] in (5, 24)
    assert len(g.q) == MC.QLEN and len(g.seqs) == MC.N_TARGETS == len(g.hits)
    lens = [len(t) for t in g.seqs]
    assert max(lens) <= MC.MAX_TLEN and set(MC.BOUNDARY_LENS) <= set(lens)
    assert sum(1 for kind, _ in g.meta if kind == "noise") == 4
    if name != MC.PROTEIN:
        assert 0.01 < float((g.q == 4).mean()) < 0.06 and any((t == 4).any() for t in g.seqs)
    else:
        assert g.q.max() == 23 and max(int(t.max()) for t in g.seqs if len(t)) == 23
    live = MC.positive(g)
    assert len(live) >= 40
    runs, strips = 0, collections.Counter()
    for h in live:
        b, r, t = g.brute[h], g.refs[h], g.seqs[h]
        s, dq, dt, cols, idn = AC.rescore(r.ops, g.q, t, b[1], b[3], P.sub, P.go, P.ge, P.model)
        assert (s, dq, dt) == (b[0], b[2] - b[1] + 1, b[4] - b[3] + 1), (g.name, h)
        assert (cols, idn) == (r.n_columns, r.n_identities)
        assert r.ops[0] & 15 == AC.M and r.ops[-1] & 15 == AC.M
        runs += any(op & 15 != AC.M for op in r.ops)
        strips[(b[2] - b[1]) // 256 + 1] += 1
    assert all(g.refs[h] is None for h in g.hits if h not in live)
    assert runs >= 12, (g.name, runs)
    assert strips[2] + strips[3] >= 8 and min(strips[1], strips[2], strips[3]) >= 1, strips


def test_matrix_family_is_deterministic():
    P = MC.matrix_param("asym-ncol", C.GAP_GOTOH)
    g = MC.matrix_family(P)
    q, seqs, meta = MC._inputs(P, MC.WINDOW, (45, 210, 480, MC.MAX_TLEN), MC.MAX_TLEN)
    assert np.array_equal(q, g.q) and meta == g.meta
    assert all(np.array_equal(a, b) for a, b in zip(seqs, g.seqs))
    other = MC.matrix_family(MC.matrix_param("asym-ncol", C.GAP_MERGED))
    assert not np.array_equal(other.q, g.q)


@pytest.mark.parametrize("name,model", MC.PARAMS)
def test_matrix_family_transposed(name, model):
    """The forward mutant: a kernel that read the matrix transposed (the table of
    tests/matrix_cases.py records the figures)."""
    P = MC.matrix_param(name, model)
    for mutant, sub2 in MC.forward_mutants(P.sub).items():
        check_mutant(MC.matrix_family(P), P, mutant, sub2)
