"""The models of the non-intersecting local alignments (tests/disjoint_cases.py) on the CPU: the C
model agrees with the plain-Python restatement record for record and op for op; the anchors that
follow from the definition hold on every record (score_0 is the oracle's local Gotoh score, scores
never increase, each path re-scores to its score, the paths of a pair are cell-disjoint, first and
last op are M, round 0 is an alignment sw_align_hits could return); the plants of the GPU tests
are live in the model; and the library declares and exports the two entries."""
import re

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_check as AC
import disjoint_cases as D
import glocal_cases as G
import seam_cases as SEAMS
import test_abi as ABI

PENS = G.ENVELOPE + (G.DNA_PEN,)
MATRICES = ("dna", G.ASYM, "blosum62")


def _alignment(rec, ops):
    return S.Alignment(0, 0, *rec, ops=tuple(ops), cigar=D.cigar(ops))


def _anchors(q, t, sub, go, ge, got, check_round0=True):
    """What holds for the records of one pair whatever the path preference."""
    want0 = O.score_pair(q, t, sub, go, ge, O.GAP_GOTOH) if len(q) and len(t) else 0
    sc = D.scores(got)
    assert sc[0] == want0 and sc == sorted(sc, reverse=True), (sc, want0)
    seen = set()
    for r, (rec, ops) in enumerate(got):
        if rec[1] & D.EMPTY:
            assert (rec, ops) == D.EMPTY_REC and all(x == D.EMPTY_REC for x in got[r:])
            continue
        assert rec[0] >= 1 and rec[1] == 0 and ops
        assert ops[0] & 15 == D.OP_M and ops[-1] & 15 == D.OP_M, D.cigar(ops)
        s, dq, dt, cols, idn = AC.rescore(ops, q, t, rec[2], rec[4], sub, go, ge, AC.GAP_GOTOH)
        assert s == rec[0] and (dq, dt) == (rec[3] - rec[2] + 1, rec[5] - rec[4] + 1)
        assert (cols, idn) == rec[6:]
        path = D.cells(rec, ops)
        assert len(path) == cols == len(set(path)) and not seen & set(path), (r, rec)
        assert path[0] == (rec[2], rec[4]) and path[-1] == (rec[3], rec[5])
        seen |= set(path)
    if check_round0:
        AC.check_alignment(O, q, t, sub, go, ge, AC.GAP_GOTOH, _alignment(*got[0]))


def test_c_model_equals_python_model_on_tiny_pairs():
    """600 seeded pairs of at most 9 rows and 11 columns (L = 0 among them), five rounds each, over
    (0, 0) to (-100, -10) penalties and random asymmetric matrices: the C model's records and ops
    are the Python model's, and the anchors hold."""
    deep = zero = 0
    for q, t, sub, go, ge in D.tiny_pairs():
        want = D.py_rounds(q, t, sub, go, ge, 5)
        got = D.c_rounds(q, t, sub, go, ge, 5)
        assert got == want, (q, t, sub.tolist(), go, ge, got, want)
        _anchors(q, t, sub, go, ge, got)
        deep += sum(1 for rec, _ in got if not rec[1] & D.EMPTY) >= 3
        zero += len(t) == 0
    assert deep >= 200 and zero >= 5


def _envelope_pairs(name):
    sub = SEAMS.MATRICES[name]()
    alpha = sub.shape[0]
    letters = 4 if alpha == 5 else 20
    rng = np.random.default_rng([419, alpha, len(name)])
    out = []
    for k in range(6):
        m, L = int(rng.integers(12, 40)), int(rng.integers(20, 60))
        q = rng.integers(0, letters, m).astype(np.uint8)
        t = rng.integers(0, letters, L).astype(np.uint8)
        if k % 2 == 0:  # two noisy copies of a window of the query
            w = q[m // 4:m - 2].copy()
            v = np.delete(w, len(w) // 2)
            w[len(w) // 3] = (int(w[len(w) // 3]) + 1) % letters
            t = np.concatenate([t[:5], w, t[5:9], v, t[9:12]]).astype(np.uint8)
        out.append((q, t))
    return sub, out


@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("pen", PENS, ids=str)
def test_c_model_equals_python_model_across_the_envelope(name, pen):
    """The five penalty pairs of glocal_cases.ENVELOPE and -12 / -4 under 5 / -4, the asymmetric
    DNA matrix and BLOSUM62: six pairs each, half of them with two noisy copies, four rounds."""
    sub, pairs = _envelope_pairs(name)
    for q, t in pairs:
        want = D.py_rounds(q, t, sub, *pen, 4)
        got = D.c_rounds(q, t, sub, *pen, 4)
        assert got == want, (name, pen, got, want)
        _anchors(q, t, sub, *pen, got)


def test_min_score_and_the_ops_cap():
    """min_score above a round's score empties that round and all later ones; a cap below a
    path's ops gives NO_PATH with the same coordinates, and later rounds do not change."""
    q, t, _ = D.copies_case()
    sub = G.dna()
    full = D.c_rounds(q, t, sub, *G.DNA_PEN, 4)
    sc = D.scores(full)
    assert sc[0] > sc[1] > sc[2] > 0
    cut = D.c_rounds(q, t, sub, *G.DNA_PEN, 4, min_score=sc[2] + 1)
    assert cut[:2] == full[:2] and cut[2:] == [D.EMPTY_REC] * 2
    assert D.c_rounds(q, t, sub, *G.DNA_PEN, 4, min_score=sc[0] + 1) == [D.EMPTY_REC] * 4
    short = D.c_rounds(q, t, sub, *G.DNA_PEN, 4, cap=2)
    assert [len(ops) for _, ops in full[:3]] == [1, 1, 3] and full[3][1]
    assert short[:2] == full[:2] and short[3] == full[3]
    assert short[2] == (full[2][0][:1] + (D.NO_PATH,) + full[2][0][2:6] + (0, 0), ())


def test_planted_copies_and_the_internal_repeat():
    """Three copies come back in score order (exact, substitution, indel) and a fourth round at
    min_score between is empty; the query's repeat reuses the target range with another query
    range in round 1."""
    q, t, (a, b) = D.copies_case()
    n = b - a
    rest = D.scores(D.c_rounds(q, t, G.dna(), *G.DNA_PEN, 4))[3]
    assert 0 < rest < 200 < 5 * (n - 1) - 16  # (what is left once the three copies are used)
    got = D.c_rounds(q, t, G.dna(), *G.DNA_PEN, 4, min_score=200)
    assert D.scores(got) == [5 * n, 5 * (n - 1) - 4, 5 * (n - 1) - 16, 0]
    assert [rec[4] for rec, _ in got[:3]] == [7 + n + 9, 7, 7 + n + 9 + n + 5]
    assert D.cigar(got[0][1]) == f"{n}M" and "I" in D.cigar(got[2][1])
    _anchors(q, t, G.dna(), *G.DNA_PEN, got)
    q, t = D.repeat_case()
    r0, r1 = [rec for rec, _ in D.c_rounds(q, t, G.dna(), *G.DNA_PEN, 2)]
    assert r0[0] == r1[0] == 200 and (r0[4], r0[5]) == (r1[4], r1[5]) == (6, 45)
    assert (r0[2], r0[3]) == (9, 48) and (r1[2], r1[3]) == (62, 101)


@pytest.mark.parametrize("K", D.ROWS)
def test_seam_plants_are_live_in_the_model(K):
    """Per family at least 3 of the 4 plants change a model score under their mutant (the GPU
    test keeps exactly those): K = 4 loses the lane plant before its first seam and the block
    plant behind column 256, where too few rows remain to pay for the gap."""
    fams = D.seam_plants(K)
    for family, plants in fams.items():
        assert len(plants) == 4 and {p[2][0] for p in plants} == {D.FAMILIES[family]}
        flags = D.live(plants, G.dna(), *G.DNA_PEN)
        assert sum(flags) >= 3, (K, family, flags)
        for q, t, _ in plants:
            assert len(q) == 64 * K - 3
    for q, t, drop in fams["row"] + fams["column"]:  # round 1 of the definition is empty
        got = D.c_rounds(q, t, G.dna(), *G.DNA_PEN, 2)
        assert D.scores(got) == [20, 0]
        assert D.scores(D.c_rounds(q, t, G.dna(), *G.DNA_PEN, 2, drop=drop)) == [20, 5]


def test_header_declares_and_library_exports_the_entries():
    """include/swbank.h declares sw_align_disjoint_hits[_device] and the feature macro with its
    limits, the library exports both, and both refuse a NULL bank."""
    names = ("sw_align_disjoint_hits", "sw_align_disjoint_hits_device")
    declared = ABI._declared()
    txt = open(ABI.HEADER).read()
    for name in names:
        assert name in declared and name in S.EXPORTS and hasattr(S.lib(), name)
    assert re.search(r"#define\s+SWBANK_HAS_DISJOINT_ALIGN\s+1\b", txt)
    assert re.search(r"#define\s+SW_DISJOINT_MAX_QUERY\s+1024\b", txt)
    assert re.search(r"#define\s+SW_DISJOINT_MAX_ROUNDS\s+64\b", txt)
    assert (S.DISJOINT_MAX_QUERY, S.DISJOINT_MAX_ROUNDS) == (D.MAX_QUERY, D.MAX_ROUNDS) == (1024, 64)
    assert S.lib().sw_abi_version() == 6
    L = S.lib()
    assert L.sw_align_disjoint_hits(None, None, 0, None, None, None, 0, 1, 1, None, 0, None, 0,
                                    None, None, 0, None) == S.ERR_ARG
    assert L.sw_align_disjoint_hits_device(None, None, None, None, None, 0, 0, 1, 1, None, 0, None,
                                           0, None, None, 0, None) == S.ERR_ARG
