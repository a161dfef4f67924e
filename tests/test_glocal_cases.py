"""The model of the global-local search on the CPU (tests/glocal_cases.py): the C model against the
plain-Python restatement of the definition, the anchors that tie the three modes to each other and
to the oracle's local score, the tie rules, the liveness of the seam plants and of the asymmetric
matrix that the GPU tests rely on, and what the library publishes."""
import ctypes
import os
import re

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import glocal_cases as G
import seam_cases as SEAMS
import strand_cases as SC

GO = (0, -1, -8, -12, -100)
GE = (0, -1, -4, -30)


def _tiny(seed, count):
    """[(q, t, sub, go, ge, ends, both)]: m <= 9, L <= 12 (0 among them), DNA 5 / -4 and a random
    asymmetric 5 x 5 matrix in turn, every mode, every go and ge of the lists."""
    rng = np.random.default_rng([229, seed])
    out = []
    for k in range(count):
        m = int(rng.integers(1, 10))
        L = 0 if k % 17 == 0 else int(rng.integers(0, 13))
        q = rng.integers(0, 5 if k % 6 == 0 else 4, m).astype(np.uint8)
        t = rng.integers(0, 5 if k % 4 == 0 else 4, L).astype(np.uint8)
        if k % 3 == 0 and L >= 4:  # a shared piece, so matches, gaps and boundaries compete
            w = min(m, L - 1)
            t[1:1 + w] = q[:w]
        sub = G.dna() if k % 2 else rng.integers(-9, 10, (5, 5)).astype(np.int8)
        out.append((q, t, sub, GO[k % 5], GE[(k // 5) % 4], G.MODES[k % 3], k % 2 == 0))
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_c_model_equals_the_python_restatement(seed):
    """120 tiny pairs per seed (360 in all): score, end position and strand, with the real
    -infinity of the restatement."""
    cases = _tiny(seed, 120)
    assert sum(1 for c in cases if len(c[1]) == 0) >= 7
    assert {(c[3], c[4]) for c in cases} == {(a, b) for a in GO for b in GE}
    for k, (q, t, sub, go, ge, ends, both) in enumerate(cases):
        want = G.py_search(q, t, sub, go, ge, ends, both)
        sc, ep, sd = G.c_search(q, [t], sub, go, ge, ends, both)
        assert (int(sc[0]), int(ep[0]), int(sd[0])) == want, (seed, k, ends, both, go, ge)


def test_target_mode_is_query_mode_transposed():
    """TARGET(q, t, S) = QUERY(t, q, S^T), score and end."""
    for k, (q, t, sub, go, ge, _, _) in enumerate(_tiny(3, 150)):
        if len(t) == 0:
            continue
        a = G.c_search(q, [t], sub, go, ge, G.TARGET)
        b = G.c_search(t, [q], np.ascontiguousarray(sub.T), go, ge, G.QUERY)
        assert (int(a[0][0]), int(a[1][0])) == (int(b[0][0]), int(b[1][0])), k


def test_local_bounds_the_modes_and_the_modes_bound_both():
    """The oracle's local Gotoh score >= QUERY and TARGET, and each of those >= BOTH."""
    for k, (q, t, sub, go, ge, _, _) in enumerate(_tiny(4, 150)):
        local = O.score_pair(q, t, sub, go, ge, O.GAP_GOTOH) if len(t) else 0
        sq, st, sb = (int(G.c_search(q, [t], sub, go, ge, e)[0][0]) for e in G.MODES)
        assert local >= sq >= sb and local >= st >= sb, (k, local, sq, st, sb)


def test_a_whole_query_in_n_flanks_scores_as_the_local_search():
    """An exact plant of the whole query between flanks of N: the local score and the QUERY score
    are both 5 m, the end is the plant's last column; TARGET and BOTH pay for the flanks."""
    rng = np.random.default_rng(233)
    for m in (1, 7, 64, 65, 300):
        q = rng.integers(0, 4, m).astype(np.uint8)
        t = np.concatenate([np.full(6, 4), q, np.full(9, 4)]).astype(np.uint8)
        local = O.score_pair(q, t, G.dna(), *G.DNA_PEN, O.GAP_GOTOH)
        sc, ep, _ = G.c_search(q, [t], G.dna(), *G.DNA_PEN, G.QUERY)
        assert local == int(sc[0]) == 5 * m and int(ep[0]) == 6 + m - 1
        for e in (G.TARGET, G.BOTH):
            assert int(G.c_search(q, [t], G.dna(), *G.DNA_PEN, e)[0][0]) < 5 * m


def test_strand_tie_goes_forward():
    """A target equal to its own reverse complement scores the same on both strands: strand 0."""
    rng = np.random.default_rng(239)
    q = rng.integers(0, 4, 15).astype(np.uint8)
    t = np.concatenate([q, SC.revcomp(q)])
    assert np.array_equal(SC.revcomp(t), t)
    for e in G.MODES:
        sc, ep, sd = G.c_search(q, [t], G.dna(), *G.DNA_PEN, e, True)
        assert int(sd[0]) == 0
        assert G.py_search(q, t, G.dna(), *G.DNA_PEN, e, True) == (int(sc[0]), int(ep[0]), 0)
        if e == G.QUERY:
            assert (int(sc[0]), int(ep[0])) == (75, 14)


def test_a_window_planted_twice_gives_the_smaller_end():
    rng = np.random.default_rng(241)
    q = rng.integers(0, 4, 20).astype(np.uint8)
    gap = np.full(5, 4, np.uint8)
    t = np.concatenate([gap, q, gap, q, gap])
    sc, ep, _ = G.c_search(q, [t], G.dna(), *G.DNA_PEN, G.QUERY)
    assert (int(sc[0]), int(ep[0])) == (100, 24)
    # TARGET: the target planted twice in the query; the smaller row
    sc, ep, _ = G.c_search(t, [q], G.dna(), *G.DNA_PEN, G.TARGET)
    assert (int(sc[0]), int(ep[0])) == (100, 24)
    # on the reverse strand the end is given on the forward target: the smaller column of the
    # strand walked is the larger one there
    sc, ep, sd = G.c_search(q, [SC.revcomp(t)], G.dna(), *G.DNA_PEN, G.QUERY, True)
    assert (int(sc[0]), int(ep[0]), int(sd[0])) == (100, len(t) - 1 - 24, 1)


def test_an_all_gap_query_ends_at_the_boundary():
    """Nothing in the target is worth a column: the score is H(m-1,-1), the end SW_END_NONE."""
    q = np.zeros(3, np.uint8)
    t = np.full(5, 1, np.uint8)
    sub = np.full((5, 5), -100, np.int8)
    sc, ep, _ = G.c_search(q, [t, t[:0]], sub, -1, -1, G.QUERY)
    assert sc.tolist() == [-4, -4] and ep.tolist() == [G.END_NONE] * 2
    sc, ep, _ = G.c_search(q, [t, t[:0]], sub, -1, -1, G.TARGET)
    assert sc.tolist() == [-6, 0] and ep.tolist() == [G.END_NONE] * 2
    sc, ep, _ = G.c_search(q, [t, t[:0]], sub, -1, -1, G.BOTH)
    assert sc.tolist() == [-4 - 6, -4] and ep.tolist() == [G.END_NONE] * 2


@pytest.mark.parametrize("K", G.ROWS)
def test_seam_plants_are_live(K):
    """Per rows-per-lane count: of the four plants tried across a lane seam, and of the four
    across a block seam, at least three change the model's score when the mutant drops F
    (respectively E) at the seam.  Measured: 4 of 4 in every group."""
    q, plants = G.seam_plants(K)
    assert S.lib().swk_glocal_rows(len(q)) == K and len(q) > 64 * K - K
    flags = G.live(q, plants, G.dna(), *G.DNA_PEN)
    for kind in ("lane", "block"):
        got = [f for (k, _, _), f in zip(plants, flags) if k == kind]
        print(K, kind, sum(got), "of", len(got))
        assert len(got) == 4 and sum(got) >= 3, (K, kind, got)
    for kind, t, (what, at) in plants:
        assert at % (K if kind == "lane" else 64) == 0 and what == (1 if kind == "lane" else 2)


def test_the_transposed_matrix_moves_most_scores():
    """asym-pair at -12 / -4: a kernel reading s(t, q) cannot pass.  Measured: see DESIGN §3.17."""
    q, seqs = G.asym_case()
    sub = SEAMS.MATRICES[G.ASYM]()
    for e in G.MODES:
        share = G.transposed_share(q, seqs, sub, *G.ASYM_PEN, e, True)
        print(e, share)
        assert share > 0.5, (e, share)


def test_every_real_cell_stays_above_the_documented_floor():
    """-(|o| + (m + L) max(|e|, |smallest entry|)) bounds every result of the tiny cases."""
    for q, t, sub, go, ge, ends, both in _tiny(5, 150):
        sc = int(G.c_search(q, [t], sub, go, ge, ends, both)[0][0])
        assert sc >= -(abs(go + ge) + (len(q) + len(t)) * max(abs(ge), abs(int(sub.min()))))


def test_the_library_publishes_the_calls():
    """The header's names reach Python, refuse a NULL bank, and the ABI version stays 6."""
    assert (S.ENDS_QUERY, S.ENDS_TARGET, S.ENDS_BOTH) == G.MODES and S.END_NONE == G.END_NONE
    assert S.GLOCAL_MAX_QUERY == G.MAX_QUERY
    assert hasattr(S.ScoreBank, "score_glocal") and hasattr(S.ScoreBank, "score_glocal_device")
    assert {"sw_score_glocal", "sw_score_glocal_device"} <= set(S.EXPORTS)
    lib = S.lib()
    assert lib.sw_score_glocal(None, None, 0, None, None, 1, 1, 0, None, None, None) == S.ERR_ARG
    assert lib.sw_score_glocal_device(None, None, None, None, 1, 1, 1, 0, None, None, None,
                                      None) == S.ERR_ARG
    lib.swk_glocal_rows.restype = ctypes.c_int
    lib.swk_glocal_rows.argtypes = [ctypes.c_uint32]
    assert [lib.swk_glocal_rows(m) for m in (1, 256, 257, 512, 513, 1024)] == [4, 4, 8, 8, 16, 16]
    header = open(os.path.join(os.path.dirname(O.REPO + "/"), "include", "swbank.h")).read()
    assert re.search(r"#define SWBANK_ABI_VERSION 6\b", header) and lib.sw_abi_version() == 6
    assert re.search(r"#define SWBANK_HAS_GLOCAL 1\b", header)
    assert re.search(r"#define SW_GLOCAL_MAX_QUERY 1024\b", header)
    assert re.search(r"SW_ENDS_QUERY = 1, SW_ENDS_TARGET = 2, SW_ENDS_BOTH = 3", header)
