"""The checker and the inputs of the seam and parameter tests, on the CPU.

tests/test_gpu_params.py and tests/test_gpu_seams.py compare the kernels with the C oracle on
inputs built by tests/seam_cases.py.  Those tests prove something only if (1) the oracle is
right at the parameters they use, (2) a kernel that loses the gap value at a seam would change
the scores of that seam's targets, (3) a transposed matrix would change the scores, and (4) the
large gap penalties are still paid by the optimal alignments.  This module asserts all four."""
import numpy as np
import pytest

from oracle import oracle as O

import seam_cases as SC

MODELS = [O.GAP_MERGED, O.GAP_GOTOH]
_ALL_CASES = SC.CASES + [SC.GOTOH_REFUSED]


def _py(q, t, sub, go, ge, model):
    if model == O.GAP_GOTOH:
        return O.py_score_gotoh(list(q), list(t), sub, go, ge)
    return O.py_score_merged(list(q), list(t), sub, go, ge)


# ---- 1. the C oracle against the independent pure-Python model, over the whole case table ----
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", _ALL_CASES, ids=lambda c: c.name)
def test_oracle_matches_pure_python(case, model):
    """30 random pairs up to 40 x 40 (N and empty sequences included) and 6 straddle pairs of
    150 x 150 (a gap is taken in the mid-range cases), every parameter case, both models."""
    sub = SC.MATRICES[case.matrix]()
    A = sub.shape[0]
    rng = np.random.default_rng(len(case.name) * 97 + model)
    letters = 4 if case.alphabet == SC.DNA else 20
    pairs = []
    for k in range(30):
        m, n = (int(rng.integers(0, 41)), int(rng.integers(0, 41))) if k else (40, 40)
        q = rng.integers(0, A, m).astype(np.uint8)
        t = rng.integers(0, A, n).astype(np.uint8)
        if k % 3 == 0 and m > 8:  # a homolog with an indel
            t = np.concatenate([q[:m // 2], q[m // 2 + 2:]])
        pairs.append((q, t))
    q = rng.integers(0, letters, 150).astype(np.uint8)
    st, _ = SC.straddle_targets(q, letters, (75,), (75,), 150, rng, per=3)
    assert len(st) == 6
    pairs += [(q, t) for t in st]
    for q, t in pairs:
        want = _py(q, t, sub, case.go, case.ge, model)
        assert O.score_pair(q, t, sub, case.go, case.ge, model) == want, (case.name, len(q), len(t))
    res, offs, lens = O.pack_residues([t for _, t in pairs[30:]])
    got = O.score_batch(pairs[30][0], res, offs, lens, sub, case.go, case.ge, model)
    assert got.tolist() == [_py(q, t, sub, case.go, case.ge, model) for q, t in pairs[30:]]


# ---- 2. mutant sensitivity of every seam family ------------------------------------------------
def _family_models(name):
    # the balanced tile ranges (uniform, and the ragged plan) run merged gaps only
    return [O.GAP_MERGED] if name.startswith(("tbal", "rbal")) else MODELS


@pytest.mark.parametrize("name", list(SC.SEAMS))
def test_seam_mutants_change_scores(name):
    """First and last seam of the family, every parameter set and gap model the GPU test runs:
    dropping the vertical gap state at the seam's row changes >= 50 % of its deletion targets,
    dropping the horizontal one at the seam's column >= 50 % of its insertion targets.  Cuts
    within 6 letters of an end (SC.tight_seams: K = 4 and the last short wave's boundary) carry
    a paid gap only where extension is free, and are held to the same 50 % at that set.  Prints
    the family's line of the table in tests/seam_cases.py's docstring (pytest -s)."""
    q, tg, mt = SC.seam_family(name)
    alphabet = SC.SEAMS[name].alphabet
    shares = {"del": [], "ins": [], "tight": []}
    for model in _family_models(name):
        for tag, mat, go, ge in SC.seam_params(alphabet, model):
            sub = SC.MATRICES[mat]()
            seams = [(k, c, k) for k, c in SC.first_last_seams(name)]
            if tag == "free":  # cuts too close to an end for a paid gap at the other sets
                seams += [(k, c, "tight") for k, c in SC.tight_seams(name)]
            for kind, cut, col in seams:
                dl, ins = SC.mutant_shares(O, q, tg, mt, sub, go, ge, model, cut)
                share = dl if kind == "del" else ins
                shares[col].append(share)
                assert share >= 0.5, (name, tag, model, kind, cut, share)
    assert shares["del"] or shares["ins"]
    print("\n    " + f"{name:14s}" + "".join(
        f"  {kind} {100 * min(v):3.0f}-{100 * max(v):3.0f} % ({len(v):2d})" if v else " " * 22
        for kind, v in shares.items()), end="")


# ---- 3. matrix asymmetry -----------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in SC.CASES if "asym" in c.tags], ids=lambda c: c.name)
def test_asymmetric_matrices_bite(case):
    """A transposed table (m[target * A + query]) would change >= 50 % of the scores."""
    sub = SC.MATRICES[case.matrix]()
    assert (sub != sub.T).any()
    for qlen in case.qlens:
        q, seqs, _ = SC.case_inputs(case, qlen)
        assert len(seqs) == 260
        for model in MODELS:
            a = SC.oracle_scores(O, q, seqs, sub, case.go, case.ge, model)
            b = SC.oracle_scores(O, q, seqs, np.ascontiguousarray(sub.T), case.go, case.ge, model)
            assert (a != b).mean() >= 0.5, (case.name, qlen, model, float((a != b).mean()))


# ---- 4. gap uptake ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in SC.CASES if "uptake" in c.tags], ids=lambda c: c.name)
def test_large_gaps_are_taken(case):
    """At the case's larger query length >= 50 % of the straddle targets score differently with
    gaps than without (-32767/-32767): the penalty is paid, not avoided."""
    sub = SC.MATRICES[case.matrix]()
    qlen = max(case.qlens)
    q, seqs, mt = SC.case_inputs(case, qlen)
    st = [t for t, m in zip(seqs, mt) if m is not None]
    assert len(st) >= 12
    for model in MODELS:
        with_gaps = SC.oracle_scores(O, q, st, sub, case.go, case.ge, model)
        without = SC.oracle_scores(O, q, st, sub, -32767, -32767, O.GAP_MERGED)
        share = float((with_gaps != without).mean())
        assert share >= 0.5, (case.name, qlen, model, share)


def test_case_table_shape():
    """The table holds what tests/test_gpu_params.py promises: unique names, two query lengths
    from 33, 300, 600 and 1,100, the f16 switch at 2047 / 2048 / 2049, the 16-bit limits."""
    names = [c.name for c in SC.CASES]
    assert len(set(names)) == len(names)
    for c in SC.CASES:
        assert len(c.qlens) == 2 and set(c.qlens) <= {33, 300, 600, 1100}, c
        m = SC.MATRICES[c.matrix]().astype(int)
        S = max(0, m.max())
        for t in (2047, 2048, 2049):
            if f"neg{t}" in c.tags:
                assert -c.go - 2 * c.ge + S - m.min() == t, c
        assert not SC.expect_range_error(c, O.GAP_MERGED) and not SC.expect_range_error(c, O.GAP_GOTOH) \
            or "merged-only" in c.tags, c
    g = {c.name: c for c in SC.CASES}
    assert -g["gotoh-65535"].go - g["gotoh-65535"].ge + 5 == 65535
    assert -SC.GOTOH_REFUSED.go - SC.GOTOH_REFUSED.ge + 5 == 65536
    assert SC.expect_range_error(SC.GOTOH_REFUSED, O.GAP_GOTOH)
    assert not SC.expect_range_error(SC.GOTOH_REFUSED, O.GAP_MERGED)
    assert SC.expect_range_error(g["merged-32767"], O.GAP_GOTOH)
