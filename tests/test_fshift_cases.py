"""The model of the frameshift-tolerant translated search on the CPU (tests/fshift_cases.py): the
C model against the plain-Python restatement of the definition, the six-frame anchor at
fs = -32767, planted single-base insertions and deletions, and the strand tie."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fshift_cases as FS
import matrix_cases as MC
import seam_cases as SEAMS
import strand_cases as SC


def test_the_library_publishes_the_call():
    """The header's names reach Python: the feature exists."""
    assert S.FSHIFT_MAX_QUERY >= 1024
    assert hasattr(S.ScoreBank, "score_frameshift") and hasattr(S.ScoreBank, "score_frameshift_device")
    assert hasattr(S.lib(), "sw_score_fshift") and hasattr(S.lib(), "sw_score_fshift_device")


@pytest.mark.parametrize("table", ["standard", "custom"])
def test_c_model_equals_the_python_restatement(table):
    """100 random pairs per table: m <= 12, L <= 40, N codes in every fourth target, BLOSUM62 and
    the asymmetric matrix, every fs of FS_VALUES."""
    tab = F.custom_table() if table == "custom" else None
    rng = np.random.default_rng([101, table == "custom"])
    asym = SEAMS.MATRICES[MC.PROTEIN]()
    for k in range(100):
        m, L = int(rng.integers(1, 13)), int(rng.integers(0, 41))
        q = rng.integers(0, 24 if k % 5 == 0 else 20, m).astype(np.uint8)
        t = rng.integers(0, 5 if k % 4 == 0 else 4, L).astype(np.uint8)
        if k % 3 == 0 and k % 5 and L >= 3 * m + 1:  # a planted shift: the links are alive
            core = F.back_translate(rng, q, tab)
            t[:len(core) + 1] = np.insert(core, 3 * (m // 2), 1)
        sub = asym if k % 2 else O.BLOSUM62
        fs = FS.FS_VALUES[k % 4]
        want = FS.py_search(q, t, sub, *F.PEN, fs, tab)
        sc, sd = FS.c_search(q, [t], sub, *F.PEN, fs, tab)
        assert (int(sc[0]), int(sd[0])) == want, (k, m, L, fs)


def test_six_frame_anchor_on_the_search_case():
    """fs = -32767 can never win: the model equals merge6 of the oracle's six frame scores and the
    strand is (frame >= 3), on frame_cases.search_case and on targets of 0..9 codes."""
    qs, seqs, planted = F.search_case()
    rng = np.random.default_rng(103)
    tiny = [rng.integers(0, 4, L).astype(np.uint8) for L in range(10)]
    for i, q in enumerate(qs):
        for batch in (seqs, tiny):
            want_sc, want_sd = FS.six_frames(q, batch)
            sc, sd = FS.c_search(q, batch, O.BLOSUM62, *F.PEN, -32767)
            assert np.array_equal(sc, want_sc) and np.array_equal(sd, want_sd)
    for L in range(10):
        got = FS.py_search(qs[0], tiny[L], O.BLOSUM62, *F.PEN, -32767)
        want_sc, want_sd = FS.six_frames(qs[0], [tiny[L]])
        assert got == (int(want_sc[0]), int(want_sd[0]))


def test_planted_shifts_beat_six_frames():
    """Query A + B against bt(A) + one base + bt(B) (or bt(A) + bt(B)[1:]) on either strand at
    fs = -15: at least both halves and one shift, more than the six-frame search, on the planted
    strand."""
    for kind, rev, q, t, A, B in FS.shift_cases():
        sc, sd = FS.c_search(q, [t], O.BLOSUM62, *F.PEN, FS.SHIFT_FS)
        six, _ = FS.six_frames(q, [t])
        assert int(sc[0]) >= FS.shift_bound(kind, A, B, FS.SHIFT_FS), (kind, rev)
        assert int(sc[0]) > int(six[0]), (kind, rev)
        assert int(sd[0]) == int(rev), (kind, rev)


def test_strand_tie_goes_forward():
    """A target equal to its own reverse complement scores the same on both strands: strand 0."""
    rng = np.random.default_rng(107)
    q = rng.integers(0, 20, 15).astype(np.uint8)
    half = F.back_translate(rng, q)
    t = np.concatenate([half, SC.revcomp(half)])
    assert np.array_equal(SC.revcomp(t), t)
    for fs in FS.FS_VALUES:
        sc, sd = FS.c_search(q, [t], O.BLOSUM62, *F.PEN, fs)
        assert int(sc[0]) >= F.self_score(q) and int(sd[0]) == 0
        assert FS.py_search(q, t, O.BLOSUM62, *F.PEN, fs) == (int(sc[0]), 0)
