"""The model of the non-intersecting alignments over reading frames (tests/disjoint_frames_cases.py)
on the CPU: the plain-Python composition equals the C composition on tiny pairs, and the three
properties that follow from the definition hold on every record -- record 0 has the score and the
frame of the six-frame search, scores never increase, two records of a frame share no cell.  The
planted cases say what the GPU tests rely on.  And, without a device, the header carries the macro
and the two new entries are exported and refuse a NULL bank."""
import ctypes
import os
import re
import subprocess

import numpy as np

import swbank as S
from oracle import oracle as O

import disjoint_cases as D
import disjoint_frames_cases as DF
import frame_cases as FR

ROUNDS = 4


def test_python_and_c_compositions_agree_on_tiny_pairs():
    cases = DF.tiny_cases()
    assert len(cases) >= 300 and {len(c[1]) for c in cases} >= set(range(6))
    assert max(len(c[0]) for c in cases) <= 9 and max(len(c[1]) for c in cases) <= 33
    assert {c[5] is None for c in cases} == {True, False}
    depth, frames_seen, second_frame = set(), set(), 0
    for k, (q, t, sub, go, ge, table) in enumerate(cases):
        min_score = 1 + k % 3
        want = DF.py_merged(q, t, sub, go, ge, ROUNDS, min_score, table)
        got = DF.c_merged(q, t, sub, go, ge, ROUNDS, min_score, table)
        assert got == want, (k, q, t, go, ge)
        DF.check_anchors(q, t, sub, go, ge, got, min_score, table)
        fr = DF.frames(got)
        depth.add(len(fr))
        frames_seen |= set(fr)
        second_frame += len(set(fr)) > 1
        if len(t) < 3:
            assert got == [D.EMPTY_REC] * ROUNDS
    assert {0, 1, ROUNDS} <= depth and frames_seen == set(range(6))
    assert second_frame >= len(cases) // 4  # the merge has something to merge


def test_exons_in_three_frames_come_first():
    """Thirds of a protein in frames of two offsets and on the reverse strand: the first three
    records are the three thirds in three different frames, one of them reversed."""
    for m in (60, 300, 600):
        q, t = DF.exon_case(m)
        recs = DF.c_merged(q, t, O.BLOSUM62, *DF.PEN, 5, 20)
        fr = DF.frames(recs)
        assert len(fr) >= 3 and len(set(fr[:3])) == 3 and max(fr[:3]) >= 3, (m, fr)
        rows = sorted((rec[2], rec[3]) for rec, _ in recs[:3])
        assert all(b - a >= m // 3 - 4 for a, b in rows) and rows[0][0] <= 2 and rows[2][1] >= m - 3
        DF.check_anchors(q, t, O.BLOSUM62, *DF.PEN, recs, 20)


def test_ties_across_strands_and_a_frame_that_wins_twice():
    q, t = DF.tie_case()
    recs = DF.c_merged(q, t, O.BLOSUM62, *DF.PEN, 3, 20)
    assert recs[0][0][0] == recs[1][0][0] == FR.self_score(q)
    fr = DF.frames(recs)
    assert fr[0] < 3 <= fr[1]  # the lower frame first
    q, t = DF.twice_case()
    recs = DF.c_merged(q, t, O.BLOSUM62, *DF.PEN, 3, 20)
    fr = DF.frames(recs)
    assert fr[0] == fr[1] and recs[0][0][0] == recs[1][0][0] == FR.self_score(q)
    assert recs[0][0][4] < recs[1][0][4]  # the smaller t_end is found first
    DF.check_anchors(q, t, O.BLOSUM62, *DF.PEN, recs, 20)


def test_seam_targets_depend_on_the_codon_table():
    tab = FR.custom_table()
    q, seqs = DF.seam_cases(tab)
    assert {len(t) for t in seqs} >= set(range(7)) | {3 * b + d for b in (64, 128)
                                                       for d in range(-1, 4)}
    differ = 0
    for t in seqs:
        a = DF.c_merged(q, t, O.BLOSUM62, *DF.PEN, 3, 20, tab)
        DF.check_anchors(q, t, O.BLOSUM62, *DF.PEN, a, 20, tab)
        differ += a != DF.c_merged(q, t, O.BLOSUM62, *DF.PEN, 3, 20)
    assert 2 * differ > len(seqs)


def test_header_carries_the_macro():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "swbank.h")) as f:
        txt = f.read()
    assert re.search(r"#define\s+SWBANK_HAS_DISJOINT_FRAMES\s+1\b", txt)
    for name in ("sw_align_disjoint_frame_hits", "sw_align_disjoint_frame_hits_device"):
        assert re.search(r"sw_status\s+" + name + r"\s*\(", txt), name


def test_entries_are_exported_and_refuse_a_null_bank():
    out = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"sw_align_disjoint_frame_hits", "sw_align_disjoint_frame_hits_device"} <= syms
    L = S.lib()
    res, offs, lens = S.pack_targets([np.zeros(9, np.uint8)])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rec = np.full(2 * S.ALIGNMENT_DTYPE.itemsize, 0x3C, np.uint8)
    used = ctypes.c_size_t(7)
    assert L.sw_align_disjoint_frame_hits(None, p(res), res.size, p(offs), p(lens), None, 1, None,
                                          2, 1, None, 1, None, 1, p(rec), None, 0,
                                          ctypes.byref(used)) == S.ERR_ARG
    assert L.sw_align_disjoint_frame_hits_device(None, p(res), p(offs), p(lens), None, 1, 9, None,
                                                 2, 1, None, 1, None, 1, p(rec), None, 0,
                                                 None) == S.ERR_ARG
    assert (rec == 0x3C).all() and used.value == 7
