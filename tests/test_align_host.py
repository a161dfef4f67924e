"""Alignment checks that need no GPU: sw_cigar_string, and the CPU model of tests/align_check.py
against the two ssearch36 hits of the reference's data/alignments500.txt."""
import ctypes
import os

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_check as AC


def _cigar(ops, cap):
    a = np.asarray(ops, np.uint32)
    buf = ctypes.create_string_buffer(b"\xff" * max(cap, 1), max(cap, 1))
    need = S.lib().sw_cigar_string(a.ctypes.data_as(ctypes.c_void_p) if a.size else None, a.size,
                                   buf if cap else None, cap)
    return need, buf.raw


def test_cigar_string_round_trip_and_truncation():
    ops = AC.parse_cigar("15M2I17M4D13M")
    assert ops == (15 << 4 | 0, 2 << 4 | 1, 17 << 4 | 0, 4 << 4 | 2, 13 << 4 | 0)
    text = b"15M2I17M4D13M"
    need, raw = _cigar(ops, 64)
    assert need == len(text) and raw[:need + 1] == text + b"\0"
    assert raw[need + 1:] == b"\xff" * (64 - need - 1)       # nothing written past the NUL
    need, raw = _cigar(ops, len(text) + 1)                    # exactly fits
    assert need == len(text) and raw == text + b"\0"
    need, raw = _cigar(ops, 6)                                # truncated, still NUL-terminated
    assert need == len(text) and raw == b"15M2I\0"
    need, raw = _cigar(ops, 1)
    assert need == len(text) and raw == b"\0"
    assert _cigar(ops, 0)[0] == len(text)                     # length query, nothing written
    assert _cigar((), 4) == (0, b"\0\xff\xff\xff")
    big = ((1 << 28) - 1) << 4 | 2
    assert S.cigar_string([big, 14000 << 4]) == f"{(1 << 28) - 1}D14000M"
    assert AC.parse_cigar(S.cigar_string(ops)) == ops
    assert S.cigar_string([3 << 4 | 9]) == "3?"


def test_header_announces_alignments():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "swbank.h")).read()
    assert "#define SWBANK_HAS_ALIGN 1" in txt and "#define SWBANK_ABI_VERSION 6" in txt
    assert ctypes.sizeof(S.AlignmentRecord) == S.ALIGNMENT_DTYPE.itemsize == 56


@pytest.mark.parametrize("model", [O.GAP_MERGED, O.GAP_GOTOH])
def test_model_reproduces_the_ssearch36_rows(model):
    """Score, 0-based coordinates, columns, identities and CIGAR of db211 and db428
    (tests/golden/alignments500.tsv, from the reference's report), and the report's own summary
    lines rebuilt from them."""
    recs = dict(O.read_fasta(O.golden_fasta("data500.fa")))
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    rows = [ln.rstrip("\n").split("\t")
            for ln in open(os.path.join(O.GOLDEN, "alignments500.tsv"))][1:]
    lines = open(os.path.join(O.GOLDEN, "alignments500_lines.txt")).read().splitlines()
    assert len(rows) == len(lines) == 2
    sub = O.dna_matrix()
    for row, line in zip(rows, lines):
        t = O.encode_dna(recs[row[0]])
        score, qs, qe, ts, te, cols, idn = (int(x) for x in row[1:8])
        assert AC.brute_ends(O, q, t, sub, -12, -4, model) == (score, qs, qe, ts, te)
        ops = AC.parse_cigar(row[8])
        assert AC.rescore(ops, q, t, qs, ts, sub, -12, -4, model) == \
            (score, qe - qs + 1, te - ts + 1, cols, idn)
        a = S.Alignment(0, 0, score, 0, qs, qe, ts, te, cols, idn, ops, row[8])
        AC.check_alignment(O, q, t, sub, -12, -4, model, a)
        assert line == (f"Smith-Waterman score: {score}; {100.0 * idn / cols:.1f}% identity "
                        f"({100.0 * idn / cols:.1f}% similar) in {cols} nt overlap "
                        f"({qs + 1}-{qe + 1}:{ts + 1}-{te + 1})")


def test_model_tie_rules_and_rejections():
    enc, sub = O.encode_dna, O.dna_matrix()
    for model in (O.GAP_MERGED, O.GAP_GOTOH):
        assert AC.brute_ends(O, enc("ACGT"), enc("ACGTTTTTACGT"), sub, -12, -4, model) == \
            (20, 0, 3, 0, 3)
        assert AC.brute_ends(O, enc("ACGTNNACGT"), enc("ACGT"), sub, -12, -4, model) == \
            (20, 0, 3, 0, 3)
        assert AC.brute_ends(O, enc("AAAA"), enc("CCCC"), sub, -12, -4, model) == (0,) * 5
    # a corner-turning gap is one run under the merged model, two under Gotoh
    q, t = enc("ACGTAAACGT"), enc("ACGTCCACGT")
    ops = AC.parse_cigar("4M2I2D4M")
    assert AC.rescore(ops, q, t, 0, 0, sub, -10, -1, O.GAP_MERGED)[0] == 40 - 10 - 4
    assert AC.rescore(ops, q, t, 0, 0, sub, -10, -1, O.GAP_GOTOH)[0] == 40 - 20 - 4
    bad = S.Alignment(0, 0, 20, 0, 0, 3, 0, 3, 4, 4, AC.parse_cigar("3M"), "3M")
    with pytest.raises(AssertionError):
        AC.check_alignment(O, enc("ACGT"), enc("ACGT"), sub, -12, -4, O.GAP_MERGED, bad)
