"""The both-strand model of the strand tests (a helper, not a test module): the definitions of
include/swbank.h "both DNA strands" restated in numpy, and the data500 facts the fixtures record.

    revcomp      the codes reversed, T <-> A (0 <-> 2), C <-> G (1 <-> 3); N stays N
    merge        max(forward, reverse); strand 1 only where the reverse score is strictly greater
    flip_record  what sw_align_strand_hits returns for a reverse hit, from what the forward call
                 returns for a batch holding rc(target): SW_ALIGN_REVERSE and the target
                 coordinates on the forward target, everything else as it is
"""
import dataclasses
import os

import numpy as np

from oracle import oracle as O

ALIGN_EMPTY, ALIGN_REVERSE = 1, 8
REF = (5, -4, -12, -4)
STRANDS_TSV = os.path.join(O.GOLDEN, "strands500.tsv")
STRAND_ALIGNMENTS_TSV = os.path.join(O.GOLDEN, "strand_alignments500.tsv")


def revcomp(codes):
    c = np.asarray(codes, np.uint8)[::-1]
    return np.where(c < 4, c ^ 2, c).astype(np.uint8)


def merge(fwd, rev):
    """(merged scores int32, strands uint8) of two score arrays of one shape."""
    fwd, rev = np.asarray(fwd, np.int32), np.asarray(rev, np.int32)
    return np.maximum(fwd, rev), (rev > fwd).astype(np.uint8)


def flip_record(a, target_len):
    """The strand call's record of a reverse hit from the forward call's record `a`
    (swbank.Alignment, or anything dataclasses.replace takes) of the batch holding rc(target)."""
    if a.score <= 0:
        return dataclasses.replace(a, flags=a.flags | ALIGN_REVERSE)
    return dataclasses.replace(a, flags=a.flags | ALIGN_REVERSE,
                               t_start=target_len - 1 - a.t_end,
                               t_end=target_len - 1 - a.t_start)


def flip_ends(ends, target_len):
    """brute_ends' (score, q_start, q_end, t_start, t_end) of rc(target) on the forward target."""
    s, qs, qe, ts, te = ends
    return ends if s <= 0 else (s, qs, qe, target_len - 1 - te, target_len - 1 - ts)


def data500():
    """(names, query, targets) of the reference's query100.fa x data500.fa, as codes."""
    recs = O.read_fasta(O.golden_fasta("data500.fa"))
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    return [n for n, _ in recs], q, [O.encode_dna(s) for _, s in recs]


def oracle_strands(q, seqs, pen=REF, model=O.GAP_MERGED):
    """(forward, reverse) oracle scores of q against the targets and their reverse complements."""
    sub = O.dna_matrix(pen[0], pen[1])
    fwd = O.score_batch(q, *O.pack_residues(seqs), sub, pen[2], pen[3], model)
    rev = O.score_batch(q, *O.pack_residues([revcomp(s) for s in seqs]), sub, pen[2], pen[3], model)
    return fwd, rev


def load_strands500():
    """[(name, forward, reverse, strand)] of tests/golden/strands500.tsv."""
    rows = [l.rstrip("\n").split("\t") for l in open(STRANDS_TSV)][1:]
    return [(r[0], int(r[1]), int(r[2]), int(r[3])) for r in rows]


def load_strand_alignments500():
    """[dict] of tests/golden/strand_alignments500.tsv (integers parsed)."""
    lines = [l.rstrip("\n").split("\t") for l in open(STRAND_ALIGNMENTS_TSV)]
    out = []
    for r in lines[1:]:
        d = dict(zip(lines[0], r))
        out.append({k: v if k in ("name", "cigar") else int(v) for k, v in d.items()})
    return out
