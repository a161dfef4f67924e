#!/usr/bin/env python3
"""Regenerate the both-strand fixtures under tests/golden/ from the oracle (oracle/) and the
reference traceback of tests/align_cases.py, on the reference's query100.fa x data500.fa at its
penalties 5 / -4 / -12 / -4 (merged gaps; the Gotoh figures are the same, which
tests/test_strand_cases.py checks against the oracle):

    python tests/golden/make_strands.py

* ``strands500.tsv``            name, forward score, reverse-strand score, strand (1: the reverse
                                score is strictly greater) of every target.
* ``strand_alignments500.tsv``  the reverse-strand hits among the six best of both strands, field
                                for field as sw_align_strand_hits reports them (target coordinates
                                on the forward target).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.dirname(HERE)]

import numpy as np  # noqa: E402

from oracle import oracle as O  # noqa: E402

import align_cases as C  # noqa: E402
import align_check as AC  # noqa: E402
import strand_cases as SC  # noqa: E402

FIELDS = ("name", "index", "length", "score", "q_start", "q_end", "t_start", "t_end", "n_columns",
          "n_identities", "cigar")


def main():
    names, q, seqs = SC.data500()
    fwd, rev = SC.oracle_strands(q, seqs)
    best, strand = SC.merge(fwd, rev)
    with open(SC.STRANDS_TSV, "w") as f:
        f.write("name\tforward\treverse\tstrand\n")
        for row in zip(names, fwd, rev, strand):
            f.write("\t".join(str(x) for x in row) + "\n")
    sub = O.dna_matrix(SC.REF[0], SC.REF[1])
    order = np.argsort(-best.astype(np.int64), kind="stable")[:6]
    with open(SC.STRAND_ALIGNMENTS_TSV, "w") as f:
        f.write("\t".join(FIELDS) + "\n")
        for k in order:
            if not strand[k]:
                continue
            t = SC.revcomp(seqs[k])
            ends = AC.brute_ends(O, q, t, sub, SC.REF[2], SC.REF[3], O.GAP_MERGED)
            ref = C.ref_path(q, t, sub, SC.REF[2], SC.REF[3], O.GAP_MERGED, ends)
            s, qs, qe, ts, te = SC.flip_ends(ends, len(t))
            text = "".join(f"{op >> 4}{'MID'[op & 15]}" for op in ref.ops)
            f.write("\t".join(str(x) for x in (names[k], k, len(t), s, qs, qe, ts, te,
                                               ref.n_columns, ref.n_identities, text)) + "\n")


if __name__ == "__main__":
    main()
