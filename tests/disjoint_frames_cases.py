"""The model of the non-intersecting alignments over the six reading frames of a hit (a helper, not
a test module): the definition of include/swbank.h "non-intersecting alignments over reading
frames" composed from the models the project already has, and the cases the CPU and GPU tests
share.

    py_merged     frame_cases.translate + disjoint_cases.py_rounds on each of the six translations,
                  merged: what the C composition is checked against
    c_merged      the same with disjoint_cases.c_rounds: what the GPU tests compare against at size
    aa_record     a merged record back in the amino-acid columns of its frame (for disjoint_cases.
                  cells)
    tiny_cases    seeded random pairs of at most 9 rows and 33 nucleotides
    exon_case     a protein whose thirds lie in three frames of one target, one of them reversed
    tie_case      a peptide on both strands of one target
    twice_case    two back-translations of a peptide in one frame
    seam_cases    targets of a few codes and around 64 and 128 codons, plants across codon 63 | 64

A record is disjoint_cases' tuple (score, flags, q_start, q_end, t_start, t_end, n_columns,
n_identities) with the frame in the flags and t_start / t_end in nucleotides on the forward target.
The merge: at each step the head with the largest score among the six sequences, a tie to the
lowest frame; when every head is empty, the slot and every later one is empty, with no frame bits.
"""
import numpy as np

from oracle import oracle as O

import disjoint_cases as D
import frame_cases as FR
import strand_cases as SC

PEN = FR.PEN


def _merged(rounds_of, q, t, sub, go, ge, rounds, min_score, table, **kw):
    t = np.asarray(t, np.uint8)
    L = len(t)
    per = [rounds_of(q, FR.translate(t, f, table), sub, go, ge, rounds, min_score, **kw)
           for f in range(6)]
    head, out = [0] * 6, []
    for _ in range(rounds):
        best, bf = 0, None
        for f in range(6):
            if head[f] < rounds:
                rec = per[f][head[f]][0]
                if not rec[1] & D.EMPTY and rec[0] > best:   # strictly: the lowest frame stays
                    best, bf = rec[0], f
        if bf is None:
            out.append(D.EMPTY_REC)
            continue
        rec, ops = per[bf][head[bf]]
        head[bf] += 1
        ts, te = FR.nt_coords(rec[4], rec[5], bf, L)
        out.append(((rec[0], rec[1] | FR.frame_flags(bf), rec[2], rec[3], ts, te, rec[6], rec[7]),
                    tuple(ops)))
    return out


def py_merged(q, t, sub, go, ge, rounds, min_score=1, table=None):
    return _merged(D.py_rounds, q, t, sub, go, ge, rounds, min_score, table)


def c_merged(q, t, sub, go, ge, rounds, min_score=1, table=None, cap=None):
    """cap: the ops a slot holds (more: no path, the cells used all the same)."""
    return _merged(D.c_rounds, q, t, sub, go, ge, rounds, min_score, table, cap=cap)


def frames(recs):
    """The frames of the non-empty records of a hit, in order."""
    return [FR.frame_of(rec[1]) for rec, _ in recs if not rec[1] & D.EMPTY]


def aa_record(rec, L):
    """The record with t_start / t_end as columns of its frame's translation."""
    f = FR.frame_of(rec[1])
    o = f % 3
    fs, fe = (rec[4], rec[5]) if f < 3 else (L - 1 - rec[5], L - 1 - rec[4])
    assert (fs - o) % 3 == 0 and (fe - 2 - o) % 3 == 0
    return rec[:4] + ((fs - o) // 3, (fe - 2 - o) // 3) + rec[6:]


def check_anchors(q, t, sub, go, ge, recs, min_score, table=None):
    """The three properties that follow from the definition, on the records of one hit."""
    per = FR.oracle_frames(q, [t], sub, (go, ge), table=table)[:, 0]
    best, frame = int(per.max()), int(per.argmax())
    rec0 = recs[0][0]
    if best >= min_score:
        assert (rec0[0], FR.frame_of(rec0[1])) == (best, frame), (rec0, per)
    else:
        assert recs[0] == D.EMPTY_REC
    sc = D.scores(recs)
    assert all(a >= b for a, b in zip(sc, sc[1:])), sc
    seen = {}
    for rec, ops in recs:
        if rec[1] & D.EMPTY:
            assert (rec, ops) == D.EMPTY_REC
            continue
        assert rec[0] >= min_score
        if rec[1] & D.NO_PATH:
            continue
        cells = set(D.cells(aa_record(rec, len(t)), ops))
        f = FR.frame_of(rec[1])
        assert not seen.get(f, set()) & cells, (f, rec)
        seen[f] = seen.get(f, set()) | cells


# ---- cases ---------------------------------------------------------------------------------------
def tiny_cases(count=300, seed=7):
    """[(q, t, sub, go, ge, table)]: m <= 9 rows over a few amino acids, L <= 33 nucleotides (L =
    0..5 among them, N now and then), BLOSUM62 or a random asymmetric matrix, the penalty pairs of
    disjoint_cases.tiny_pairs, the standard and the custom codon table."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        go, ge = [(0, 0), (0, -3), (-8, 0), (-12, -4), (-100, -10), (-1, -1)][k % 6]
        sub = np.asarray(O.BLOSUM62, np.int8)
        if rng.integers(0, 2):
            sub = rng.integers(-6, 7, (O.PROT_ALPHA, O.PROT_ALPHA)).astype(np.int8)
        m = int(rng.integers(1, 10))
        L = k % 50 if k % 50 < 6 else int(rng.integers(6, 34))
        table = FR.custom_table() if (k // 6) % 2 else None
        letters = (2, 4)[int(rng.integers(0, 2))]   # few nucleotides: repeats, so several rounds
        t = rng.integers(0, letters, L).astype(np.uint8)
        if k % 11 == 3 and L:
            t[int(rng.integers(0, L))] = 4
        # the query from the target's own frames, so that pairs align at all
        pool = np.concatenate([FR.translate(t, f, table) for f in range(6)] + [np.arange(4)])
        q = rng.choice(pool, m).astype(np.uint8)
        out.append((q, t, sub, go, ge, table))
    return out


def _spacer(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def exon_case(m, seed=5, table=None):
    """(q, t): thirds of a protein of m residues back-translated at offsets 0 and 2 mod 3 and, the
    last third, reverse-complemented, between random spacers."""
    rng = np.random.default_rng([503, m, seed])
    q = rng.integers(0, 20, m).astype(np.uint8)
    a, b = m // 3, 2 * m // 3
    parts = [_spacer(rng, 9), FR.back_translate(rng, q[:a], table)]
    at = sum(len(p) for p in parts)
    parts.append(_spacer(rng, 12 + (2 - (at + 12)) % 3))          # the second third at 2 mod 3
    parts.append(FR.back_translate(rng, q[a:b], table))
    parts.append(_spacer(rng, 17))
    parts.append(SC.revcomp(FR.back_translate(rng, q[b:], table)))
    parts.append(_spacer(rng, 8))
    t = np.concatenate(parts).astype(np.uint8)
    assert sum(len(p) for p in parts[:3]) % 3 == 2
    return q, t


def tie_case(seed=5):
    """(q, t): a 40-residue peptide's back-translation and its reverse complement between N."""
    rng = np.random.default_rng([509, seed])
    q = rng.integers(0, 20, 40).astype(np.uint8)
    core = FR.back_translate(rng, q)
    N = lambda n: np.full(n, 4, np.uint8)  # noqa: E731
    return q, np.concatenate([N(6), core, N(9), SC.revcomp(core), N(6)]).astype(np.uint8)


def twice_case(seed=5):
    """(q, t): two independent back-translations of a 40-residue peptide in one frame."""
    rng = np.random.default_rng([521, seed])
    q = rng.integers(0, 20, 40).astype(np.uint8)
    N = lambda n: np.full(n, 4, np.uint8)  # noqa: E731
    return q, np.concatenate([N(3), FR.back_translate(rng, q), N(12), FR.back_translate(rng, q),
                              N(6)]).astype(np.uint8)


def indel_case(seed=5):
    """(q, t): 90 residues; the first 45 with a codon deleted in frame 0 (three ops), residues
    45..59 in frame 1 and the last 30 on the reverse strand (one op each)."""
    rng = np.random.default_rng([541, seed])
    q = rng.integers(0, 20, 90).astype(np.uint8)
    N = lambda n: np.full(n, 4, np.uint8)  # noqa: E731
    first = FR.back_translate(rng, np.delete(q[:45], 20))
    t = np.concatenate([N(3), first, N(10), FR.back_translate(rng, q[45:60]), N(8),
                        SC.revcomp(FR.back_translate(rng, q[60:])), N(5)]).astype(np.uint8)
    assert (3 + len(first) + 10) % 3 == 1
    return q, t


def seam_cases(table=None, seed=5):
    """(q, [t]): a 30-residue protein against targets of 0..6 codes and of 3 x 64 + d, d = -1..3,
    and 3 x 128 + d codes: random ones, ones where the protein straddles codon 63 | 64 of a forward
    and of a reverse frame, and ones with an N inside a planted codon."""
    rng = np.random.default_rng([523, seed])
    q = rng.integers(0, 20, 30).astype(np.uint8)
    seqs = [_spacer(rng, L) for L in range(7)]
    seqs[3] = FR.back_translate(rng, q[:1], table)
    seqs[6] = FR.back_translate(rng, q[:2], table)
    for base in (64, 128):
        for d in range(-1, 4):
            L = 3 * base + d
            for kind in range(3):
                t = _spacer(rng, L)
                o = (d + kind) % 3
                # codons 49 .. 78 of frame o, across 63 | 64; a short target: its last 30 codons
                p = o + 3 * (49 if base == 128 else FR.frame_len(L, o) - 30)
                t[p:p + 90] = FR.back_translate(rng, q, table)
                if kind == 1:                       # the same columns of a reverse frame
                    t = SC.revcomp(t)
                if kind == 2:
                    t[p + 3 * 14 + 1] = 4           # N inside codon 63 of the plant
                    t[5] = 4
                seqs.append(t)
    return q, seqs
