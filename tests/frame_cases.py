"""The translated-search model of the frame tests (a helper, not a test module): the definitions
of include/swbank.h "translated search" restated in numpy.

    translate     frame f (0..2 forward, 3..5 those of rc(target)) of DNA codes as protein codes:
                  table[c0 * 16 + c1 * 4 + c2] over T, C, A, G = 0..3; a codon holding a code of 4
                  or more is X; a stop is * and stays in the frame
    merge6        max over the six frames; the lowest frame that reaches it
    nt_coords     the nucleotide range, on the forward target, of amino positions a_start..a_end
                  of frame f of a target of L codes
    frame_record  what sw_align_frame_hits returns for a hit, from what sw_align_set_hits returns
                  for a batch holding the translation of the hit's frame
"""
import dataclasses

import numpy as np

from oracle import oracle as O

import strand_cases as SC

STANDARD_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
ALIGN_EMPTY, ALIGN_NO_PATH, ALIGN_NO_HIT, ALIGN_REVERSE = 1, 2, 4, 8
ALIGN_FRAME_SHIFT, ALIGN_FRAME_MASK = 4, 0x30
X, STOP = O.PROT_LETTERS.index("X"), O.PROT_LETTERS.index("*")
TAGS = ("+1", "+2", "+3", "-1", "-2", "-3")
PEN = (-11, -1)  # BLOSUM62's usual gap penalties


def standard_table():
    return O.encode_protein(STANDARD_CODE)


def custom_table():
    """A code that differs from the standard one in every entry (each amino acid's code + 1,
    modulo the alphabet): a kernel that ignored the caller's table could not pass."""
    return ((standard_table().astype(np.int64) + 1) % O.PROT_ALPHA).astype(np.uint8)


def frame_len(L, f):
    o = f % 3
    return (L - o) // 3 if L >= o + 3 else 0


def translate(codes, f, table=None):
    c = np.asarray(codes, np.uint8)
    tab = standard_table() if table is None else np.asarray(table, np.uint8)
    assert 0 <= f < 6 and tab.shape == (64,)
    if f >= 3:
        c = SC.revcomp(c)
    n = frame_len(len(c), f)
    cod = c[f % 3:f % 3 + 3 * n].astype(np.int64).reshape(n, 3)
    ok = (cod < 4).all(axis=1)
    idx = np.where(ok, cod[:, 0] * 16 + cod[:, 1] * 4 + cod[:, 2], 0)
    return np.where(ok, tab[idx], X).astype(np.uint8)


def merge6(scores):
    """(merged int32, frames uint8) of scores[6, ...]: a tie goes to the lowest frame."""
    s = np.asarray(scores, np.int32)
    assert s.shape[0] == 6
    return s.max(axis=0), s.argmax(axis=0).astype(np.uint8)


def nt_coords(a_start, a_end, f, L):
    o = f % 3
    fs, fe = o + 3 * a_start, o + 3 * a_end + 2
    return (fs, fe) if f < 3 else (L - 1 - fe, L - 1 - fs)


def frame_flags(f):
    return ((f % 3) << ALIGN_FRAME_SHIFT) | (ALIGN_REVERSE if f >= 3 else 0)


def frame_of(flags):
    return ((flags & ALIGN_FRAME_MASK) >> ALIGN_FRAME_SHIFT) + (3 if flags & ALIGN_REVERSE else 0)


def frame_record(a, f, L, index, ident):
    """The frame call's record from the set call's record `a` (swbank.Alignment) of the batch
    holding the translation of frame f of the target at `index`, L codes long."""
    if a.flags & ALIGN_NO_HIT:
        return a
    a = dataclasses.replace(a, index=index, id=ident, flags=a.flags | frame_flags(f))
    if a.score <= 0:
        return a
    ts, te = nt_coords(a.t_start, a.t_end, f, L)
    return dataclasses.replace(a, t_start=ts, t_end=te)


def back_translate(rng, aa, table=None):
    """DNA codes of a random choice among each amino acid's codons."""
    tab = standard_table() if table is None else np.asarray(table, np.uint8)
    out = []
    for a in aa:
        c = int(rng.choice(np.nonzero(tab == a)[0]))
        out += [c >> 4, (c >> 2) & 3, c & 3]
    return np.array(out, np.uint8)


def plant(rng, q, L, o, reverse, table=None):
    """A random target of L codes with the back-translation of protein q at a position p with
    p % 3 == o, reverse-complemented when `reverse`: (target, planted frame)."""
    core = back_translate(rng, q, table)
    slots = (L - len(core) - o) // 3
    assert slots >= 0
    p = o + 3 * int(rng.integers(0, slots + 1))
    t = rng.integers(0, 4, L).astype(np.uint8)
    t[p:p + len(core)] = core
    return (SC.revcomp(t), 3 + o) if reverse else (t, o)


def self_score(q, sub=O.BLOSUM62):
    return int(sum(int(sub[a][a]) for a in q))


def oracle_frames(q, seqs, sub=O.BLOSUM62, pen=PEN, model=O.GAP_GOTOH, table=None):
    """scores[6, n] of protein q against the model's translations of every target."""
    return np.stack([O.score_batch(q, *O.pack_residues([translate(s, f, table) for s in seqs]),
                                   sub, pen[0], pen[1], model) for f in range(6)])


def want_frames(qs, seqs, model=O.GAP_GOTOH, table=None):
    """(merged [nq, n], frames [nq, n], per-frame [nq, 6, n]) by the oracle."""
    per = np.stack([oracle_frames(q, seqs, model=model, table=table) for q in qs])
    merged = [merge6(p) for p in per]
    return np.stack([m[0] for m in merged]), np.stack([m[1] for m in merged]), per


def search_case(seed=71, n=200, qlens=(17, 130, 60)):
    """Protein queries and n DNA targets of 0..400 codes: random ones (N codes among them),
    empty and codon-less ones, and plants of every query at every offset on both strands."""
    rng = np.random.default_rng(seed)
    qs = [rng.integers(0, 20, m).astype(np.uint8) for m in qlens]
    seqs, planted = [], {}
    for k in range(n):
        L = int(rng.integers(0, 401))
        i = k % len(qs)
        if k % 4 == 1:  # (k // 4 walks through query x offset x strand)
            L = int(rng.integers(3 * len(qs[i]) + 2, 401))
            t, f = plant(rng, qs[i], L, (k // 12) % 3, (k // 36) % 2 == 1)
            planted[k] = (i, f)
        else:
            t = rng.integers(0, 5 if k % 5 == 0 else 4, L).astype(np.uint8)
        seqs.append(t)
    for k, L in zip((0, 2, 3, 6), (0, 1, 2, 4)):
        seqs[k] = seqs[k][:L] if len(seqs[k]) >= L else rng.integers(0, 4, L).astype(np.uint8)
        planted.pop(k, None)
    return qs, seqs, planted
