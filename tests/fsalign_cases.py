"""The model of the alignments of frameshift hits (a helper, not a test module): the contract of
include/swbank.h "alignments of frameshift hits" restated twice.

    py_align     plain Python over dictionaries of cells: the end cell, a brute-force start (the
                 anchored matrix from every candidate start cell), the anchored walk over the
                 matrices' values (no direction bytes), the record
    rescore      what a list of ops scores and consumes, with no preference in it
    c_align      tests/c/fsalign_model.c, compiled with the host compiler on first use and loaded
                 with ctypes: the reversed local pass for the start, direction bytes for the walk;
                 what the GPU tests compare against at size
    c_mutant     the C model with the gap state of one pass dropped at a seam: what keeps the
                 targets of seam_family live
    tiny_cases   the tie-rich pairs on which the two restatements are compared
    seam_family  per pass an I run across a lane seam and a D run across a 64-codon block seam

A record is (score, flags, q_start, q_end, t_start, t_end, n_columns, n_identities) and a tuple
of ops.  Everything else (translation, the tables, the matrices, the planted shifts) is
frame_cases' and fshift_cases'.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import frame_cases as F
import fshift_cases as FS
import strand_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
NEG = -(1 << 60)
OP_M, OP_I, OP_D, OP_SKIP, OP_BACK = 0, 1, 2, 3, 4
OP_TEXT = "MID/\\"
EMPTY = ((0, F.ALIGN_EMPTY, 0, 0, 0, 0, 0, 0), ())


def aminos(c, table=None):
    """a(p) for the codon starts p = 0 .. L - 3 of the strand c."""
    tab = F.standard_table() if table is None else np.asarray(table, np.uint8)
    c = [int(x) for x in c]
    return [int(tab[c[p] * 16 + c[p + 1] * 4 + c[p + 2]]) if max(c[p:p + 3]) < 4 else F.X
            for p in range(len(c) - 2)]


def cigar_text(ops):
    return "".join(f"{op >> 4}{OP_TEXT[op & 15]}" for op in ops)


# ---- the plain-Python restatement --------------------------------------------------------------
def _matrices(q, a, sub, o, e, fs, anchor):
    """M, E, F, H over rows q and columns a.  anchor False: the local matrix of the definition.
    anchor True: no floor, nothing outside, a 0 diagonal at cell (0, 0) only."""
    out = NEG if anchor else 0
    M, E, Fg, H = {}, {}, {}, {}

    def h(i, p):
        return H.get((i, p), out)

    for i in range(len(q)):
        for p in range(len(a)):
            links = [h(i - 1, p - 3), h(i - 1, p - 2) + fs, h(i - 1, p - 4) + fs]
            if anchor:
                via = 0 if (i, p) == (0, 0) else max(links)
            else:
                via = max([0] + links)
            M[i, p] = int(sub[q[i]][a[p]]) + via
            E[i, p] = max(h(i, p - 3) + o, E.get((i, p - 3), NEG) + e)
            Fg[i, p] = max(h(i - 1, p) + o, Fg.get((i - 1, p), NEG) + e)
            H[i, p] = max(M[i, p], E[i, p], Fg[i, p]) if anchor else \
                max(0, M[i, p], E[i, p], Fg[i, p])
    return M, E, Fg, H


def py_end(q, a, sub, o, e, fs):
    """(score, i_end, p_end): among the cells with H = score the smallest p, then the smallest i."""
    H = _matrices(q, a, sub, o, e, fs, False)[3]
    score = max(H.values(), default=0)
    if score <= 0:
        return 0, 0, 0
    p, i = min((p, i) for (i, p), v in H.items() if v == score)
    return score, i, p


def py_start(q, a, sub, o, e, fs, score, ie, pe):
    """Brute force: the largest p, then the largest i among the cells from which an anchored
    alignment reaches the end cell, as an M cell, with the score."""
    best = None
    for i0 in range(ie + 1):
        for p0 in range(pe + 1):
            M = _matrices(q[i0:ie + 1], a[p0:pe + 1], sub, o, e, fs, True)[0]
            if M[ie - i0, pe - p0] == score and (best is None or (p0, i0) > best):
                best = (p0, i0)
    return best[1], best[0]


def py_walk(q, a, sub, o, e, fs):
    """The ops of the preferred path over the anchored matrix of the window (rows q, columns a),
    first to last, from the matrices' values; the value at the end cell."""
    M, E, Fg, H = _matrices(q, a, sub, o, e, fs, True)
    i, p, state, back = len(q) - 1, len(a) - 1, "M", []
    for _ in range(len(q) + len(a) + 3):
        if state == "H":  # M, then E, then F
            state = "M" if H[i, p] == M[i, p] else "E" if H[i, p] == E[i, p] else "F"
        if state == "M":
            back.append(OP_M)
            if (i, p) == (0, 0):
                break
            via = M[i, p] - int(sub[q[i]][a[p]])
            if via == H.get((i - 1, p - 3), NEG):  # in frame, then p - 2, then p - 4
                p -= 3
            elif via == H.get((i - 1, p - 2), NEG) + fs:
                back.append(OP_BACK)
                p -= 2
            else:
                assert via == H.get((i - 1, p - 4), NEG) + fs
                back.append(OP_SKIP)
                p -= 4
            i, state = i - 1, "H"
        elif state == "E":  # a run opens rather than extends
            back.append(OP_D)
            state = "H" if E[i, p] == H.get((i, p - 3), NEG) + o else "E"
            p -= 3
        else:
            back.append(OP_I)
            state = "H" if Fg[i, p] == H.get((i - 1, p), NEG) + o else "F"
            i -= 1
    else:
        raise AssertionError("the walk did not reach the start cell")
    ops = []
    for code in reversed(back):
        if ops and ops[-1] & 15 == code and code < OP_SKIP:
            ops[-1] += 16
        else:
            ops.append(16 | code)
    return tuple(ops), M[len(q) - 1, len(a) - 1]


def rescore(ops, q, a, i0, p0, sub, go, ge, fs):
    """(score, query rows, bases, columns, identities) of the ops from cell (i0, p0)."""
    i, p, score, cols, ids, shift = i0, p0, 0, 0, 0, 0
    for op in ops:
        n, code = op >> 4, op & 15
        if code == OP_M:
            for _ in range(n):
                score += int(sub[q[i]][a[p + shift]])
                ids += q[i] == a[p + shift]
                p, i, shift = p + shift + 3, i + 1, 0
            cols += n
        elif code == OP_I:
            score += go + n * ge
            i, cols = i + n, cols + n
        elif code == OP_D:
            score += go + n * ge
            p, cols = p + 3 * n, cols + n
        else:
            assert n == 1 and shift == 0 and code in (OP_SKIP, OP_BACK)
            score += fs
            shift = 1 if code == OP_SKIP else -1
    assert shift == 0
    return score, i - i0, p - p0, cols, ids


def py_align(q, t, sub, go, ge, fs, table=None):
    """(record, ops) of protein q against the DNA target t."""
    q, t = [int(x) for x in q], np.asarray(t, np.uint8)
    L, o, e = len(t), go + ge, ge
    if L < 3 or not q:
        return EMPTY
    strands = [aminos(t, table), aminos(SC.revcomp(t), table)]
    ends = [py_end(q, a, sub, o, e, fs) for a in strands]
    rev = int(ends[1][0] > ends[0][0])
    (score, ie, pe), a = ends[rev], strands[rev]
    if score <= 0:
        return EMPTY
    i0, p0 = py_start(q, a, sub, o, e, fs, score, ie, pe)
    ops, at_end = py_walk(q[i0:ie + 1], a[p0:pe + 1], sub, o, e, fs)
    assert at_end == score
    _, _, _, cols, ids = rescore(ops, q, a, i0, p0, sub, go, ge, fs)
    flags = (F.ALIGN_REVERSE if rev else 0) | (p0 % 3) << F.ALIGN_FRAME_SHIFT
    ts, te = (L - 1 - (pe + 2), L - 1 - p0) if rev else (p0, pe + 2)
    return (score, flags, i0, ie, ts, te, cols, ids), ops


def check_record(rec, ops, q, t, sub, go, ge, fs, table=None):
    """The ops re-score to the record's score and span its window."""
    score, flags, qs, qe, ts, te, cols, ids = rec
    if flags & F.ALIGN_EMPTY:
        assert rec == EMPTY[0] and not ops
        return
    t = np.asarray(t, np.uint8)
    L, rev = len(t), bool(flags & F.ALIGN_REVERSE)
    a = aminos(SC.revcomp(t) if rev else t, table)
    p0, pe = (L - 1 - te, L - 1 - ts - 2) if rev else (ts, te - 2)
    assert (flags & F.ALIGN_FRAME_MASK) >> F.ALIGN_FRAME_SHIFT == p0 % 3
    assert ops[0] & 15 == OP_M and ops[-1] & 15 == OP_M
    assert all(x & 15 != y & 15 for x, y in zip(ops, ops[1:]))
    assert all(nxt & 15 == OP_M for op, nxt in zip(ops, ops[1:]) if op & 15 >= OP_SKIP)
    got = rescore(ops, [int(x) for x in q], a, qs, p0, sub, go, ge, fs)
    assert got == (score, qe - qs + 1, pe + 2 - p0 + 1, cols, ids), (got, rec, cigar_text(ops))


# ---- the C model ---------------------------------------------------------------------------------
_LIB = None


def model_lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="fsalign_model_")
        so = os.path.join(d, "libfsalign_model.so")
        subprocess.run([FS._compiler(), "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC",
                        os.path.join(HERE, "c", "fsalign_model.c"), "-o", so], check=True)
        lib = ctypes.CDLL(so)
        P = ctypes.c_void_p
        lib.fsalign_model.restype = ctypes.c_int64
        lib.fsalign_model.argtypes = [P, ctypes.c_size_t, P, ctypes.c_size_t, P, ctypes.c_int, P,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P,
                                      ctypes.c_size_t]
        _LIB = lib
    return _LIB


def c_align(q, t, sub, go, ge, fs, table=None, ops_cap=None):
    """(record, ops) by the C model; ops_cap: the ops the slot holds (default: enough)."""
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    sub = np.ascontiguousarray(sub, np.int8)
    tab = np.ascontiguousarray(F.standard_table() if table is None else table, np.uint8)
    cap = len(q) + len(t) + 2 if ops_cap is None else ops_cap
    rec, ops = np.zeros(9, np.uint32), np.zeros(max(cap, 1), np.uint32)
    p = FS._p
    at_end = model_lib().fsalign_model(p(q), len(q), p(t), len(t), p(sub), sub.shape[0], p(tab),
                                       go, ge, fs, p(rec), p(ops), cap)
    assert at_end == int(rec[0]), "the anchored matrix does not reach the score at the end cell"
    return tuple(int(x) for x in rec[:8]), tuple(int(x) for x in ops[:int(rec[8])])


def no_path(rec):
    """The record of a hit whose path was not produced."""
    return rec[:1] + (rec[1] | F.ALIGN_NO_PATH,) + rec[2:6] + (0, 0)


# ---- the tiny pairs of the CPU tests -------------------------------------------------------------
TINY_FS = (0, -1, -4, -15)
TINY_PEN = ((-11, -1), (-2, -1), (-1, 0), (-4, -4))


def tiny_cases(seed=5, n_random=168, n_planted=96):
    """[(q, t, go, ge, fs)]: m <= 7, L <= 25, 2- and 4-letter DNA; random queries, queries read off
    the target with steps of 2, 3 and 4 bases, and queries with a planted gap of one or two
    codons (dropped from the query: D; put into it: I) under the cheap gap penalties."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_random):
        m, L = int(rng.integers(1, 8)), int(rng.integers(0, 26))
        t = rng.integers(0, 2 if k % 2 else 4, L).astype(np.uint8)
        q = rng.integers(0, 20, m).astype(np.uint8)
        if k % 3 == 0 and L >= 6:
            a, step = aminos(t), (2, 3, 4)[(k // 3) % 3]
            q = np.array([a[p] for p in range(int(rng.integers(0, 3)), len(a), step)][:m], np.uint8)
        out.append((q, t, *TINY_PEN[(k // 4) % 4], TINY_FS[k % 4]))
    for k in range(n_planted):
        g = 1 + k % 2
        t = rng.integers(0, 4, int(rng.integers(21, 26))).astype(np.uint8)
        a = aminos(t)[int(rng.integers(0, 3))::3]
        if k % 4 < 2:  # the target holds g codons the query lacks
            q = a[:3] + a[3 + g:7]
        else:          # the query holds g residues the target lacks
            q = a[:3] + [int(x) for x in rng.integers(0, 20, g)] + a[3:7 - g]
        out.append((np.array(q, np.uint8), t, *TINY_PEN[1 + (k // 4) % 2], TINY_FS[(k // 8) % 4]))
    return out


# ---- the passes at their own seams -----------------------------------------------------------------
def c_mutant(q, t, sub, go, ge, fs, mpass, mrow=-1, mcol=-1, table=None):
    """(record, ops) by the C model with the gap state of pass `mpass` ("A", "B", "C") dropped at
    a seam, in that pass's own numbering: F does not extend into row mrow, E does not extend into
    the columns of codon index mcol.  What the mutant returns need not be an alignment."""
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    sub = np.ascontiguousarray(sub, np.int8)
    tab = np.ascontiguousarray(F.standard_table() if table is None else table, np.uint8)
    cap = len(q) + len(t) + 2
    rec, ops = np.zeros(9, np.uint32), np.zeros(cap, np.uint32)
    lib, p = model_lib(), FS._p
    lib.fsalign_mutant.restype = ctypes.c_int64
    lib.fsalign_mutant.argtypes = lib.fsalign_model.argtypes + [ctypes.c_int, ctypes.c_ssize_t,
                                                                ctypes.c_ssize_t]
    lib.fsalign_mutant(p(q), len(q), p(t), len(t), p(sub), sub.shape[0], p(tab), go, ge, fs,
                       p(rec), p(ops), cap, ord(mpass), mrow, mcol)
    return tuple(int(x) for x in rec[:8]), tuple(int(x) for x in ops[:int(rec[8])])


SEAM_QLEN = {4: 200, 8: 400, 16: 800}  # a query for each of the kernels' rows per lane
SEAM_TIGHT = 3                         # rows of a pass-B window before its run
SEAM_FLANK = 12                        # N codes around a plant: X scores -1, the window is the plant


def seam_family(K, sub, pen, fs=-15, seed=181):
    """(q, [(target, pass, kind, mrow, mcol)], tried): for each pass a window of the query whose
    first row is no multiple of K, with (kind "I") two query rows the target lacks, lying across
    the lane seam K * 5 - 1 | K * 5 in that pass's own row numbering, and (kind "D") two codons
    the query lacks at the codon indices 63 | 64 of that pass's own column numbering, each on
    both strands; a target is kept only if the C model that drops the gap state at that seam in
    that pass returns another record.  Pass B returns no score, only where its best cell lies, and
    losing the gap value moves that cell only if what lies beyond the run is worth less than
    opening the gap again: its windows start SEAM_TIGHT rows before the run."""
    rng = np.random.default_rng([seed, K])
    q = rng.integers(0, 20, SEAM_QLEN[K]).astype(np.uint8)
    n4 = np.full(SEAM_FLANK, 4, np.uint8)
    kept, tried = [], 0
    for pas in "ABC":
        for kind in "ID":
            for rev in (False, True):
                qs = 2 * K + 1
                if kind == "I" and pas == "B":  # (tight: see below)
                    r = qs + SEAM_TIGHT + 1
                    qe = r - 1 + 5 * K
                    core = np.concatenate([F.back_translate(rng, q[qs:r - 1]),
                                           F.back_translate(rng, q[r + 1:qe + 1])])
                    mrow, mcol = 5 * K, -1
                elif kind == "I":
                    qe = qs + 10 * K + 2
                    r = {"A": 5 * K, "C": qs + 5 * K}[pas]  # the run: rows r - 1, r
                    core = np.concatenate([F.back_translate(rng, q[qs:r - 1]),
                                           F.back_translate(rng, q[r + 1:qe + 1])])
                    mrow, mcol = 5 * K, -1
                else:
                    W = 63 + SEAM_TIGHT if pas == "B" else 130
                    qe = qs + W - 1
                    after = {"A": 63 - SEAM_FLANK // 3, "C": 63, "B": W - 63}[pas]
                    core = np.concatenate([F.back_translate(rng, q[qs:qs + after]),
                                           rng.integers(0, 4, 6).astype(np.uint8),
                                           F.back_translate(rng, q[qs + after:qe + 1])])
                    mrow, mcol = -1, 64
                t = np.concatenate([n4, core, n4]).astype(np.uint8)
                t = SC.revcomp(t) if rev else t
                tried += 1
                want = c_align(q, t, sub, *pen, fs)
                if (want[0][2], want[0][3]) != (qs, qe) or bool(want[0][1] & F.ALIGN_REVERSE) != rev:
                    continue
                if c_mutant(q, t, sub, *pen, fs, pas, mrow, mcol) != want:
                    kept.append((t, pas, kind, mrow, mcol))
    return q, kept, tried
