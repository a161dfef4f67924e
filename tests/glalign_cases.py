"""The model of the alignments of global-local hits (a helper, not a test module): the definition
of include/swbank.h "alignments of global-local hits" restated twice, and the cases the CPU and
GPU tests share.

    py_align     plain Python over dictionaries of cells with a real -infinity: the search of
                 glocal_cases.py_search, the start by brute force over the boundary cells (the
                 BOTH score of every candidate window), the path by the documented preference in
                 the anchored window: what the C model is checked against
    c_align      tests/c/glalign_model.c, compiled with the host compiler on first use and loaded
                 with ctypes: what the GPU tests compare against at size.  drops=(A, B, C), each
                 (kind, at), selects a seam mutant of one pass in that pass's own rows and columns
    rescore      what a list of ops scores, and the rows and columns it consumes
    pass_plants  per pass, pairs whose gap runs cross a lane seam and a 64-step block seam of
    live         that pass, and which of them the pass's mutant moves
    tie_pairs    low-complexity pairs whose paths are rich in co-optimal alternatives

A record is the tuple (score, flags, q_start, q_end, t_start, t_end, n_columns, n_identities);
flags use the library's bits (1 empty, 2 no path, 8 reverse).
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import glocal_cases as G
import strand_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
QUERY, TARGET, BOTH = G.QUERY, G.TARGET, G.BOTH
EMPTY, NO_PATH, REVERSE = 1, 2, 8
OP_M, OP_I, OP_D = 0, 1, 2
NEG = float("-inf")
NO_DROPS = ((0, 0), (0, 0), (0, 0))


def cigar(ops):
    return "".join(f"{op >> 4}{'MID'[op & 15]}" for op in ops)


# ---- the plain-Python restatement --------------------------------------------------------------
def _anchored_path(q, c, sub, go, ge):
    """(score, ops, columns, identities) of the anchored matrix of q x c, walked back from the
    last cell in state H: M, then D (E), then I (F); a run opens when opening and extending tie."""
    m, L = len(q), len(c)
    o, e = go + ge, ge
    H, E, F = {(-1, -1): 0}, {}, {}
    for i in range(m):
        H[i, -1] = o + i * e
    for j in range(L):
        H[-1, j] = o + j * e
    for i in range(m):
        for j in range(L):
            E[i, j] = max(H[i, j - 1] + o, E.get((i, j - 1), NEG) + e)
            F[i, j] = max(H[i - 1, j] + o, F.get((i - 1, j), NEG) + e)
            H[i, j] = max(int(sub[q[i]][c[j]]) + H[i - 1, j - 1], E[i, j], F[i, j])
    back, i, j, state, idn = [], m - 1, L - 1, "H", 0
    while i >= 0 and j >= 0:
        if state == "H":
            if int(sub[q[i]][c[j]]) + H[i - 1, j - 1] == H[i, j]:
                state = "M"
            elif E[i, j] == H[i, j]:
                state = "E"
            else:
                state = "F"
        if state == "M":
            back.append(OP_M)
            idn += q[i] == c[j]
            i, j, state = i - 1, j - 1, "H"
        elif state == "E":
            back.append(OP_D)
            state = "E" if E.get((i, j - 1), NEG) + e > H[i, j - 1] + o else "H"
            j -= 1
        else:
            back.append(OP_I)
            state = "F" if F.get((i - 1, j), NEG) + e > H[i - 1, j] + o else "H"
            i -= 1
    back += [OP_D] * (j + 1) + [OP_I] * (i + 1)
    ops = []
    for code in reversed(back):
        if ops and ops[-1][1] == code:
            ops[-1][0] += 1
        else:
            ops.append([1, code])
    return H[m - 1, L - 1], tuple(n << 4 | code for n, code in ops), len(back), idn


def py_align(q, t, sub, go, ge, ends, both=False):
    """(record, ops) of one pair by the definition."""
    q, t = [int(x) for x in q], [int(x) for x in t]
    m, L = len(q), len(t)
    score, end, strand = G.py_search(q, t, sub, go, ge, ends, both)
    if (L == 0) if ends == BOTH else end == G.END_NONE:
        return (score, EMPTY, 0, 0, 0, 0, 0, 0), ()
    c = [int(x) for x in SC.revcomp(np.array(t, np.uint8))] if strand else t
    qs, qe, ts, te = 0, m - 1, 0, L - 1
    if ends == QUERY:
        te = L - 1 - end if strand else end  # on the strand walked
        ts = max(a + 1 for a in range(-1, te)
                 if G.py_strand(q, c[a + 1:te + 1], sub, go, ge, BOTH)[0] == score)
        assert all(G.py_strand(q, c[a + 1:te + 1], sub, go, ge, BOTH)[0] <= score
                   for a in range(-1, te))
    elif ends == TARGET:
        qe = end
        qs = max(r + 1 for r in range(-1, qe)
                 if G.py_strand(q[r + 1:qe + 1], c, sub, go, ge, BOTH)[0] == score)
        assert all(G.py_strand(q[r + 1:qe + 1], c, sub, go, ge, BOTH)[0] <= score
                   for r in range(-1, qe))
    got, ops, cols, idn = _anchored_path(q[qs:qe + 1], c[ts:te + 1], sub, go, ge)
    assert got == score, (got, score)
    t0, t1 = (L - 1 - te, L - 1 - ts) if strand else (ts, te)
    return (score, REVERSE if strand else 0, qs, qe, t0, t1, cols, idn), ops


# ---- the C model ---------------------------------------------------------------------------------
class _Rec(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32)] + [(n, ctypes.c_uint32) for n in (
        "flags", "q_start", "q_end", "t_start", "t_end", "n_columns", "n_identities", "n_ops",
        "tie_diag", "tie_left", "tie_open")]


_LIB = None


def model_lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="glalign_model_")
        so = os.path.join(d, "libglalign_model.so")
        subprocess.run([G._compiler(), "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC",
                        os.path.join(HERE, "c", "glalign_model.c"), "-o", so], check=True)
        lib = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int
        lib.glalign_model.restype = None
        lib.glalign_model.argtypes = [P, ctypes.c_size_t, P, ctypes.c_size_t, P, I, ctypes.c_int32,
                                      ctypes.c_int32, I, I, P, ctypes.POINTER(_Rec), P,
                                      ctypes.c_uint32]
        _LIB = lib
    return _LIB


def c_align(q, t, sub, go, ge, ends, both=False, drops=NO_DROPS, cap=None, ties=False):
    """(record, ops) of one pair by the C model; cap: the ops the slot holds (else no path).
    ties: also the counts (diagonal/gap, left/up, open/extend) of co-optimal path cells."""
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    sub = np.ascontiguousarray(sub, np.int8)
    assert sub.shape[0] == sub.shape[1] and ends in G.MODES and not (both and sub.shape[0] != 5)
    assert (len(q) == 0 or q.max() < sub.shape[0]) and (len(t) == 0 or t.max() < sub.shape[0])
    cap = len(q) + len(t) + 1 if cap is None else cap
    ops = np.zeros(max(cap, 1), np.uint32)
    dr = np.array(drops, np.uint32).reshape(6)
    r = _Rec()
    G_p = G._p
    model_lib().glalign_model(G_p(q), len(q), G_p(t), len(t), G_p(sub), sub.shape[0], go, ge, ends,
                              int(both), G_p(dr), ctypes.byref(r), G_p(ops), cap)
    rec = (r.score, r.flags, r.q_start, r.q_end, r.t_start, r.t_end, r.n_columns, r.n_identities)
    out = rec, tuple(int(x) for x in ops[:r.n_ops])
    return out + ((r.tie_diag, r.tie_left, r.tie_open),) if ties else out


# ---- preference-free checks ----------------------------------------------------------------------
def rescore(ops, q, c, sub, go, ge):
    """(score, rows, columns) of the ops over the query window q and the strand window c: a gap
    run of k columns costs open + k extend."""
    i = j = score = 0
    for op in ops:
        n, code = op >> 4, op & 15
        if code == OP_M:
            score += sum(int(sub[q[i + k]][c[j + k]]) for k in range(n))
            i, j = i + n, j + n
        else:
            score += go + n * ge
            i, j = (i + n, j) if code == OP_I else (i, j + n)
    return score, i, j


def check_record(rec, ops, q, t, sub, go, ge, ends, both):
    """What holds for every record whatever the preference: the search's score, end and strand;
    the ops consume the window, merge equal codes and re-score to the score."""
    score, flags, qs, qe, ts, te, cols, idn = rec
    m, L = len(q), len(t)
    sc, ep, sd = (int(x[0]) for x in G.c_search(q, [t], sub, go, ge, ends, both))
    assert score == sc and bool(flags & REVERSE) == bool(sd)
    if flags & EMPTY:
        assert (L == 0) if ends == BOTH else ep == G.END_NONE
        assert rec[2:] == (0,) * 6 and not ops and not flags & REVERSE
        return
    if ends == QUERY:
        assert (qs, qe) == (0, m - 1) and (ts if sd else te) == ep
    elif ends == TARGET:
        assert (ts, te) == (0, L - 1) and qe == ep
    else:
        assert (qs, qe, ts, te) == (0, m - 1, 0, L - 1)
    if flags & NO_PATH:
        assert not ops and cols == idn == 0
        return
    c = SC.revcomp(np.asarray(t, np.uint8)) if sd else np.asarray(t, np.uint8)
    c0, c1 = (L - 1 - te, L - 1 - ts) if sd else (ts, te)
    got, rows, columns = rescore(ops, q[qs:qe + 1], c[c0:c1 + 1], sub, go, ge)
    assert (got, rows, columns) == (score, qe - qs + 1, c1 - c0 + 1), (rec, cigar(ops), got)
    assert all((a & 15) != (b & 15) for a, b in zip(ops, ops[1:])) and all(op >> 4 for op in ops)
    assert cols == sum(op >> 4 for op in ops) and idn <= cols


# ---- seam plants, per pass -----------------------------------------------------------------------
def _block(w, a, reverse):
    """w with two more residues before its residue a, unlike each other and their neighbours: a
    run of two target residues against gaps at columns a and a + 1 with one place only."""
    free = [x for x in range(4) if x not in (int(w[a - 1]), int(w[a]))]
    t = np.concatenate([w[:a], free, w[a:]]).astype(np.uint8)
    return SC.revcomp(t) if reverse else t


def _q(K, m):
    return G._codes(np.random.default_rng([311, K, m]), m)


def _lane_b(q, rev):
    """The query behind a flank of N without its rows 2 and 3: in pass B's rows r' = m - 1 - i
    the run goes from r' = m - 4 into m - 3.  So near the end of the reversed walk the run is
    worth only 6 more than four mismatches from two columns earlier, which cross that seam on the
    diagonal: a walk that pays for opening the run twice (12) finds another start."""
    t = np.concatenate([np.full(3, 4), q[:2], q[4:]]).astype(np.uint8)
    return SC.revcomp(t) if rev else t


def _block_b(q, rev):
    """The query with two more residues behind its row 2, no flanks: in pass B's columns
    j' = t_end - j they lie at j' = m - 3 and m - 2.  The run is worth 7 more than three
    mismatches from two columns later (the two residues match none of the rows 0 to 2 there)."""
    x = [c for c in range(4) if c not in (int(q[1]), int(q[2]), int(q[3]))][0]
    t = np.concatenate([q[:3], [x, q[1]], q[3:]]).astype(np.uint8)
    return SC.revcomp(t) if rev else t


def pass_plants(K):
    """{family: [(q, target, drops)] x 4}: per pass, runs of two query residues against gaps
    across a lane seam K l - 1 | K l and runs of two target residues against gaps across a block
    seam 64 b - 1 | 64 b, in THAT pass's own rows and columns, on both strands.  drops is the C
    model's mutant that loses the gap state at that seam.

    Pass B walks the rows q[q_end..0] and the columns c[t_end..0]: its row r' is the query row
    q_end - r', its column j' the strand column t_end - j'.  Only the POSITION of its best cell
    goes into the record, so a plant of pass B lies near the start of the alignment, where losing
    the gap state moves the start (see _lane_b, _block_b).  Pass C walks the window from q_start
    and t_start.
      "B query"   ends = QUERY: a lane seam at r' = m - 3 (queries of K l + 3 rows) and a block
                  seam at j' = m - 2 (queries of 64 b + 2 rows).
      "B target"  ends = TARGET: the target is the query's rows lead .. hi - 1 without the rows
                  lead + 3 and lead + 4 (worth 7 more than three mismatches from two rows later):
                  lane seams at r' = hi - 4 - lead = K l, l = 40 and 41.
      "C query"   ends = QUERY: the plants of glocal_cases (the query in N flanks): the window's
                  rows are the query's and its columns start behind the flank.
      "C target"  ends = TARGET: the target is the query's rows lead .. hi - 1 (lead = 2 K + 1), so
                  the window's rows start at q_start = lead, no multiple of K: pass C's lane seams
                  are not pass A's."""
    def in_b(kind, at):
        return ((0, 0), (kind, at), (0, 0))

    def in_c(kind, at):
        return ((0, 0), (0, 0), (kind, at))

    out = {"B query": [], "B target": [], "C query": [], "C target": []}
    ml = K * 62 + 3                               # 251, 499, 995 rows
    mb = 64 * {4: 3, 8: 5, 16: 9}[K] + 2          # 194, 322, 578 rows
    for rev in (False, True):
        out["B query"].append((_q(K, ml), _lane_b(_q(K, ml), rev), in_b(1, ml - 3)))
        out["B query"].append((_q(K, mb), _block_b(_q(K, mb), rev), in_b(2, mb - 2)))
    q = G.plant_query(K)
    m = len(q)
    lead = 2 * K + 1
    for lane, rev in ((40, False), (40, True), (41, False), (41, True)):
        hi = lead + 4 + K * lane
        w = np.delete(q[lead:hi], [3, 4])
        out["B target"].append((q, SC.revcomp(w) if rev else w, in_b(1, K * lane)))
    for lane, rev in ((1, False), (2, True)):
        out["C query"].append((q, G.lane_plant(q, K * lane, rev)[0], in_c(1, K * lane)))
        w = np.delete(q[lead:m - 5], [K * lane - 1, K * lane])  # window rows K l - 1 | K l
        out["C target"].append((q, SC.revcomp(w) if rev else w, in_c(1, K * lane)))
    for rev in (False, True):
        # block_plant(q, 68): a flank of 4 N, q[:63], the two residues, the rest of q: the window
        # starts behind the flank, so the run lies at its columns 63 | 64
        out["C query"].append((q, G.block_plant(q, 68, rev)[0], in_c(2, 64)))
        out["C target"].append((q, _block(q[lead:lead + 150], 63, rev), in_c(2, 64)))
    return out


ENDS_OF = {"B query": QUERY, "B target": TARGET, "C query": QUERY, "C target": TARGET}


def live(plants, sub, go, ge, ends):
    """Per plant: does the C model's mutant of the plant's pass change the record or the ops."""
    return [c_align(q, t, sub, go, ge, ends, True) != c_align(q, t, sub, go, ge, ends, True, drops)
            for q, t, drops in plants]


# ---- ties ----------------------------------------------------------------------------------------
def tie_pairs(n=24, seed=313):
    """[(q, t)]: two-letter sequences, where many cells have co-optimal sources."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m, L = int(rng.integers(20, 70)), int(rng.integers(20, 90))
        q = rng.integers(0, 2, m).astype(np.uint8) * 2   # T and A: the reverse strand is alike
        t = rng.integers(0, 2, L).astype(np.uint8) * 2
        if k % 3 == 0:
            t = np.concatenate([t[:L // 2], q[m // 4:3 * m // 4], t[L // 2:]]).astype(np.uint8)
        out.append((q, t))
    return out
