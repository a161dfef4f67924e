"""The model of the non-intersecting local alignments of a pair (a helper, not a test module): the
definition of include/swbank.h "non-intersecting local alignments" restated twice, and the cases
the CPU and GPU tests share.

    py_rounds     plain Python, written straight from the recurrence over dictionaries of cells
                  with a real -infinity and a set of used cells: what the C model is checked against
    c_rounds      tests/c/disjoint_model.c, compiled with the host compiler on first use and
                  loaded with ctypes: what the GPU tests compare against at size.  drop=(kind, at)
                  selects one of its mutants: 1 / 2 lose F / E across a row / column seam, 3 / 4
                  forget the used cells of a row / column
    cells         the cells a record's ops visit
    tiny_pairs    seeded random pairs of at most 9 rows and 11 columns
    copies_case   a target with three copies of a query window: exact, a substitution, an indel
    repeat_case   a query with an internal repeat against a target that holds the unit once
    seam_plants   per rows-per-lane count K the four families of plants of the kernel's seams
    live          which plants a mutant moves

A record is the tuple (score, flags, q_start, q_end, t_start, t_end, n_columns, n_identities);
flags use the library's bits (1 empty, 2 no path).  Every function returns `rounds` (record, ops)
pairs per hit.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import glocal_cases as G

HERE = os.path.dirname(os.path.abspath(__file__))
EMPTY, NO_PATH = 1, 2
OP_M, OP_I, OP_D = 0, 1, 2
NEG = float("-inf")
EMPTY_REC = ((0, EMPTY, 0, 0, 0, 0, 0, 0), ())
MAX_QUERY, MAX_ROUNDS = 1024, 64
ROWS = G.ROWS
FAMILIES = {"lane": 1, "block": 2, "row": 3, "column": 4}   # the family's mutant


def cigar(ops):
    return "".join(f"{op >> 4}{'MID'[op & 15]}" for op in ops)


def _merge(codes):
    ops = []
    for code in codes:
        if ops and ops[-1][1] == code:
            ops[-1][0] += 1
        else:
            ops.append([1, code])
    return tuple(n << 4 | code for n, code in ops)


# ---- the plain-Python restatement --------------------------------------------------------------
def py_rounds(q, t, sub, go, ge, rounds, min_score=1):
    q, t = [int(x) for x in q], [int(x) for x in t]
    m, L = len(q), len(t)
    o, e = go + ge, ge
    used, out = set(), []
    for _ in range(rounds):
        H, E, F = {}, {}, {}
        best, at = 0, None
        for j in range(L):          # columns outside, rows inside: the first maximal cell met
            for i in range(m):      # has the smallest t_end, then the smallest q_end
                if (i, j) in used:
                    H[i, j], E[i, j], F[i, j] = 0, NEG, NEG
                    continue
                M = int(sub[q[i]][t[j]]) + H.get((i - 1, j - 1), 0)
                E[i, j] = max(H.get((i, j - 1), 0) + o, E.get((i, j - 1), NEG) + e)
                F[i, j] = max(H.get((i - 1, j), 0) + o, F.get((i - 1, j), NEG) + e)
                H[i, j] = max(0, M, E[i, j], F[i, j])
                if H[i, j] > best:
                    best, at = H[i, j], (i, j)
        if best < min_score:
            break
        (i, j), state, back, path, idn = at, "H", [], [], 0
        while i >= 0 and j >= 0:
            if state == "H":
                if H[i, j] == 0:
                    break
                if int(sub[q[i]][t[j]]) + H.get((i - 1, j - 1), 0) == H[i, j]:
                    state = "M"
                elif E[i, j] == H[i, j]:
                    state = "E"
                else:
                    state = "F"
            path.append((i, j))
            if state == "M":
                back.append(OP_M)
                idn += q[i] == t[j]
                i, j, state = i - 1, j - 1, "H"
            elif state == "E":
                back.append(OP_D)
                state = "E" if E.get((i, j - 1), NEG) + e > H.get((i, j - 1), 0) + o else "H"
                j -= 1
            else:
                back.append(OP_I)
                state = "F" if F.get((i - 1, j), NEG) + e > H.get((i - 1, j), 0) + o else "H"
                i -= 1
        assert state == "H" and not used & set(path)
        used |= set(path)
        qs, ts = path[-1]
        out.append(((best, 0, qs, at[0], ts, at[1], len(back), idn), _merge(reversed(back))))
    return out + [EMPTY_REC] * (rounds - len(out))


# ---- the C model ---------------------------------------------------------------------------------
class _Rec(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32)] + [(n, ctypes.c_uint32) for n in (
        "flags", "q_start", "q_end", "t_start", "t_end", "n_columns", "n_identities", "n_ops")]


_LIB = None


def model_lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="disjoint_model_")
        so = os.path.join(d, "libdisjoint_model.so")
        subprocess.run([G._compiler(), "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC",
                        os.path.join(HERE, "c", "disjoint_model.c"), "-o", so], check=True)
        lib = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int
        lib.disjoint_model.restype = I
        lib.disjoint_model.argtypes = [P, ctypes.c_size_t, P, ctypes.c_size_t, P, I, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32, I,
                                       ctypes.c_uint32, ctypes.POINTER(_Rec), P, ctypes.c_uint32]
        _LIB = lib
    return _LIB


def c_rounds(q, t, sub, go, ge, rounds, min_score=1, drop=(0, 0), cap=None):
    """`rounds` (record, ops) of one pair by the C model; cap: the ops a slot holds (more: no
    path, the cells used all the same)."""
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    sub = np.ascontiguousarray(sub, np.int8)
    assert sub.shape[0] == sub.shape[1] and rounds >= 1
    assert (len(q) == 0 or q.max() < sub.shape[0]) and (len(t) == 0 or t.max() < sub.shape[0])
    cap = 2 * min(len(q), len(t)) + 1 if cap is None else cap
    ops = np.zeros(max(cap * rounds, 1), np.uint32)
    recs = (_Rec * rounds)()
    st = model_lib().disjoint_model(G._p(q), len(q), G._p(t), len(t), G._p(sub), sub.shape[0], go,
                                    ge, rounds, min_score, drop[0], drop[1], recs, G._p(ops), cap)
    assert st == 0
    return [((r.score, r.flags, r.q_start, r.q_end, r.t_start, r.t_end, r.n_columns,
              r.n_identities), tuple(int(x) for x in ops[k * cap:k * cap + r.n_ops]))
            for k, r in enumerate(recs)]


def scores(rounds_):
    return [rec[0] for rec, _ in rounds_]


def cells(rec, ops):
    """The cells the ops visit from (q_start, t_start): one per M, I and D column."""
    i, j, out = rec[2], rec[4], []
    for op in ops:
        n, code = op >> 4, op & 15
        for _ in range(n):
            if code == OP_M:
                out.append((i, j))
                i, j = i + 1, j + 1
            elif code == OP_I:   # a query residue against a gap: the cell the walk left upwards
                out.append((i, j - 1))
                i += 1
            else:
                out.append((i - 1, j))
                j += 1
    return out


# ---- cases ---------------------------------------------------------------------------------------
def tiny_pairs(count=600, seed=5):
    """[(q, t, sub, go, ge)]: at most 9 rows and 11 columns (L = 0 among them) over two or four
    letters, the 5 / -4 matrix or a random asymmetric one, penalties from free to prohibitive."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        go, ge = [(0, 0), (0, -3), (-8, 0), (-12, -4), (-100, -10), (-1, -1)][k % 6]
        a = (2, 4)[int(rng.integers(0, 2))]
        sub = np.full((a, a), -4, np.int8)
        np.fill_diagonal(sub, 5)
        if rng.integers(0, 2):
            sub = rng.integers(-6, 7, (a, a)).astype(np.int8)
        m, L = int(rng.integers(1, 10)), int(rng.integers(0, 12))
        if k % 50 == 7:
            L = 0
        out.append((rng.integers(0, a, m).astype(np.uint8), rng.integers(0, a, L).astype(np.uint8),
                    sub, go, ge))
    return out


def copies_case(m=90, seed=11):
    """(q, t, (a, b)): a query of m rows and a target that holds its window q[a:b] three times
    between flanks of N: one with a substitution, the exact one, one with a deleted residue."""
    rng = np.random.default_rng([401, m, seed])
    q = G._codes(rng, m)
    a, b = m // 6, m - m // 8
    w = q[a:b]
    sub_ = w.copy()
    sub_[len(w) // 2] = (int(sub_[len(w) // 2]) + 1) % 4
    indel = np.delete(w, len(w) // 3)
    N = lambda n: np.full(n, 4, np.uint8)  # noqa: E731
    t = np.concatenate([N(7), sub_, N(9), w, N(5), indel, N(6)]).astype(np.uint8)
    return q, t, (a, b)


def repeat_case(unit=40, seed=13):
    """(q, t): the query holds a unit twice with a spacer between, the target holds it once."""
    rng = np.random.default_rng([409, unit, seed])
    u = G._codes(rng, unit)
    q = np.concatenate([rng.integers(0, 4, 9), u, rng.integers(0, 4, 13), u,
                        rng.integers(0, 4, 5)]).astype(np.uint8)
    t = np.concatenate([np.full(6, 4), u, np.full(8, 4)]).astype(np.uint8)
    return q, t


def _island(m, row, L, col, shift):
    """A query and a target of N except for the island T C A G, whose cell `shift` of four lies at
    (row, col): the one alignment is that diagonal, and no other cell of the matrix matches, so
    round 1 of the definition is empty."""
    q, t = np.full(m, 4, np.uint8), np.full(L, 4, np.uint8)
    q[row - shift:row - shift + 4] = [0, 1, 2, 3]
    t[col - shift:col - shift + 4] = [0, 1, 2, 3]
    return q, t


def seam_plants(K):
    """{family: [(q, t, drop)]}, four plants each, for queries of 64K - 3 rows.
    lane / block: glocal_cases' plants, a run of two query residues against gaps across the lane
    seam K l - 1 | K l, a run of two target residues against gaps across the block seam
    64 b - 1 | 64 b (mutants 1 and 2).  row / column: an island whose path crosses row K l,
    l = 1 and the last seam but one, or column 64 b, as its second or third cell (mutants 3 and
    4): a walk that forgets the used cells there finds that cell of the copy again in round 1."""
    q = G.plant_query(K)
    m = len(q)
    nl = (m + K - 1) // K
    out = {"lane": [], "block": [], "row": [], "column": []}
    # (K = 4: before the first seam lie too few rows to pay for the gap, as behind the last ones)
    for l in (1, 2, nl // 2, nl - 4):
        t, drop = G.lane_plant(q, K * l, False)
        out["lane"].append((q, t, drop))
    for b in (1, 2, 3, max(4, m // 64 - 2)):  # (K = 4: behind column 256 lie too few rows to pay)
        t, drop = G.block_plant(q, 64 * b, False)
        out["block"].append((q, t, drop))
    for l in (1, nl - 2):
        for shift in (1, 2):
            qq, t = _island(m, K * l, 150, 70 + l % 7, shift)
            out["row"].append((qq, t, (3, K * l)))
    for b in (1, 3):
        for shift in (1, 2):
            qq, t = _island(m, (m // 3) + b, 64 * b + 40, 64 * b, shift)
            out["column"].append((qq, t, (4, 64 * b)))
    return out


def live(plants, sub, go, ge, rounds=3):
    """Per plant: does its mutant change a score of the model."""
    return [scores(c_rounds(q, t, sub, go, ge, rounds)) !=
            scores(c_rounds(q, t, sub, go, ge, rounds, drop=drop)) for q, t, drop in plants]
