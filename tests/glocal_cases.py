"""The model of the global-local search (a helper, not a test module): the definition of
include/swbank.h "global-local search" restated twice, and the cases the CPU and GPU tests share.

    py_strand, py_search   plain Python, written straight from the four lines of the recurrence
                           over dictionaries of cells with a real -infinity: what the C model is
                           checked against
    c_search[_packed|_set] tests/c/glocal_model.c, compiled with the host compiler on first use
                           and loaded with ctypes: what the GPU tests compare against at size.
                           drop=(kind, at) selects one of its seam mutants
    lane_plant             a target that lacks two query rows across a lane seam K l - 1 | K l
    block_plant            a target with two residues the query lacks across a block seam
                           64 j - 1 | 64 j of the strand walked
    seam_plants, live      the plants of one rows-per-lane count and which of them a mutant moves
    asym_case              a batch under an asymmetric DNA matrix and the share its transpose moves
"""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import seam_cases as SEAMS
import strand_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
QUERY, TARGET, BOTH = 1, 2, 3
MODES = (QUERY, TARGET, BOTH)
END_NONE = 0xFFFFFFFF
NEG = float("-inf")
MAX_QUERY = 1024
DNA_PEN = (-12, -4)      # with the 5 / -4 matrix, the reference's penalties
PROT_PEN = (-11, -1)     # with BLOSUM62
ROWS = (4, 8, 16)        # the kernel's rows per lane (swk_glocal_rows): <= 256, <= 512, <= 1,024
ENVELOPE = ((0, 0), (0, -3), (-8, 0), (-100, -10), (-1000, -1))  # (gap_open, gap_extend)


def dna():
    return SEAMS.MATRICES["dna"]()


# ---- the plain-Python restatement --------------------------------------------------------------
def py_strand(q, t, sub, go, ge, ends):
    """(score, end) of one strand; end None for the boundary index -1."""
    m, L = len(q), len(t)
    o, e = go + ge, ge
    H, E, F = {(-1, -1): 0}, {}, {}
    for i in range(m):
        H[i, -1] = o + i * e if ends != TARGET else 0
    for j in range(L):
        H[-1, j] = o + j * e if ends != QUERY else 0
    for i in range(m):
        for j in range(L):
            M = int(sub[q[i]][t[j]]) + H[i - 1, j - 1]
            E[i, j] = max(H[i, j - 1] + o, E.get((i, j - 1), NEG) + e)
            F[i, j] = max(H[i - 1, j] + o, F.get((i - 1, j), NEG) + e)
            H[i, j] = max(M, E[i, j], F[i, j])
    if ends == BOTH:
        return H[m - 1, L - 1], None
    line = [(H[m - 1, j], j) for j in range(-1, L)] if ends == QUERY else \
        [(H[i, L - 1], i) for i in range(-1, m)]
    best = max(v for v, _ in line)
    at = min(x for v, x in line if v == best)
    return best, (None if at < 0 else at)


def py_search(q, t, sub, go, ge, ends, both=False):
    """(score, end, strand): strand 1 only where the reverse strand is strictly better; a QUERY
    end on the reverse strand is given on the forward target."""
    q, t = [int(x) for x in q], [int(x) for x in t]
    fw, fe = py_strand(q, t, sub, go, ge, ends)
    if both:
        rc = [int(x) for x in SC.revcomp(np.array(t, np.uint8))]
        rv, re = py_strand(q, rc, sub, go, ge, ends)
        if rv > fw:
            if ends == QUERY and re is not None:
                re = len(t) - 1 - re
            return rv, END_NONE if re is None else re, 1
    return fw, END_NONE if fe is None else fe, 0


# ---- the C model ---------------------------------------------------------------------------------
_LIB = None


def _compiler():
    for c in ("cc", "gcc", "clang"):
        if shutil.which(c):
            return shutil.which(c)
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang")
    if os.path.exists(rocm):
        return rocm
    raise RuntimeError("no host C compiler was found")


def model_lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="glocal_model_")
        so = os.path.join(d, "libglocal_model.so")
        subprocess.run([_compiler(), "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC",
                        os.path.join(HERE, "c", "glocal_model.c"), "-o", so], check=True)
        lib = ctypes.CDLL(so)
        P, I = ctypes.c_void_p, ctypes.c_int
        lib.glocal_model.restype = None
        lib.glocal_model.argtypes = [P, ctypes.c_size_t, P, P, P, ctypes.c_size_t, P, I,
                                     ctypes.c_int32, ctypes.c_int32, I, I, I, ctypes.c_uint32,
                                     P, P, P]
        _LIB = lib
    return _LIB


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def c_search_packed(q, res, offs, lens, sub, go, ge, ends, both=False, drop=(0, 0)):
    """(scores int32 [n], ends uint32 [n], strands uint8 [n]) of q against a packed batch."""
    q = np.ascontiguousarray(q, np.uint8)
    res = np.ascontiguousarray(res, np.uint8)
    offs = np.ascontiguousarray(offs, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint32)
    sub = np.ascontiguousarray(sub, np.int8)
    assert sub.shape[0] == sub.shape[1] and len(offs) == len(lens) and ends in MODES
    assert all(int(o) + int(n) <= len(res) for o, n in zip(offs, lens))
    assert (len(q) == 0 or q.max() < sub.shape[0]) and not (both and sub.shape[0] != 5)
    n = len(lens)
    sc, ep, sd = (np.zeros(max(n, 1), d) for d in (np.int32, np.uint32, np.uint8))
    model_lib().glocal_model(_p(q), len(q), _p(res), _p(offs), _p(lens), n, _p(sub), sub.shape[0],
                             go, ge, ends, int(both), drop[0], drop[1], _p(sc), _p(ep), _p(sd))
    return sc[:n], ep[:n], sd[:n]


def pack(seqs):
    lens = np.array([len(s) for s in seqs], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) \
        if len(seqs) else np.zeros(0, np.uint64)
    res = np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [np.zeros(1, np.uint8)])
    return res, offs, lens


def c_search(q, seqs, sub, go, ge, ends, both=False, drop=(0, 0)):
    return c_search_packed(q, *pack(seqs), sub, go, ge, ends, both, drop)


def c_search_set(qs, seqs, sub, go, ge, ends, both=False):
    """(scores [nq, n], ends [nq, n], strands [nq, n])."""
    per = [c_search(q, seqs, sub, go, ge, ends, both) for q in qs]
    return tuple(np.stack([p[i] for p in per]) for i in range(3))


# ---- seam plants ---------------------------------------------------------------------------------
def _codes(rng, n):
    """n random codes of T, C, A, G, none equal to either of the two before it: a run of two gaps
    has one place only (it slides by one where q[i] == q[i + 2])."""
    out = np.zeros(n, np.uint8)
    for i in range(n):
        c = int(rng.integers(0, 4))
        while c in (int(out[i - 1]) if i else -1, int(out[i - 2]) if i > 1 else -1):
            c = int(rng.integers(0, 4))
        out[i] = c
    return out


def lane_plant(q, row, reverse):
    """The whole query without its rows row - 1 and row, in N flanks: the alignment holds a run of
    two query residues against gaps from row - 1 into row.  (target, (1, row))."""
    t = np.concatenate([np.full(3, 4), q[:row - 1], q[row + 1:], np.full(2, 4)]).astype(np.uint8)
    return (SC.revcomp(t) if reverse else t), (1, row)


def block_plant(q, col, reverse):
    """The whole query with two more residues at columns col - 1 and col of the strand walked,
    behind a flank of N: a run of two target residues against gaps from col - 1 into col.  The
    two differ from each other and from the query's residues on either side, so the run has one
    place.  (target, (2, col)); the query has at least 8 rows and col >= 9."""
    a = min(len(q) - 4, col - 5)         # query rows before the two residues
    flank = col - 1 - a
    free = [c for c in range(4) if c not in (int(q[a - 1]), int(q[a]))]
    t = np.concatenate([np.full(flank, 4), q[:a], free, q[a:], np.full(3, 4)]).astype(np.uint8)
    assert flank >= 1 and len(free) == 2 and flank + a == col - 1
    return (SC.revcomp(t) if reverse else t), (2, col)


def plant_query(K):
    """A query for the seams of K rows per lane: the longest that K serves, less three rows."""
    m = {4: 256, 8: 512, 16: 1024}[K] - 3
    return _codes(np.random.default_rng([211, K]), m)


def seam_plants(K):
    """[(kind, target, drop)]: four lane plants (two seams, both strands) and four block plants
    (two seams, both strands) for the query plant_query(K)."""
    q = plant_query(K)
    nl = (len(q) + K - 1) // K
    out = []
    for l in (1, nl - 2):  # (behind the last seam too few rows are left to pay for a gap)
        for rev in (False, True):
            out.append(("lane",) + lane_plant(q, K * l, rev))
    for j in (1, (len(q) // 2) // 64 + 1):
        for rev in (False, True):
            out.append(("block",) + block_plant(q, 64 * j, rev))
    return q, out


def live(q, plants, sub, go, ge, ends=QUERY):
    """Per plant: does the model's mutant (F or E dropped at the plant's seam) change the score
    of the both-strand search."""
    flags = []
    for _, t, drop in plants:
        want = c_search(q, [t], sub, go, ge, ends, True)
        mut = c_search(q, [t], sub, go, ge, ends, True, drop)
        flags.append(int(want[0][0]) != int(mut[0][0]))
    return flags


# ---- an asymmetric matrix ------------------------------------------------------------------------
ASYM = "asym-pair"
ASYM_PEN = (-12, -4)


def asym_case():
    """(q, targets): 48 DNA targets for a 70-row query, two thirds of them noisy copies of a
    window of it on either strand."""
    rng = np.random.default_rng(227)
    q = rng.integers(0, 4, 70).astype(np.uint8)
    seqs = []
    for k in range(48):
        if k % 3 == 2:
            seqs.append(rng.integers(0, 5, int(rng.integers(0, 120))).astype(np.uint8))
            continue
        a = int(rng.integers(0, 30))
        w = q[a:a + int(rng.integers(20, 41))].copy()
        w[rng.integers(0, len(w), 3)] = rng.integers(0, 4, 3)
        t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 9))), w,
                            rng.integers(0, 4, int(rng.integers(0, 9)))]).astype(np.uint8)
        seqs.append(SC.revcomp(t) if k % 2 else t)
    return q, seqs


def transposed_share(q, seqs, sub, go, ge, ends, both):
    """The share of the batch's scores that the transposed matrix changes in the model."""
    want = c_search(q, seqs, sub, go, ge, ends, both)[0]
    wrong = c_search(q, seqs, np.ascontiguousarray(np.asarray(sub).T), go, ge, ends, both)[0]
    return float((want != wrong).mean())
