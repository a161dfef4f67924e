"""The model of the frameshift-tolerant translated search (a helper, not a test module): the
definition of include/swbank.h "frameshift-tolerant translated search" restated twice.

    py_strand, py_search   plain Python, written straight from the four lines of the recurrence
                           over dictionaries of cells: what the C model is checked against
    c_search               tests/c/fshift_model.c, compiled with the host compiler on first use
                           and loaded with ctypes: what the GPU tests compare against at size
    six_frames             the merged six-frame scores and strands (frame >= 3) by the oracle on
                           the model's translations (frame_cases): the anchor at fs = -32767
    shift_case             a query A + B and a target holding bt(A) + one base + bt(B) (an
                           insertion) or bt(A) + bt(B)[1:] (a deletion) in random flanks, on
                           either strand

Everything else (translate, back_translate, the tables, the matrices) is frame_cases' and
matrix_cases'.
"""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

import frame_cases as F
import strand_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
FS_VALUES = (0, -1, -15, -32767)
NEG = -(1 << 60)
PEN = F.PEN
SHIFT_FS = -15
SHIFT_HALF = 20  # |A| = |B|


# ---- the plain-Python restatement --------------------------------------------------------------
def py_strand(q, c, sub, go, ge, fs, table=None):
    """The strand score of protein q against the DNA codes c."""
    tab = F.standard_table() if table is None else np.asarray(table, np.uint8)
    m, L = len(q), len(c)
    if L < 3:
        return 0
    o, e = go + ge, ge
    a = [int(tab[c[p] * 16 + c[p + 1] * 4 + c[p + 2]])
         if max(c[p], c[p + 1], c[p + 2]) < 4 else F.X for p in range(L - 2)]
    H, E, Fg = {}, {}, {}

    def h(i, p):
        return H.get((i, p), 0)

    best = 0
    for i in range(m):
        for p in range(L - 2):
            M = int(sub[q[i]][a[p]]) + max(0, h(i - 1, p - 3), h(i - 1, p - 2) + fs,
                                           h(i - 1, p - 4) + fs)
            E[i, p] = max(h(i, p - 3) + o, E.get((i, p - 3), NEG) + e)
            Fg[i, p] = max(h(i - 1, p) + o, Fg.get((i - 1, p), NEG) + e)
            H[i, p] = max(0, M, E[i, p], Fg[i, p])
            best = max(best, H[i, p])
    return best


def py_search(q, t, sub, go, ge, fs, table=None):
    """(score, strand) of the search: strand 1 only where the reverse strand is strictly better."""
    q, t = [int(x) for x in q], [int(x) for x in t]
    fw = py_strand(q, t, sub, go, ge, fs, table)
    rv = py_strand(q, [int(x) for x in SC.revcomp(np.array(t, np.uint8))], sub, go, ge, fs, table)
    return (rv, 1) if rv > fw else (fw, 0)


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
        d = tempfile.mkdtemp(prefix="fshift_model_")
        so = os.path.join(d, "libfshift_model.so")
        subprocess.run([_compiler(), "-O2", "-std=c11", "-Wall", "-Werror", "-shared", "-fPIC",
                        os.path.join(HERE, "c", "fshift_model.c"), "-o", so], check=True)
        lib = ctypes.CDLL(so)
        P = ctypes.c_void_p
        lib.fshift_model.restype = None
        lib.fshift_model.argtypes = [P, ctypes.c_size_t, P, P, P, ctypes.c_size_t, P, ctypes.c_int,
                                     P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P]
        _LIB = lib
    return _LIB


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def c_search_packed(q, res, offs, lens, sub, go, ge, fs, table=None):
    """(scores int32 [n], strands uint8 [n]) of protein q against a packed DNA batch."""
    q = np.ascontiguousarray(q, np.uint8)
    res = np.ascontiguousarray(res, np.uint8)
    offs = np.ascontiguousarray(offs, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint32)
    sub = np.ascontiguousarray(sub, np.int8)
    tab = np.ascontiguousarray(F.standard_table() if table is None else table, np.uint8)
    assert sub.shape[0] == sub.shape[1] and tab.shape == (64,) and len(offs) == len(lens)
    assert all(int(o) + int(n) <= len(res) for o, n in zip(offs, lens))
    n = len(lens)
    sc, sd = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
    model_lib().fshift_model(_p(q), len(q), _p(res), _p(offs), _p(lens), n, _p(sub), sub.shape[0],
                             _p(tab), go, ge, fs, _p(sc), _p(sd))
    return sc[:n], sd[:n]


def c_search(q, seqs, sub, go, ge, fs, table=None):
    lens = np.array([len(s) for s in seqs], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) \
        if len(seqs) else np.zeros(0, np.uint64)
    res = np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [np.zeros(1, np.uint8)])
    return c_search_packed(q, res, offs, lens, sub, go, ge, fs, table)


def c_search_set(qs, seqs, sub, go, ge, fs, table=None):
    """(scores [nq, n], strands [nq, n])."""
    per = [c_search(q, seqs, sub, go, ge, fs, table) for q in qs]
    return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])


# ---- the six-frame anchor ------------------------------------------------------------------------
def six_frames(q, seqs, sub=O.BLOSUM62, pen=PEN, table=None):
    """(merged scores, strands = (frame >= 3)) by the oracle on the model's six translations."""
    sc, fr = F.merge6(F.oracle_frames(q, seqs, sub, pen, O.GAP_GOTOH, table))
    return sc, (fr >= 3).astype(np.uint8)


# ---- planted shifts ------------------------------------------------------------------------------
def shift_case(rng, kind, reverse, flank=(0, 40), table=None):
    """(query A + B, target, A, B): the target is random flanks around bt(A) + one base + bt(B)
    (kind "ins") or around bt(A) + bt(B)[1:] (kind "del"), reverse-complemented when `reverse`."""
    A = rng.integers(0, 20, SHIFT_HALF).astype(np.uint8)
    B = rng.integers(0, 20, SHIFT_HALF).astype(np.uint8)
    a, b = F.back_translate(rng, A, table), F.back_translate(rng, B, table)
    mid = np.concatenate([a, rng.integers(0, 4, 1).astype(np.uint8), b]) if kind == "ins" else \
        np.concatenate([a, b[1:]])
    left, right = (rng.integers(0, 4, int(rng.integers(flank[0], flank[1] + 1))).astype(np.uint8)
                   for _ in range(2))
    t = np.concatenate([left, mid, right]).astype(np.uint8)
    return np.concatenate([A, B]), (SC.revcomp(t) if reverse else t), A, B


def shift_bound(kind, A, B, fs, sub=O.BLOSUM62):
    """What the planted pair scores at least: both halves in their frames and one shift; a
    deletion takes B's first codon, whose residue then meets a codon of any amino acid."""
    if kind == "ins":
        return F.self_score(A, sub) + F.self_score(B, sub) + fs
    return F.self_score(A, sub) + F.self_score(B[1:], sub) + fs + int(np.asarray(sub)[:20, :20].min())


def shift_cases(seed=97, per=10):
    """[(kind, reverse, q, t, A, B)]: `per` cases of each kind on each strand."""
    rng = np.random.default_rng(seed)
    return [(kind, rev) + shift_case(rng, kind, rev)
            for kind in ("ins", "del") for rev in (False, True) for _ in range(per)]
