"""The scoring-parameter envelope of the frameshift search and its aligner (a helper, not a test
module): what seam_cases.CASES is to the plain kernels, for sw_score_fshift*,
sw_align_fshift_hits* and sw_estimate_fshift_statistics* (include/swbank.h).

    MATRICES, CASES   the protein matrices and the (matrix, open, extend) cases; the limit case
                      o + e + S = 65535; REFUSED, the two cases past the accepted envelope
    FS_VALUES         the frameshift penalties every case runs under
    noise_batch       per (case, K) a query of 33 / 300 / 700 rows and 64 DNA targets of 0..400
                      codes: shifted windows, windows with codons dropped or added, windows planted
                      twice (the best value at two cells), random targets, N codes, an empty and a
                      two-code target
    seam_family       per (case with go < 0, K) a query of 256 / 512 / 1,024 rows and targets whose
                      gap runs across a lane seam (kind I) or a 64-step block seam (kind D) of the
                      *score* walk, on both strands in N flanks; the mutant of the C model
                      (fsalign_cases.c_mutant, pass "A") says which are live
    edge_batch        pad rows and pad columns: queries of 255 .. 257 and 1,023 / 1,024 rows against
                      windows of their last rows at the very end of a strand, L mod 3 = 0, 1, 2
    fuzz_case         one seeded random case
    stats_reference   stat_cases.shuffle -> fshift_cases.c_search_set -> histogram -> fit under any
                      matrix and penalties
    best_cells        how many cells of the winning strand hold the score (the C model counts)

A gap is paid for only where the flanks outweigh it and its re-opening: each side of a planted run
gets NEED(case) = (|o| + |e| + |go|) / 4 + 20 rows, the lane seams are those with that many rows on
both sides (the middle one where none has), the block seams the first two multiples of 64 past the
flank.  A cheap shift replaces a dear gap (at fs = -15 and -100 / -10 six p - 2 steps absorb a
two-residue gap for about 109 points), so the families of the cases with |go| >= 100 are made and
measured at fs = -32767; the other frameshift values still run over them for exactness.  With
go = 0 extending never beats opening, no mutant can be live, and those cases have no family: they
are the tie-rule cases instead.
"""
import collections
import ctypes
import functools

import numpy as np

from oracle import oracle as O

import frame_cases as F
import fsalign_cases as A
import fshift_cases as FS
import fshift_stats_cases as FSS
import seam_cases as SEAMS
import stat_cases as ST
import strand_cases as SC

Case = collections.namedtuple("Case", "name matrix go ge tags")
FS_VALUES = (0, -1, -15, -32767)
NOISE_QLEN = {4: 33, 8: 300, 16: 700}    # per rows-per-lane of the kernels
SEAM_QLEN = {4: 256, 8: 512, 16: 1024}
ROWS = (4, 8, 16)
N_FLANK = 12                             # N codes around a plant: four codon indices


# ---- matrices ------------------------------------------------------------------------------------
def _nopos_prot(top):
    rng = np.random.default_rng(31 - top)
    m = rng.integers(-9, top + 1, (24, 24)).astype(np.int8)
    m[np.arange(24), np.arange(24)] = top
    assert m.max() == top and (m != m.T).any()
    return m


def _wide_prot():
    """+-127 only, span exactly 254, not symmetric."""
    m = np.full((24, 24), -127, np.int8)
    m[np.arange(24), np.arange(24)] = 127
    m[3, 17] = m[9, 2] = m[14, 15] = 127
    assert int(m.max()) - int(m.min()) == 254 and (m != m.T).any()
    return m


def _pad_prot():
    """asym-prot with -128 (the kernels' pad score) in one entry in twelve of the rows of real
    residues, off the diagonal, and in the whole X column: a codon holding N scores what a cell
    outside the matrix scores."""
    m = SEAMS.MATRICES["asym-prot"]().copy()
    rng = np.random.default_rng(47)
    hit = rng.random((20, 24)) < 1 / 12
    hit[np.arange(20), np.arange(20)] = False
    m[:20][hit] = -128
    m[:, F.X] = -128
    assert m.min() == -128 and m.max() == 12 and (m != m.T).mean() > 0.8
    assert (m[:20, :20] == -128).any(axis=1).sum() >= 8
    return m


def _span255_prot():
    m = _wide_prot()
    m[5, 6] = -128
    return m


MATRICES = {
    "blosum62": SEAMS.MATRICES["blosum62"], "asym-prot": SEAMS.MATRICES["asym-prot"],
    "nopos0-prot": lambda: _nopos_prot(0), "nopos1-prot": lambda: _nopos_prot(-1),
    "wide-prot": _wide_prot, "pad-prot": _pad_prot, "span255-prot": _span255_prot,
}


@functools.lru_cache(maxsize=None)
def matrix(name):
    m = np.ascontiguousarray(MATRICES[name](), np.int8)
    m.setflags(write=False)
    return m


# ---- cases ---------------------------------------------------------------------------------------
PAIRS = ((0, 0), (0, -3), (-8, 0), (-1, -30), (-100, -10), (-300, -40), (-1000, -1))
LIMIT = (-32767, -32757)  # o + e + S = 32767 + 32757 + 11 = 65535 under BLOSUM62


def _cases():
    out = []

    def add(mat, go, ge, *tags):
        tags = set(tags) | ({"tie"} if go == 0 else {"seam"})
        out.append(Case(f"{mat}{go}/{ge}", mat, go, ge, frozenset(tags)))

    for go, ge in PAIRS:
        add("blosum62", go, ge)
    for go, ge in ((0, 0), (-8, 0), (-100, -10)):
        add("asym-prot", go, ge, "asym")
    for mat in ("pad-prot", "wide-prot"):
        for go, ge in ((0, 0), (-8, 0)):
            add(mat, go, ge, "edge", *(["asym"] if mat == "pad-prot" else []))
    add("nopos0-prot", -11, -1, "nopos")
    add("nopos1-prot", -11, -1, "nopos")
    add("blosum62", *LIMIT, "limit")
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# the two refusals (SW_ERR_RANGE): an entry span past 254, and Gotoh gaps with o + e + S > 65535
REFUSED = (Case("span255", "span255-prot", -11, -1, frozenset()),
           Case("gotoh-65536", "blosum62", LIMIT[0], LIMIT[1] - 1, frozenset()))
# a family exists where a planted gap is the path: never at go = 0 (nothing to lose), under the
# nopos matrices (nothing scores), at the limit (no flank of 1,024 rows outweighs 65,524), or
# under wide-prot with free extension (a chance match is worth 127, so the model's path is a
# chain of free I runs from one chance match to the next and not the plant: its CIGARs at -8 / 0
# hold an I run every few columns)
SEAM_CASES = [c for c in CASES if c.go < 0 and not c.tags & {"nopos", "limit"}
              and c.matrix != "wide-prot"]
TIE_CASES = [c for c in CASES if c.go == 0]


def pen(case):
    return case.go, case.ge


def live_fs(case):
    """The frameshift penalty a case's family is made and measured under."""
    return -32767 if case.go <= -100 else -15


def need(case):
    """Rows each side of a planted run needs to outweigh the gap and its re-opening."""
    return (-(case.go + case.ge) - case.ge - case.go) // 4 + 20


def _seed(case, K, what):
    return [sum(ord(ch) * (k + 1) for k, ch in enumerate(case.name)), K, what]


# ---- the tiny pairs of the CPU comparison of the two restatements ---------------------------------
def tiny_pairs(case, n=24):
    """[(q, t, fs)]: m <= 7, L <= 25, as fsalign_cases.tiny_cases makes them (random queries,
    queries read off the target with steps of 2, 3 and 4 bases, planted gaps of one or two
    codons), the frameshift values in turn; an N code in one target in four (every target under
    pad-prot), so the X column is read."""
    rng = np.random.default_rng(_seed(case, 0, 3))
    out = []
    for k in range(n):
        if k % 2 == 0:  # a planted gap: D (dropped from the query), then I (put into it)
            g = 1 + (k // 2) % 2
            t = rng.integers(0, 4, int(rng.integers(21, 26))).astype(np.uint8)
            a = A.aminos(t)[int(rng.integers(0, 3))::3]
            q = a[:3] + a[3 + g:7] if k % 4 == 0 else \
                a[:3] + [int(x) for x in rng.integers(0, 20, g)] + a[3:7 - g]
        else:
            m, L = int(rng.integers(1, 8)), int(rng.integers(0, 26))
            t = rng.integers(0, 2 if k % 4 == 1 else 4, L).astype(np.uint8)
            q = [int(x) for x in rng.integers(0, 20, m)]
            if k % 8 < 6 and L >= 6:
                a, step = A.aminos(t), (2, 3, 4)[(k // 2) % 3]
                q = [a[p] for p in range(int(rng.integers(0, 3)), len(a), step)][:m]
        if len(t) and (k % 4 == 3 or case.matrix == "pad-prot"):
            t[int(rng.integers(0, len(t)))] = 4
        out.append((np.array(q, np.uint8), t, FS_VALUES[(k // 2 + k) % 4]))
    return out


# ---- the noise batch -----------------------------------------------------------------------------
def _window(rng, q, lo, hi):
    ln = min(len(q), int(rng.integers(lo, hi + 1)))
    a = int(rng.integers(0, len(q) - ln + 1))
    return q[a:a + ln]


def _shifted(rng, w, table=None):
    core = F.back_translate(rng, w, table)
    at = 3 * (len(w) // 2) + int(rng.integers(0, 3))
    if rng.random() < 0.5 or len(core) <= 3:
        return np.insert(core, at, int(rng.integers(0, 4)))
    return np.delete(core, at)


def _codon_gap(rng, w, table=None):
    """The window with one or two codons dropped (the query holds rows the target lacks: I) or
    one or two random codons put in (D), near its middle."""
    g, mid = 1 + int(rng.integers(0, 2)), len(w) // 2
    if rng.random() < 0.5 and len(w) > 2 * g + 2:
        return F.back_translate(rng, np.concatenate([w[:mid], w[mid + g:]]), table)
    return np.concatenate([F.back_translate(rng, w[:mid], table),
                           rng.integers(0, 4, 3 * g).astype(np.uint8),
                           F.back_translate(rng, w[mid:], table)])


def _flanked(rng, core, room=400):
    spare = max(0, room - len(core))
    left = rng.integers(0, 4, int(rng.integers(0, min(30, spare // 2) + 1))).astype(np.uint8)
    right = rng.integers(0, 4, int(rng.integers(0, min(30, spare // 2) + 1))).astype(np.uint8)
    return np.concatenate([left, core, right]).astype(np.uint8)[:room]


@functools.lru_cache(maxsize=None)
def noise_batch(name, K):
    """(q, seqs): 64 DNA targets of 0..400 codes for the case's query of NOISE_QLEN[K] rows."""
    case = BY_NAME[name]
    rng = np.random.default_rng(_seed(case, K, 1))
    q = rng.integers(0, 20, NOISE_QLEN[K]).astype(np.uint8)
    seqs = []
    for k in range(64):
        kind = k % 8
        if kind in (0, 4):
            t = _flanked(rng, _shifted(rng, _window(rng, q, 8, 110)))
        elif kind in (1, 5):
            t = _flanked(rng, _codon_gap(rng, _window(rng, q, 12, 110)))
        elif kind == 2:  # a shift and a codon gap
            w = _window(rng, q, 30, 110)
            t = _flanked(rng, np.concatenate([_shifted(rng, w[:len(w) // 2]),
                                              _codon_gap(rng, w[len(w) // 2:])]))
        elif kind == 6:  # one window twice: the best value lies at two cells at the least
            core = F.back_translate(rng, _window(rng, q, 6, 40))
            t = _flanked(rng, np.concatenate([core, np.full(6, 4, np.uint8), core]))
        else:
            t = rng.integers(0, 5 if kind == 7 else 4, int(rng.integers(0, 401))).astype(np.uint8)
        if kind < 7 and len(t) and k % 16 >= 8 and rng.random() < 0.5:
            t[rng.integers(0, len(t), 1 + len(t) // 100)] = 4
        seqs.append(SC.revcomp(t) if k % 2 else t)
    seqs[3], seqs[11] = np.zeros(0, np.uint8), np.array([1, 2], np.uint8)
    assert len(seqs) == 64 and max(len(t) for t in seqs) <= 400
    return q, seqs


# ---- the gap-state seams of the score walk ---------------------------------------------------------
Plant = collections.namedtuple("Plant", "target kind seam reverse mrow mcol live")


def _lane_seams(case, K):
    m, nd = SEAM_QLEN[K], need(case)
    fit = [l for l in (5, 17, 32, 47, 58) if min(l * K - 1, m - l * K - 1) >= nd]
    return fit[:3] if len(fit) > 3 else fit or [32]


def _block_seams(case):
    first = 64 * ((need(case) + 5 + 63) // 64)
    return [first, first + 64]


@functools.lru_cache(maxsize=None)
def seam_family(name, K):
    """(q, plants, tried): every plant whose model strand is the planted one, `live` where the
    score of the C model that drops the gap state at the seam (F into row mrow = K * l, E into
    codon index mcol = 64 * j of the strand walked) differs from the model's.  Kind I: the target
    lacks the query rows K * l - 1 and K * l.  Kind D: the target holds two codons the query
    lacks at the codon indices 64 j - 1 and 64 j of its strand."""
    case = BY_NAME[name]
    assert case in SEAM_CASES
    sub, fs, nd, m = matrix(case.matrix), live_fs(case), need(case), SEAM_QLEN[K]
    rng = np.random.default_rng(_seed(case, K, 2))
    q = rng.integers(0, 20, m).astype(np.uint8)
    n4 = np.full(N_FLANK, 4, np.uint8)
    plants, tried = [], 0
    for kind, seams in (("I", _lane_seams(case, K)), ("D", _block_seams(case))):
        for s in seams:
            for rev in (False, True):
                if kind == "I":
                    r = s * K
                    qs, qe = max(0, r - 1 - nd), min(m - 1, r + nd)
                    core = np.concatenate([F.back_translate(rng, q[qs:r - 1]),
                                           F.back_translate(rng, q[r + 1:qe + 1])])
                    mrow, mcol = r, -1
                else:
                    after = s - 1 - N_FLANK // 3  # codons of the plant before the run
                    qs = int(rng.integers(1, 4))
                    qe = min(m - 1, qs + after + nd)
                    if qs + after >= m - 10:
                        continue  # (the query ends before the seam)
                    core = np.concatenate([F.back_translate(rng, q[qs:qs + after]),
                                           rng.integers(0, 4, 6).astype(np.uint8),
                                           F.back_translate(rng, q[qs + after:qe + 1])])
                    mrow, mcol = -1, s
                t = np.concatenate([n4, core, n4]).astype(np.uint8)
                t = SC.revcomp(t) if rev else t
                tried += 1
                want = A.c_align(q, t, sub, case.go, case.ge, fs, ops_cap=0)[0]
                if want[0] <= 0 or bool(want[1] & F.ALIGN_REVERSE) != rev:
                    continue
                mut = A.c_mutant(q, t, sub, case.go, case.ge, fs, "A", mrow, mcol)[0]
                plants.append(Plant(t, kind, s, rev, mrow, mcol, mut[0] != want[0]))
    return q, plants, tried


def liveness():
    """{(case name, K): (tried, live, cells)}: cells = the (kind, reverse) pairs that hold a live
    plant."""
    out = {}
    for case in SEAM_CASES:
        for K in ROWS:
            _, plants, tried = seam_family(case.name, K)
            live = [p for p in plants if p.live]
            out[case.name, K] = (tried, len(live), {(p.kind, p.reverse) for p in live})
    return out


# ---- pad rows and pad columns ----------------------------------------------------------------------
EDGE_QLENS = (255, 256, 257, 1023, 1024)


@functools.lru_cache(maxsize=None)
def edge_batch(m):
    """(q, seqs): windows of the last rows of a query of m rows (so the rows past it, which the
    kernels pad, lie right below the hit) at the very end of the strand walked, followed by 0, 1
    or 2 bases, so that every L mod 3 occurs and the frames of the last codon index that run past
    the strand (the pad columns) lie right beside the hit; whole and with a shift or a dropped
    codon, on both strands, some holding N, and two random targets."""
    rng = np.random.default_rng([211, m])
    q = rng.integers(0, 20, m).astype(np.uint8)
    seqs = []
    for k in range(18):
        w = q[m - int(rng.integers(20, 70)):]
        core = (F.back_translate(rng, w), _shifted(rng, w), _codon_gap(rng, w))[k // 6]
        t = np.concatenate([rng.integers(0, 4, int(rng.integers(3, 40))).astype(np.uint8), core])
        while len(t) % 3 != k % 3:
            t = np.concatenate([t, rng.integers(0, 4, 1).astype(np.uint8)])
        if k % 6 == 5:
            t[int(rng.integers(0, len(t)))] = 4
        seqs.append(SC.revcomp(t) if (k // 3) % 2 else t)
    seqs += [rng.integers(0, 5, 200 + r).astype(np.uint8) for r in (0, 1)]
    assert {len(t) % 3 for t in seqs} == {0, 1, 2}
    return q, seqs


# ---- the seeded fuzz -------------------------------------------------------------------------------
FUZZ_QLENS = (1, 4, 5, 64, 255, 256, 257, 513, 1024)


def fuzz_case(seed):
    """(sub, go, ge, fs, table, q, seqs): a random 24 x 24 int8 matrix of span <= 254, not
    symmetric; go in [-20, 0], ge in [-5, 0]; fs from {0, -1 .. -30, -32767}; the standard or the
    custom codon table; 1..80 targets of 0..600 codes, one in four a window of the query with a
    shift or a codon gap, N in some."""
    rng = np.random.default_rng([223, seed])
    lo = int(rng.choice([-128, -127, -60, -12, -8]))
    hi = int(rng.integers(max(lo + 1, 1), min(lo + 254, 127) + 1))
    sub = rng.integers(lo, hi + 1, (24, 24)).astype(np.int8)
    sub[np.arange(20), np.arange(20)] = rng.integers(max(1, hi // 2), hi + 1, 20)
    assert max(0, int(sub.max())) - int(sub.min()) <= 254 and (sub != sub.T).any()
    go, ge = -int(rng.integers(0, 21)), -int(rng.integers(0, 6))
    fs = int(rng.choice([0, -32767] + [-int(x) for x in rng.integers(1, 31, 4)]))
    table = F.custom_table() if rng.random() < 0.4 else None
    m = int(rng.choice(FUZZ_QLENS))
    q = rng.integers(0, 20, m).astype(np.uint8)
    seqs = []
    for k in range(int(rng.integers(1, 81))):
        if k % 4 == 0 and m >= 4:
            w = _window(rng, q, 4, 150)
            core = _shifted(rng, w, table) if rng.random() < 0.5 else _codon_gap(rng, w, table)
            t = _flanked(rng, core, 600)
            t = SC.revcomp(t) if k % 8 else t
        else:
            t = rng.integers(0, 4, int(rng.integers(0, 601))).astype(np.uint8)
        if len(t) and rng.random() < 0.25:
            t[rng.random(len(t)) < 0.03] = 4
        seqs.append(t.astype(np.uint8))
    return np.ascontiguousarray(sub), go, ge, fs, table, q, seqs


# ---- references --------------------------------------------------------------------------------------
def best_cells(q, t, sub, go, ge, fs, table=None):
    """How many cells of the winning strand's local matrix hold the score, by the C model."""
    lib = A.model_lib()
    P = ctypes.c_void_p
    lib.fsalign_best_cells.restype = ctypes.c_size_t
    lib.fsalign_best_cells.argtypes = [P, ctypes.c_size_t, P, ctypes.c_size_t, P, ctypes.c_int, P,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    q = np.ascontiguousarray(q, np.uint8)
    t = np.ascontiguousarray(t, np.uint8)
    sub = np.ascontiguousarray(sub, np.int8)
    tab = np.ascontiguousarray(F.standard_table() if table is None else table, np.uint8)
    p = FS._p
    return int(lib.fsalign_best_cells(p(q), len(q), p(t), len(t), p(sub), sub.shape[0], p(tab),
                                      go, ge, fs))


STATS_ROUNDS = 2


@functools.lru_cache(maxsize=None)
def stats_batch():
    """(q, residues, offsets, lengths): a query of 33 rows, 64 targets of 300 nt, N in some."""
    rng = np.random.default_rng(227)
    q = rng.integers(0, 20, 33).astype(np.uint8)
    seqs = [rng.integers(0, 5 if k % 8 == 7 else 4, 300).astype(np.uint8) for k in range(64)]
    return (q,) + tuple(O.pack_residues(seqs))


def stats_reference(sub, go, ge, fs, seed, rounds=STATS_ROUNDS):
    """(lambda, K, degenerate, n_samples, min_score, max_score, n_clamped) of the reference
    pipeline over stats_batch under any matrix and penalties."""
    q, res, offs, lens = stats_batch()
    per = []
    for r in range(rounds):
        shuf = ST.shuffle(res, offs, lens, seed + r)
        per.append(FS.c_search_set([q], FSS.targets_of(shuf, offs, lens), sub, go, ge, fs)[0])
    counts, sums, clamped = FSS.pool(per, lens, 1)
    lam, K, degenerate = ST.fit(counts[0], sums[0], len(q))
    occ = np.nonzero(counts[0])[0]
    return (lam, K, degenerate, int(counts[0].sum()), int(occ[0]), int(occ[-1]), int(clamped[0]))
