"""Alignment inputs under asymmetric matrices (a helper, not a test module).

include/swbank.h lets a substitution matrix be asymmetric (row = query code, column = target
code).  Under a match / mismatch table, and under BLOSUM62, s(q, c) = s(c, q), and for DNA
s(q, comp c) = s(comp q, c): an alignment kernel that read its profile transposed, or one whose
reverse-strand matrix smat'[q][c] = smat[q][comp c] complemented the wrong side, returns the
records of the right one.  The families of tests/align_cases.py cannot be built under the
asymmetric matrices of tests/seam_cases.py (their liveness is defined by seam mutants and by a
letter that is negative against two codes), so this module builds one whose liveness is defined
by matrix mutants:

1. ``matrix_family(P)``: one query of 700 codes (DNA: N at about 3 %) and 48 targets of at most
   760 codes: windows of the query of 30-650 codes with a substitution every 7th code, a third
   of them with a 1-6 code deletion or insertion near the middle (alignments over one, two and
   three 256-row strips), windows of the align_cases.boundary_case lengths {0, 1, 63, 64, 65,
   129}, and four random targets.  Deterministic in (matrix name, model).  The references are
   align_cases.prepare's: brute_batch (score and coordinates) and ref_paths (the ops).
   ``col0_family()`` is the same construction with targets of 1-200 codes at the merged
   penalties 3 / -3 / -1 / -1, where max(s) > open + extend and the first-column rule is alive;
   it carries scores only (see the comment above it).

2. The mutants.  ``forward_mutants``: the transposed matrix.  ``reverse_mutants``: what a strand
   kernel computes that builds smat' wrongly: from the matrix uncomplemented, with the rows
   complemented, from the transposed matrix, with both sides complemented.  Each is given as the
   matrix it amounts to on (query, forward family target), so the numpy model scores it.
   ``mutant_share``: the share of a group's positive hits whose score a mutant changes;
   ``mutant_moved``: how many records' coordinates or ops it changes (over the shorter hits).

3. ``strand_form``: the family as a strand call sees it: alternating strands, a reverse hit's
   stored target being rc(t) (its expected record is the forward one through
   strand_cases.flip_record); ``set_form``: the family as a set of three queries.

4. ``frame_case``: the protein matrix through the reading frames: windows of protein queries
   with a substitution every 7th residue, back-translated and planted in a chosen frame of DNA
   targets of at most 3,000 codes; ``stop_x_table``: a genetic code with two more stop codons
   and a codon for X, so that rows and columns 22 / 23 of the matrix are read.

Measured on the CPU by tests/test_align_cases.py, tests/test_strand_cases.py and
tests/test_frame_cases.py (the share of the positive hits whose score the mutant changes; the
tests assert >= 80 % for each; in brackets the records, of the hits of at most 140 codes, whose
coordinates or ops it changes; model 0 merged, 1 Gotoh):

    matrix / model   forward      reverse: the wrong smat' is built
                     transposed   no-complement  rows        transposed  both-sides
    asym-pair / 0     96 % (6)    100 % (12)    100 % (5)    96 % (6)    96 % (12)
    asym-pair / 1     98 % (3)     98 % (12)    100 % (5)    98 % (3)    98 % (12)
    asym-ncol / 0     94 % (6)    100 % (12)     98 % (5)    94 % (6)    98 % (12)
    asym-ncol / 1     96 % (3)    100 % (12)    100 % (5)    96 % (3)    98 % (12)
    asym-odd  / 0     98 % (3)    100 % (11)     98 % (4)    98 % (3)   100 % (11)
    asym-odd  / 1     96 % (3)     98 % (12)     96 % (3)    96 % (3)    98 % (12)
    asym-prot / 0     98 % (4)
    asym-prot / 1     98 % (6)

(The reverse "transposed" mutant amounts to the transposed matrix on the forward target, so its
figures are the forward ones.)  Frames (frame_case; planted targets whose frame score the
transposed matrix changes): standard table 27 of 27 under both models, stop_x_table 25 of 27
merged and 27 of 27 Gotoh.  col0_family: 15 of the 24 reverse hits need the first column, the
first-column rule is alive on 7 (the test asserts a quarter for each).
"""
import numpy as np

from oracle import oracle as O

import align_cases as C
import frame_cases as F
import seam_cases as SC
import strand_cases as ST

COMP = np.array([2, 3, 0, 1, 4])  # T <-> A, C <-> G, N stays
MATRIX_SETS = {"asym-pair": (-12, -4), "asym-ncol": (-12, -4), "asym-odd": (-14, -3),
               "asym-prot": (-11, -1)}
PROTEIN = "asym-prot"
PARAMS = [(name, model) for name in MATRIX_SETS for model in C.MODELS]  # the eight sets
DNA_PARAMS = [(name, model) for name, model in PARAMS if name != PROTEIN]
QLEN, N_TARGETS, MAX_TLEN = 700, 48, 760
WINDOW = (30, 650)
BOUNDARY_LENS = (0, 1, 63, 64, 65, 129)  # align_cases.TLENS' lane and block edges
SHORT = 140  # mutant_moved looks at the hits of at most this many codes


def matrix_param(name, model):
    go, ge = MATRIX_SETS[name]
    return C.Param(name, 24 if name == PROTEIN else 4, SC.MATRICES[name](), go, ge, model)


def col0_param():
    """Merged gaps with max(s) = 3 > open + extend = 2 (tests/test_gpu_queries.py's "col0")."""
    return C.Param("col0", 4, O.dna_matrix(3, -3), -1, -1, C.GAP_MERGED)


# ---------------------------------------------------------------------------------------
# 1. the family
def _window(P, rng, q, ln, indel, flanks, skip_second=False):
    """A window of q of ln codes with a substitution every 7th code, an indel of 1-6 codes
    within 4 codes of its middle (indel: None | "del" | "ins"), in random flanks.  skip_second:
    the window's second code is left out (see col0_family)."""
    A = P.sub.shape[0]
    skip_second = skip_second and ln >= 8
    for _ in range(64):
        a = int(rng.integers(0, len(q) - ln + 1))
        # pinned: the skipped code differs from its neighbours, so the one-row gap cannot slide
        if not skip_second or (q[a + 1] != q[a] and q[a + 1] != q[a + 2]):
            break
    core = q[a:a + ln].astype(np.int64)
    # (a substitution within a few codes of the skipped one would outweigh the gap: CPU probe,
    # 8 of 24 pinned windows live with the first substitution at code 3, 23 of 24 at code 10)
    pos = np.arange(10 if skip_second else 3, ln, 7)
    core[pos] = (core[pos] + 1 + rng.integers(0, A - 1, len(pos))) % A
    core = [int(c) for c in core]
    if indel:
        g, at = int(rng.integers(1, 7)), ln // 2 + int(rng.integers(-4, 5))
        if indel == "del":
            del core[at:at + g]
        else:
            core[at:at] = [int(c) for c in rng.integers(0, P.letters, g)]
    if skip_second:
        del core[1]
    left, right = (rng.integers(0, P.letters, n) for n in flanks)
    return np.concatenate([left, np.array(core, np.int64), right]).astype(np.uint8)


def _targets(P, rng, q, window, noise_lens, flank=8, skip_second=False):
    """48 targets: 38 windows (13 with an indel, those of at least 100 codes), the boundary
    lengths, four random ones; shuffled.  Every other window has no left flank: the target
    starts with it.  skip_second (col0_family): no window has one, and every other window loses
    its second code.  meta[k] = (kind, window length): kind "plain" | "del" | "ins" | "edge" |
    "noise"."""
    lo, hi = window
    gapped = np.linspace(max(lo, min(100, hi // 2)), hi, 13).astype(int)
    plain = np.linspace(lo, hi - 10, 25).astype(int)
    out = [(("del", "ins")[k % 2], int(ln)) for k, ln in enumerate(gapped)]
    out += [("plain", int(ln)) for ln in plain]
    out += [("edge", ln) for ln in BOUNDARY_LENS]
    seqs, meta = [], []
    for kind, ln in out:
        first = len(seqs) % 2 == 1 or kind == "edge" or skip_second
        fl = (0 if first else int(rng.integers(0, flank + 1)),
              int(rng.integers(0, flank + 1)))
        if kind == "edge":
            fl = (0, 0)  # the boundary lengths are the targets' lengths
        seqs.append(_window(P, rng, q, ln, kind if kind in ("del", "ins") else None, fl,
                            skip_second and len(seqs) % 2 == 1 and kind != "edge"))
        meta.append((kind, ln))
    for ln in noise_lens:
        seqs.append(rng.integers(0, P.sub.shape[0], ln).astype(np.uint8))
        meta.append(("noise", ln))
    order = [int(k) for k in rng.permutation(len(seqs))]
    return [seqs[k] for k in order], [meta[k] for k in order]


def _inputs(P, window, noise_lens, max_len, **kw):
    rng = np.random.default_rng([29, sum(ord(ch) for ch in P.tag), P.model])
    q = rng.integers(0, P.letters, QLEN).astype(np.uint8)
    if P.letters == 4:
        q[rng.random(QLEN) < 0.03] = 4
    seqs, meta = _targets(P, rng, q, window, noise_lens, **kw)
    assert len(seqs) == N_TARGETS and max(len(t) for t in seqs) <= max_len
    assert {len(t) for t in seqs} >= set(BOUNDARY_LENS)
    return q, seqs, meta


def matrix_family(P):
    """Group of one parameter set of PARAMS (see the module's text)."""
    def make():
        q, seqs, meta = _inputs(P, WINDOW, (45, 210, 480, MAX_TLEN), MAX_TLEN)
        brute, refs = C.prepare(q, seqs, P)
        return C.Group(f"matrix-{P.tag}-{P.model}", q, seqs, list(range(N_TARGETS)), brute, refs,
                       meta)
    return C._cached(("matrix", P.tag, P.model), make)


# The first-column rule of the merged model (oracle/sw_oracle.c: in a target's first column the
# gap value takes ZERO for its neighbours) bites where max(s) > open + extend: a match in the
# first column cannot be followed by a query-only gap.  It is the one rule that is not
# reversal-symmetric, so under col0_param():
# - the start rule of include/swbank.h (the end rule on the reversed prefixes) has no reversed
#   problem that scores what the pair scores (align_check.brute_ends_batch asserts it, and does
#   for this family; tests/test_strand_cases.py shows it), the alignment entries refuse these
#   penalties with SW_ERR_UNSUPPORTED, and there are no alignment records to expect;
# - the scores are defined, and a reverse hit's first column is the stored target's last code.
# So the col0 family carries scores only.  Its windows without a left flank also lose their
# second code: the first code then matches in the first column, a one-row gap follows, and the
# rule (the target's own first column) and its mirror image (the rule applied at the target's
# last column, which is what scoring rc(query) against the stored target amounts to) differ.
def col0_family():
    """Group (brute and refs None) of the construction at col0_param(), targets of 1-200 codes
    (and the empty one).  meta = (per-target kinds, forward oracle scores of q against the
    family targets, the mirror-image scores, touches) with touches[k] True when leaving out
    target k's first code lowers its score: every optimal alignment then uses the first column."""
    def make():
        P = col0_param()
        q, seqs, meta = _inputs(P, (1, 178), (20, 77, 150, 200), 200, skip_second=True)
        args = (P.sub, P.go, P.ge, P.model)
        want = SC.oracle_scores(O, q, seqs, *args)
        assert SC.scores_with_cut(q, seqs, *args).tolist() == want.tolist()
        mirror = SC.oracle_scores(O, q[::-1].copy(), [t[::-1].copy() for t in seqs], *args)
        less = SC.oracle_scores(O, q, [t[1:] for t in seqs], *args)
        return C.Group("col0", q, seqs, list(range(N_TARGETS)), None, None,
                       (meta, want, mirror, less < want))
    return C._cached("col0", make)


# ---------------------------------------------------------------------------------------
# 2. the mutants
def forward_mutants(sub):
    return {"transposed": np.ascontiguousarray(np.asarray(sub).T)}


def reverse_mutants(sub):
    """{name: matrix}: a strand kernel reads stored code c = comp(t) and scores it with
    smat'[q][c]; the right smat' is sub[:, COMP].  Each wrong smat' is returned as the matrix it
    amounts to on (q, t): smat'[:, COMP]."""
    sub = np.asarray(sub)
    assert sub.shape == (5, 5)
    wrong = {"no-complement": sub, "rows": sub[COMP], "transposed": sub.T[:, COMP],
             "both-sides": sub[COMP][:, COMP]}
    assert np.array_equal(sub[:, COMP][:, COMP], sub)
    return {k: np.ascontiguousarray(m[:, COMP]) for k, m in wrong.items()}


def positive(g):
    return [h for h in g.hits if g.brute[h][0] > 0]


def mutant_share(g, P, sub2):
    """The share of the group's positive hits whose score the matrix sub2 changes (the numpy
    model of seam_cases.scores_with_cut; with the right matrix it is the brute-force score)."""
    def make():
        live = positive(g)
        ts = [g.seqs[h] for h in live]
        base = SC.scores_with_cut(g.q, ts, P.sub, P.go, P.ge, P.model)
        assert base.tolist() == [g.brute[h][0] for h in live], "the model is the oracle"
        got = SC.scores_with_cut(g.q, ts, sub2, P.go, P.ge, P.model)
        return float((got != base).mean())
    return C._cached(("share", g.name, np.asarray(sub2, np.int8).tobytes()), make)


def mutant_moved(g, P, sub2):
    """How many of the positive hits of at most SHORT codes get other coordinates or other ops
    under sub2 (brute force and the reference traceback under the mutant)."""
    def make():
        ks = [h for h in positive(g) if len(g.seqs[h]) <= SHORT]
        brute, refs = C.prepare(g.q, [g.seqs[h] for h in ks], P._replace(sub=sub2))
        return sum(1 for h, b, r in zip(ks, brute, refs)
                   if b[1:] != g.brute[h][1:] or (r.ops if r else ()) != g.refs[h].ops)
    return C._cached(("moved", g.name, np.asarray(sub2, np.int8).tobytes()), make)


# ---------------------------------------------------------------------------------------
# 3. the strand form
def strand_form(g):
    """(stored targets, strands [n]): odd targets are reverse hits, stored as rc(t)."""
    strands = np.arange(len(g.seqs), dtype=np.uint8) % 2
    return [ST.revcomp(t) if s else t for t, s in zip(g.seqs, strands)], strands


SET_HITS = 90
SET_NONE = {7: "query", 40: "target", 41: "both"}  # sentinel slots of the set form's hit list


def set_form(g):
    """The family as a set call sees it: (queries, hit_queries, hits): the 700-row query, its
    rows 100-400 and a 40-row piece; hit h pairs query h % 3 with target (5 (h // 3) + 16 (h % 3))
    % 48 (the queries interleave, every query meets 30 different targets), SET_NONE's slots name
    no pair."""
    queries = [g.q, g.q[100:400].copy(), g.q[330:370].copy()]
    hq = np.array([h % 3 for h in range(SET_HITS)], np.uint32)
    hv = np.array([(5 * (h // 3) + 16 * (h % 3)) % len(g.seqs) for h in range(SET_HITS)],
                  np.uint64)
    for h, kind in SET_NONE.items():
        if kind in ("query", "both"):
            hq[h] = 0xFFFFFFFF
        if kind in ("target", "both"):
            hv[h] = 0xFFFFFFFFFFFFFFFF
    return queries, hq, hv


# ---------------------------------------------------------------------------------------
# 4. the frames
FRAME_QLENS = (300, 90)
FRAME_TARGETS = 36
FRAME_MAX = 3000


def stop_x_table():
    """The standard code with CTG and ATA as two more stops and GGG as X."""
    tab = F.standard_table().copy()
    tab[[19, 34]] = F.STOP
    tab[63] = F.X
    assert F.STANDARD_CODE[19] == "L" and F.STANDARD_CODE[34] == "I" and F.STANDARD_CODE[63] == "G"
    return tab


def frame_case(table=None):
    """(queries, DNA targets, planted): two protein queries (with the custom table: X and *
    codes among their letters), FRAME_TARGETS targets of at most FRAME_MAX codes; target k with
    k % 4 != 3 holds the back-translation of a window of query k % 2 with a substitution every
    7th residue (every third one with a 1-3 residue deletion) in frame k % 6, the rest are
    random (N codes among them).  planted = {k: (query, frame)}."""
    def make():
        custom = table is not None
        rng = np.random.default_rng([31, int(custom)])
        qs = [rng.integers(0, 20, n).astype(np.uint8) for n in FRAME_QLENS]
        if custom:
            for q in qs:
                q[5::17] = F.X
                q[11::23] = F.STOP
        seqs, planted = [], {}
        for k in range(FRAME_TARGETS):
            if k % 4 == 3:
                L = int(rng.integers(0, FRAME_MAX + 1)) if k != 3 else 2
                seqs.append(rng.integers(0, 5 if k % 8 == 7 else 4, L).astype(np.uint8))
                continue
            q = qs[k % 2]
            ln = int(rng.integers(len(q) // 3, len(q) + 1))
            a = int(rng.integers(0, len(q) - ln + 1))
            w = q[a:a + ln].astype(np.int64)
            pos = np.arange(3, ln, 7)
            w[pos] = (w[pos] + 1 + rng.integers(0, 19, len(pos))) % 20
            w = [int(c) for c in w]
            if k % 3 == 0:
                at = ln // 2
                del w[at:at + int(rng.integers(1, 4))]
            L = int(rng.integers(3 * len(w) + 2, FRAME_MAX + 1))
            t, f = F.plant(rng, np.array(w, np.uint8), L, k % 3, k % 6 >= 3, table)
            seqs.append(t)
            planted[k] = (k % 2, f)
        assert max(len(t) for t in seqs) <= FRAME_MAX
        assert {f for _, f in planted.values()} == set(range(6))
        return qs, seqs, planted
    return C._cached(("frames", table is not None), make)


def frame_oracle(table, model, sub=None):
    """(merged [nq, n], frames [nq, n]) of frame_case(table) by the oracle on the model's
    translations under asym-prot (or `sub`) at -11 / -1."""
    def make():
        qs, seqs, _ = frame_case(table)
        m = SC.MATRICES[PROTEIN]() if sub is None else sub
        per = [F.merge6(F.oracle_frames(q, seqs, m, MATRIX_SETS[PROTEIN], model, table))
               for q in qs]
        return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
    if sub is not None:
        return make()
    return C._cached(("frame-oracle", table is not None, model), make)
