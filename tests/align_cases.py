"""Inputs and the reference traceback of the alignment-pass tests (a helper, not a test module).

The alignment kernels (csrc/swbank_kalign.hip) run one walk in three coordinate systems: pass A
over q[0..), pass B over the reversed prefixes q[q_end..0] x t[t_end..0], pass C over the window
from (q_start, t_start); pass D indexes the direction store by window row.  Each pass has its
own 256-row strip seams, 4-row lanes and 64-column blocks.  This module builds inputs whose gaps
and ties lie at those places in every one of the three systems, and the model that says what
the CIGAR must be:

1. ``ref_path`` / ``ref_paths``: an int64 numpy model of the CIGAR rule of include/swbank.h and
   of the header comment of swbank_kalign.hip (the specification; the kernel's code is not): an
   anchored DP over the window (only the window's first cell starts a path, no local floor) and
   the walk back from the end cell.  Gotoh: H prefers the diagonal, then E (left, D), then F
   (above, I); E and F open rather than extend.  Merged: H prefers M over the gap value, the gap
   comes from the left before from above, and at the source cell the gap opened from that
   cell's M unless extending is strictly better.  It returns the ops and, per kind, the number
   of path cells at which two moves were co-optimal (``dg`` diagonal / gap, ``lu`` left / up,
   ``oe`` open / extend).  The anchored value at the end cell must equal the brute-force score.

2. Families of inputs, every one checked by CPU conditions when it is built (a family that
   cannot meet them raises; nothing is dropped silently):
   a. ``seam_family``: one vertical (query-only, I) run over a strip seam of pass A, pass C or
      pass B; kept only if the gap-dropping mutant (seam_cases.scores_with_cut) on that pass's
      problem changes the score and the reference path has an I run over the seam.  Pass B
      shows only in the start it reports: its "Bt" targets start so few letters before the run
      that the mutant's best cell is another one (tight_rows).
   b. ``edge_family``: windows of exactly 255 .. 513 rows and of exactly 63 .. 129 columns with
      an indel within 8 cells of the last row or column.
   c. ``tie_family``: equal maximal cells in different lanes and strips (end rule) and equal
      starts in different lanes and strips (start rule).
   d. ``tie_rich_family``: low-complexity sequences at penalties where co-optimal moves are
      common.
   ``reuse_case``: the hit lists that make a wave align several hits in turn.

Free extension (open -8, extend 0) is left out of families a-c: FREE_EXTENSION_LEFT_OUT.
"""
import collections
import math

import numpy as np

from oracle import oracle as O

import align_check as AC
import seam_cases as SC

GAP_MERGED, GAP_GOTOH = 0, 1
MODELS = [GAP_MERGED, GAP_GOTOH]
REF = (5, -4, -12, -4)
ALT = (5, -4, -10, -1)   # merged differs from Gotoh: gaps that turn the corner occur
DNA_SETS = {"ref": REF, "alt": ALT}
# The one named omission: with a free extension a gap run costs its opening however long it is,
# so the local window floats off the planted one and no target of families a-c keeps a gap over
# a chosen row (CPU probe: 0 of 45 seam targets live).  The score kernels' seam tests cover it.
FREE_EXTENSION_LEFT_OUT = ("free", (5, -4, -8, 0))
# Tie-rich penalties (merged: max(s) <= open + extend).  At the second set a mismatch costs more
# than an I and a D, so paths turn corners and the gap from the left ties with the one from above.
TIE_SETS = {"m4o4": (4, -4, -4, -4), "m4x12o0": (4, -12, 0, -4)}
_NEG = -(1 << 40)
_CLIP = -(1 << 30)
_CACHE = {}

Param = collections.namedtuple("Param", "tag letters sub go ge model")
Ref = collections.namedtuple("Ref", "ops n_columns n_identities ties")
Group = collections.namedtuple("Group", "name q seqs hits brute refs meta")


def dna_param(tag, model, sets=DNA_SETS):
    ma, mi, go, ge = sets[tag]
    return Param(tag, 4, O.dna_matrix(ma, mi), go, ge, model)


def protein_param():
    return Param("blosum62", 20, O.BLOSUM62, -11, -1, GAP_GOTOH)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------
# 1. the reference traceback
def _anchored(S, go, ge, model):
    """The anchored matrices of a batch of window substitution tensors S [B, m, n], computed in
    int64 and kept as int32 (values below -2^30, "no path", clipped): Gotoh (H, E, F), merged
    (M, I).  Cell (0, 0) alone has a 0 diagonal; there is no floor."""
    B, m, n = S.shape
    S = S.astype(np.int64)
    col = np.arange(n, dtype=np.int64)
    out = [np.empty((B, m, n), np.int32) for _ in range(3 if model == GAP_GOTOH else 2)]
    neg = np.full((B, 1), _NEG, np.int64)
    Hp = np.full((B, n), _NEG, np.int64)
    Xp = np.full((B, n), _NEG, np.int64)  # Gotoh: F of the row above; merged: T
    for i in range(m):
        diag = np.concatenate([neg if i else np.zeros((B, 1), np.int64), Hp[:, :-1]], axis=1)
        if model == GAP_GOTOH:
            F = np.maximum(Hp + go + ge, Xp + ge)
            Ht = np.maximum(diag + S[:, i, :], F)  # H without E (an E-derived H opens no better E)
            E = np.full((B, n), _NEG, np.int64)
            if n > 1:
                acc = np.maximum.accumulate(Ht - ge * col, axis=1)
                E[:, 1:] = acc[:, :-1] + go + ge * col[1:]
            H = np.maximum(Ht, E)
            for dst, src in zip(out, (H, E, F)):
                dst[:, i, :] = np.maximum(src, _CLIP)
            Hp, Xp = H, F
        else:
            M = diag + S[:, i, :]
            a = Xp.copy()  # I(j) = max(T above, M(j-1) - o - e, I(j-1) - e)
            if n > 1:
                a[:, 1:] = np.maximum(a[:, 1:], M[:, :-1] + go + ge)
            I = np.maximum.accumulate(a - ge * col, axis=1) + ge * col
            for dst, src in zip(out, (M, I)):
                dst[:, i, :] = np.maximum(src, _CLIP)
            Hp, Xp = np.maximum(M, I), np.maximum(M + go + ge, I + ge)
    return out


def _emit(ops, code):
    if ops and ops[-1][1] == code:
        ops[-1][0] += 1
    else:
        ops.append([1, code])


def _walk_gotoh(H, E, F, S, go, ge):
    """Ops (backwards) and tie counts of the walk from the last cell of H to cell (0, 0)."""
    i, j = H.shape[0] - 1, H.shape[1] - 1
    ops, ties, state = [], {"dg": 0, "lu": 0, "oe": 0}, "H"
    for _ in range(H.shape[0] + H.shape[1] + 2):
        if state == "H":
            up = int(H[i - 1, j - 1]) if i and j else 0 if i == 0 and j == 0 else _CLIP
            d, e, f, h = up + int(S[i, j]), int(E[i, j]), int(F[i, j]), int(H[i, j])
            assert h == max(d, e, f) and h > _CLIP // 2, (i, j, h, d, e, f)
            if d == h:
                ties["dg"] += max(e, f) == h
                _emit(ops, AC.M)
                if i == 0 and j == 0:
                    return ops, ties
                i, j = i - 1, j - 1
            else:
                ties["lu"] += e == f
                state = "E" if e == h else "F"
        elif state == "E":
            _emit(ops, AC.D)
            opens, extends = int(H[i, j - 1]) + go + ge, int(E[i, j - 1]) + ge
            assert j > 0 and int(E[i, j]) == max(opens, extends)
            ties["oe"] += opens == extends
            state = "H" if opens >= extends else "E"
            j -= 1
        else:
            _emit(ops, AC.I)
            opens, extends = int(H[i - 1, j]) + go + ge, int(F[i - 1, j]) + ge
            assert i > 0 and int(F[i, j]) == max(opens, extends)
            ties["oe"] += opens == extends
            state = "H" if opens >= extends else "F"
            i -= 1
    raise AssertionError("the walk did not reach the window's first cell")


def _walk_merged(M, I, go, ge):
    i, j = M.shape[0] - 1, M.shape[1] - 1
    ops, ties, state = [], {"dg": 0, "lu": 0, "oe": 0}, "H"

    def T(r, c):  # the gap value that leaves cell (r, c)
        return max(int(M[r, c]) + go + ge, int(I[r, c]) + ge) if r >= 0 and c >= 0 else _NEG

    for _ in range(2 * (M.shape[0] + M.shape[1]) + 2):
        if state == "H":
            m, g = int(M[i, j]), int(I[i, j])
            assert max(m, g) > _CLIP // 2, (i, j, m, g)
            ties["dg"] += m == g
            state = "M" if m >= g else "G"
        if state == "M":
            _emit(ops, AC.M)
            if i == 0 and j == 0:
                return ops, ties
            assert i and j, (i, j)
            i, j, state = i - 1, j - 1, "H"
        else:
            left, up = T(i, j - 1), T(i - 1, j)
            assert int(I[i, j]) == max(left, up) > _CLIP // 2, (i, j)
            ties["lu"] += left == up
            if left >= up:
                _emit(ops, AC.D)
                j -= 1
            else:
                _emit(ops, AC.I)
                i -= 1
            opens, extends = int(M[i, j]) + go + ge, int(I[i, j]) + ge
            ties["oe"] += opens == extends
            state = "G" if extends > opens else "M"
    raise AssertionError("the walk did not reach the window's first cell")


def ref_paths(q, targets, ends, sub, go, ge, model, cells=6_000_000):
    """[Ref | None] of q against every target, `ends` being brute_ends_batch's records; None
    for a pair scoring 0.  The windows are batched, `cells` matrix cells at a time."""
    q = np.asarray(q, np.uint8)
    out = [None] * len(targets)
    live = [k for k, e in enumerate(ends) if e[0] > 0]
    live.sort(key=lambda k: (ends[k][2] - ends[k][1], ends[k][4] - ends[k][3]))
    at = 0
    while at < len(live):
        n, rows, cols = 0, 0, 0
        while at + n < len(live):  # a chunk's tensor is padded to its largest window
            _, a, b, c, d = ends[live[at + n]]
            r2, c2 = max(rows, b - a + 1), max(cols, d - c + 1)
            if n and (n + 1) * r2 * c2 > cells:
                break
            n, rows, cols = n + 1, r2, c2
        chunk = live[at:at + n]
        at += n
        pairs = [(q[ends[k][1]:ends[k][2] + 1],
                  np.asarray(targets[k], np.uint8)[ends[k][3]:ends[k][4] + 1]) for k in chunk]
        S = AC._sub_tensor(pairs, sub)
        mats = _anchored(S, go, ge, model)
        for x, k in enumerate(chunk):
            qw, tw = pairs[x]
            m, n_ = len(qw), len(tw)
            sl = [a[x, :m, :n_] for a in mats]
            if model == GAP_GOTOH:
                assert int(sl[0][m - 1, n_ - 1]) == ends[k][0], ("anchored vs brute", k, ends[k])
                back, ties = _walk_gotoh(sl[0], sl[1], sl[2], S[x], go, ge)
            else:
                assert max(int(sl[0][m - 1, n_ - 1]), int(sl[1][m - 1, n_ - 1])) == ends[k][0], \
                    ("anchored vs brute", k, ends[k])
                back, ties = _walk_merged(sl[0], sl[1], go, ge)
            ops = tuple(ln << 4 | code for ln, code in reversed(back))
            _, dq, dt, cols, idn = AC.rescore(ops, qw, tw, 0, 0, sub, go, ge, model)
            assert (dq, dt) == (m, n_), ("the reference path spans the window", k)
            out[k] = Ref(ops, cols, idn, ties)
    return out


def ref_path(q, t, sub, go, ge, model, ends=None):
    """Ref of one pair (None when it scores 0); `ends` defaults to brute_ends."""
    if ends is None:
        ends = AC.brute_ends(O, q, t, sub, go, ge, model)
    return ref_paths(q, [t], [ends], sub, go, ge, model)[0]


def brute_batch(q, seqs, P, chunk=12):
    """brute_ends_batch in chunks of similar length (its matrices are padded to the longest)."""
    order = sorted(range(len(seqs)), key=lambda k: len(seqs[k]))
    out = [None] * len(seqs)
    for at in range(0, len(order), chunk):
        ks = order[at:at + chunk]
        for k, e in zip(ks, AC.brute_ends_batch(O, q, [seqs[k] for k in ks], P.sub, P.go, P.ge,
                                                P.model)):
            out[k] = e
    return out


def prepare(q, seqs, P):
    """(brute, refs) of a batch."""
    brute = brute_batch(q, seqs, P)
    return brute, ref_paths(q, seqs, brute, P.sub, P.go, P.ge, P.model)


def runs_of(ops, code):
    """[(first, last + 1)] in window rows (I) or window columns (D) of the runs of `code`."""
    i = j = 0
    out = []
    for op in ops:
        ln, c = op >> 4, op & 15
        if c == code:
            out.append((i, i + ln) if code == AC.I else (j, j + ln))
        if c != AC.D:
            i += ln
        if c != AC.I:
            j += ln
    return out


# ---------------------------------------------------------------------------------------
# 2. inputs
def _unlike(rng, P, *codes):
    """A letter that scores below 0 against every one of `codes`."""
    ok = [x for x in range(P.letters) if all(int(P.sub[int(c)][x]) < 0 for c in codes)]
    assert ok, codes
    return ok[int(rng.integers(0, len(ok)))]


def _flanks(rng, P, q, s, e, n=None, also=()):
    """Random letters that cannot extend the diagonal through q[s..e): left[-1-k] is unlike
    q[s-1-k], right[k] unlike q[e+k]; `also` lists further (s, e) to keep clear of.  n None:
    FLANK[0]..FLANK[1] letters on either side."""
    spans = [(s, e)] + list(also)
    if n is None:
        a, b = (int(x) for x in rng.integers(FLANK[0], FLANK[1] + 1, 2))
        left, _ = _flanks(rng, P, q, s, e, a, also)
        return left, _flanks(rng, P, q, s, e, b, also)[1]
    left = [_unlike(rng, P, *[q[a - 1 - k] for a, _ in spans if a - 1 - k >= 0])
            for k in range(n)][::-1]
    right = [_unlike(rng, P, *[q[b + k] for _, b in spans if b + k < len(q)]) for k in range(n)]
    return np.array(left, np.uint8), np.array(right, np.uint8)


# ---- a. pass-seam straddles ----------------------------------------------------------------
SEAM_QLEN, SEAM_WINDOW = 700, (37, 650)
# Flanks are short (2-8 random letters, none of which continues the window's diagonal): with
# cheap gaps (ALT) a longer random flank offers a few matching letters behind a gap often enough
# to move the window, and with it the seams of passes B and C, off the planted run.
FLANK = (2, 8)
SEAM_RUNS = (9, 13)  # runs over two and three whole lanes, beside the 2-6-row ones


def seam_rows(s=SEAM_WINDOW[0], e=SEAM_WINDOW[1]):
    """{(pass, seam): query row c}: the seam of that pass lies between query rows c - 1 and c
    (pass B walks down the query, so its reversed rows 255 | 256 are query rows c | c - 1)."""
    return {("A", 256): 256, ("A", 512): 512, ("C", 256): s + 256, ("C", 512): s + 512,
            ("B", 256): e - 1 - 255, ("B", 512): e - 1 - 511}


# Pass B returns no score, only where its best cell lies.  A pass B that loses the gap value at a
# seam still finds the start if what lies beyond the run (towards the start) outweighs opening
# the gap again.  "Bt" targets are pass-B targets whose window starts so few letters before the
# run that it does not: the letters before the run score more than the run costs (the gap is
# taken) but no more than the run and another opening, so the mutant's best cell is the one
# after the run, and q_start and t_start change.
def tight_rows(e=SEAM_WINDOW[1]):
    return {("Bt", 256): e - 1 - 255, ("Bt", 512): e - 1 - 511}


def _pass_rows(pas, lo, hi, qs, qe):
    """Rows [lo, hi) of the query in the pass's own row numbers."""
    return (lo, hi) if pas == "A" else (lo - qs, hi - qs) if pas == "C" else (qe - hi + 1,
                                                                               qe - lo + 1)


def _tight_start(q, P, lo, g):
    """The row at which a window must start for the letters [start, lo) before a g-row run to
    score more than the run costs and at most the run and another opening; None if no row does."""
    cost, x = -(P.go + g * P.ge), 0
    for s in range(lo - 1, lo - 12, -1):
        x += int(P.sub[q[s]][q[s]])
        if x > cost:
            return s if x <= cost - P.go else None
    return None


def _seam_candidates(q, P, rng):
    s, e = SEAM_WINDOW
    assert s % 4 and len({c % 256 for c in seam_rows().values()}) == 3
    out, made = [], collections.Counter()
    for (pas, seam), c in list(seam_rows().items()) + list(tight_rows().items()):
        for g, a in [(g, a) for a in range(1, 13) for g in (2, 3, 4, 5, 6) + SEAM_RUNS if a < g]:
            kind = (pas, seam, g if g > 6 else "short")
            if (pas in ("A", "Bt") and g > 6) or made[kind] >= (7 if g <= 6 else 5):
                continue  # (more candidates than a seam keeps: some are not live)
            lo, hi = c - a, c - a + g
            if g <= 6 and (q[lo] == q[hi] or q[lo - 1] == q[hi - 1]):
                continue  # pinned: the run cannot slide off the seam (a long one may slide)
            plo, phi = _pass_rows(pas, lo, hi, s, e - 1)
            if g > 6 and phi // 4 - -(-plo // 4) < g // 4:
                continue  # the long runs cover g // 4 whole lanes of their pass
            first = s if pas != "Bt" else _tight_start(q, P, lo, g)
            if first is None:
                continue
            left, right = _flanks(rng, P, q, first, e)
            made[kind] += 1
            out.append((np.concatenate([left, q[first:lo], q[hi:e], right]).astype(np.uint8),
                        (pas, seam, g)))
    return out


def _seam_live(q, seqs, meta, brute, refs, P):
    """Per target: the mutant of its pass changes its score, and the reference path has an I run
    over the seam (both in the pass's own rows of the brute-force window).  A "Bt" target's
    mutant must also score what the window after the run scores, less than the pair: its best
    cell is then no farther than the cell after the run, and the start it reports is wrong."""
    live = [False] * len(seqs)
    jobs = collections.defaultdict(list)  # (pass, query rows, seam) -> targets
    for k, (pas, seam, g) in enumerate(meta):
        sc, qs, qe, ts, te = brute[k]
        if sc <= 0 or refs[k] is None:
            continue
        spans = [_pass_rows(pas, qs + a, qs + b, qs, qe) for a, b in runs_of(refs[k].ops, AC.I)]
        # rows seam - 1 and seam both in the run; a long run covers g // 4 whole lanes
        if any(lo < seam < hi and (g <= 6 or hi // 4 - -(-lo // 4) >= g // 4) for lo, hi in spans):
            jobs[(pas, qs, qe, seam)].append(k)
    for (pas, qs, qe, seam), ks in jobs.items():
        if pas == "A":
            qq, tt = q, [seqs[k] for k in ks]
        elif pas == "C":
            qq, tt = q[qs:qe + 1], [seqs[k][brute[k][3]:brute[k][4] + 1] for k in ks]
        else:
            qq = q[qs:qe + 1][::-1]
            tt = [seqs[k][brute[k][3]:brute[k][4] + 1][::-1] for k in ks]
        whole = SC.scores_with_cut(qq, tt, P.sub, P.go, P.ge, P.model)
        assert whole.tolist() == [brute[k][0] for k in ks], "the model without a cut is the oracle"
        cut = SC.scores_with_cut(qq, tt, P.sub, P.go, P.ge, P.model, cut_row=seam)
        for k, a, b in zip(ks, whole, cut):
            live[k] = bool(a != b)
            if pas == "Bt":
                n, hi = runs_of(refs[k].ops, AC.I)[0]
                after = O.score_pair(q[qs + hi:qe + 1], seqs[k][brute[k][3] + n:brute[k][4] + 1],
                                     P.sub, P.go, P.ge, P.model)
                live[k] = bool(b == after < a)
    return live


def seam_family(P):
    """Group of family a for one parameter set: per (pass B | C, seam 256 | 512) four targets
    with a 2-6-row run and one each with a 9- and a 13-row run, two per forward seam, and two
    per seam of pass B whose window starts just before the run ("Bt", see tight_rows); every one
    live (see _seam_live).  meta[k] = (pass, seam, run length)."""
    def make():
        err = None
        for attempt in range(16):
            rng = np.random.default_rng([len(P.tag), P.letters, P.model, attempt])
            q = rng.integers(0, P.letters, SEAM_QLEN).astype(np.uint8)
            cand = _seam_candidates(q, P, rng)
            seqs, meta = [t for t, _ in cand], [m for _, m in cand]
            brute, refs = prepare(q, seqs, P)
            live = _seam_live(q, seqs, meta, brute, refs, P)
            keep, count = [], collections.Counter()
            for k, (pas, seam, g) in enumerate(meta):
                kind = (pas, seam, "short" if g <= 6 else g)
                want = 1 if g > 6 else 2 if pas in ("A", "Bt") else 4
                if live[k] and count[kind] < want:
                    count[kind] += 1
                    keep.append(k)
            short = [(p, s, kind) for (p, s) in list(seam_rows()) + list(tight_rows())
                     for kind in (("short",) if p in ("A", "Bt") else ("short",) + SEAM_RUNS)
                     if count[(p, s, kind)] < (1 if kind != "short" else
                                               2 if p in ("A", "Bt") else 4)]
            if not short:
                pick = lambda xs: [xs[k] for k in keep]
                return Group(f"seams-{P.tag}-{P.model}", q, pick(seqs), list(range(len(keep))),
                             pick(brute), pick(refs), pick(meta))
            err = (P.tag, P.model, attempt, short, dict(count))
        raise ValueError(f"seam family: too few live targets: {err}")
    return _cached(("seams", P.tag, P.model), make)


# ---- b. window edges ---------------------------------------------------------------------------
EDGE_HEIGHTS = (255, 256, 257, 511, 512, 513)
EDGE_WIDTHS = (63, 64, 65, 127, 128, 129)


def _edge_target(q, P, rng, kind, size, nth):
    """(target, window start): the nth start row from 37 on that is no multiple of 4 and at
    which the run is pinned (it cannot slide); the run's last cell is 7 from the window's."""
    for s in range(37, 137):
        if s % 4 == 0:
            continue
        if kind == "rows":
            lo, hi, e = s + size - 9, s + size - 7, s + size
            ok = q[lo] != q[hi] and q[lo - 1] != q[hi - 1]
            core = [q[s:lo], q[hi:e]]
        else:
            at, e = s + size - 9, s + size - 2
            ins = np.array([_unlike(rng, P, q[at]), _unlike(rng, P, q[at - 1])], np.uint8)
            ok = ins[0] != q[at - 1] and ins[1] != q[at]
            core = [q[s:at], ins, q[at:e]]
        if ok and nth == 0:
            break
        nth -= ok
    else:
        raise ValueError(f"edge family: no pinned run for {kind} {size}")
    left, right = _flanks(rng, P, q, s, e)
    return np.concatenate([left] + core + [right]).astype(np.uint8), s


def edge_family(P):
    """Group of family b: for every height a window of exactly that many rows with a 2-row I run
    at window rows [h - 9, h - 7), for every width a window of exactly that many columns with a
    2-column D run at window columns [w - 9, w - 7).  A target whose window is not the intended
    one is drawn again at the next start row (6 times at most).
    meta[k] = ("rows" | "cols", size)."""
    def make():
        rng = np.random.default_rng([7, len(P.tag), P.model])
        q = rng.integers(0, P.letters, SEAM_QLEN).astype(np.uint8)
        meta = [(kind, size) for kind, sizes in (("rows", EDGE_HEIGHTS), ("cols", EDGE_WIDTHS))
                for size in sizes]
        seqs, brute, refs = ([None] * len(meta) for _ in range(3))
        todo, why = list(range(len(meta))), None
        for nth in range(6):
            drawn = [_edge_target(q, P, rng, *meta[k], nth) for k in todo]
            bs, rs = prepare(q, [t for t, _ in drawn], P)
            again = []
            for k, (t, s), b, r in zip(todo, drawn, bs, rs):
                kind, size = meta[k]
                got = b[2] - b[1] + 1 if kind == "rows" else b[4] - b[3] + 1
                runs = runs_of(r.ops, AC.I if kind == "rows" else AC.D) if r else None
                if got != size or b[1] != s or runs != [(size - 9, size - 7)]:
                    again.append(k)
                    why = (kind, size, b, runs)
                seqs[k], brute[k], refs[k] = t, b, r
            todo = again
            if not todo:
                return Group(f"edges-{P.tag}-{P.model}", q, seqs, list(range(len(seqs))), brute,
                             refs, meta)
        raise ValueError(f"edge family {P.tag}/{P.model}: not the intended window: {why}")
    return _cached(("edges", P.tag, P.model), make)


# ---- c. ties across lanes and strips -------------------------------------------------------------
# Everything around the units is N (code 4, which matches nothing, itself included): under
# ALT's cheap merged gaps two random DNA sequences align with a score that grows with their
# length, so random letters around a unit extend one copy and the tie is gone.
TIE_UNIT, TIE_FLANK, TIE_N = 24, 10, 4
Tie = collections.namedtuple("Tie", "name kind cells want")
# kind "end": `cells` are maximal cells (row, column) of the forward H; "start": of the H of the
# reversed prefixes.  want = (q_start, q_end, t_start, t_end).


def _max_cells(q, t, P):
    H = AC._h_batch(AC._sub_tensor([(q, t)], P.sub), P.go, P.ge, P.model)[0]
    rows, cols = np.nonzero(H == H.max())
    return {(int(r), int(c)) for r, c in zip(rows, cols)}


def _tie_pairs(P, rng):
    U, W = TIE_UNIT, TIE_FLANK
    out = []

    def query(spots):
        q = np.full(600, TIE_N, np.uint8)
        for r, unit in spots:
            q[r:r + len(unit)] = unit
        return q

    def letters(n):
        return rng.integers(0, P.letters, n).astype(np.uint8)

    def fill(n):
        return np.full(n, TIE_N, np.uint8)

    # the unit at two query rows, once in the target: the smaller q_end
    for name, r1, r2 in (("end-lanes", 10, 50), ("end-strips", 10, 300),
                         ("end-strips-same-lane", 10, 266)):
        unit = letters(U)
        q = query([(r1, unit), (r2, unit)])
        t = np.concatenate([fill(W), unit, fill(W)])
        assert (r1 // 4 % 64 == r2 // 4 % 64) == name.endswith("same-lane")
        out.append((q, t, Tie(name, "end", [(r1 + U - 1, W + U - 1), (r2 + U - 1, W + U - 1)],
                              (r1, r1 + U - 1, W, W + U - 1))))
    # the unit twice in the target (different 64-column blocks), once in the query: the smaller
    # t_end
    unit = letters(U)
    r, c2 = 300, W + U + 100
    q = query([(r, unit)])
    t = np.concatenate([fill(W), unit, fill(c2 - W - U), unit, fill(W)])
    assert (W + U - 1) // 64 != (c2 + U - 1) // 64
    out.append((q, t, Tie("end-columns", "end", [(r + U - 1, W + U - 1), (r + U - 1, c2 + U - 1)],
                          (r, r + U - 1, W, W + U - 1))))
    # two units of one score: the one in the later strip ends at the lower column and wins
    u1, u2 = letters(U), letters(U)
    q = query([(10, u1), (300, u2)])
    t = np.concatenate([fill(W), u2, fill(50), u1, fill(W)])
    c1 = W + U + 50
    out.append((q, t, Tie("end-mixed", "end", [(300 + U - 1, W + U - 1), (10 + U - 1, c1 + U - 1)],
                          (300, 300 + U - 1, W, W + U - 1))))
    # the start rule: a stretch before the core that scores 0 in all (matches, then mismatches)
    # gives two starts of one score on one diagonal; the nearer one (larger t_start) is the
    # start.  In the reversed walk the two lie in different lanes, or in different strips.
    ma = int(P.sub[0][0])
    mi = -int(P.sub[0][1])
    assert all(int(P.sub[a][b]) == (ma if a == b else -mi) for a in range(4) for b in range(4))
    nm, nx = mi // math.gcd(ma, mi), ma // math.gcd(ma, mi)  # nm matches pay for nx mismatches
    for name, core in (("start-lanes", 30), ("start-strips", 250)):
        rb = 100
        ra = rb + nm + nx
        e = ra + core
        q = query([(rb, letters(e - rb))])
        mis = np.array([_unlike(rng, P, q[rb + nm + k]) for k in range(nx)], np.uint8)
        t = np.concatenate([fill(W), q[rb:rb + nm], mis, q[ra:e], fill(W)])
        far = core - 1 + nm + nx
        assert (core - 1) // 4 != far // 4 and ((core - 1) // 256 != far // 256) == (core > 200)
        out.append((q, t, Tie(name, "start", [(core - 1, core - 1), (far, far)],
                              (ra, e - 1, W + nm + nx, W + nm + nx + core - 1))))
    return out


TIE_CASES = ("end-lanes", "end-strips", "end-strips-same-lane", "end-columns", "end-mixed",
             "start-lanes", "start-strips")


def tie_family(P):
    """[Group] of family c, one per case of TIE_CASES (each has a query of its own); the
    condition: the model's H has the stated maximal cells (two or more), and the brute-force
    record is the one the tie rule asks for.  A case whose random letters happen to extend one
    copy is drawn again (8 times at most)."""
    def make():
        groups, why = {}, {}
        for attempt in range(8):
            rng = np.random.default_rng([11, len(P.tag), P.model, attempt])
            for q, t, tie in _tie_pairs(P, rng):
                if tie.name in groups:
                    continue
                brute, refs = prepare(q, [t], P)
                s, qs, qe, ts, te = brute[0]
                if tie.kind == "end":
                    cells = _max_cells(q, t, P)
                else:
                    cells = _max_cells(q[:qe + 1][::-1], t[:te + 1][::-1], P)
                if set(tie.cells) <= cells and (qs, qe, ts, te) == tie.want:
                    groups[tie.name] = Group(f"{tie.name}-{P.tag}-{P.model}", q, [t], [0], brute,
                                             refs, [tie])
                else:
                    why[tie.name] = (sorted(cells)[:6], brute[0], tie)
            if len(groups) == len(TIE_CASES):
                return [groups[name] for name in TIE_CASES]
        raise ValueError(f"tie family {P.tag}/{P.model}: "
                         f"{[why[n] for n in TIE_CASES if n not in groups]}")
    return _cached(("ties", P.tag, P.model), make)


# ---- d. tie-rich paths ---------------------------------------------------------------------------
def _low_complexity(rng, n, letters=3):
    out = []
    while len(out) < n:
        unit = [int(x) for x in rng.integers(0, letters, int(rng.integers(1, 4)))]
        out += unit * int(rng.integers(2, 7))
    return np.array(out[:n], np.uint8)


def tie_rich_family(model):
    """[Group] of family d, one per set of TIE_SETS.  Conditions over the model's batch: every
    kind of co-optimal move occurs on >= 20 path cells, and >= a quarter of the pairs have a
    co-optimal path with other ops than the reference one (a diagonal / gap or left / up tie on
    the path).  A group's meta = [tie counts, pairs with another path]."""
    def make():
        groups = [_tie_rich_group(dna_param(tag, model, TIE_SETS)) for tag in TIE_SETS]
        total = collections.Counter()
        for g in groups:
            total.update(g.meta[0])
        other, n = sum(g.meta[1] for g in groups), sum(len(g.seqs) for g in groups)
        if min(total[k] for k in ("dg", "lu", "oe")) < 20 or 4 * other < n:
            raise ValueError(f"tie-rich family, model {model}: ties {dict(total)}, "
                             f"{other} of {n} pairs with another path")
        return groups
    return _cached(("tierich", model), make)


def _tie_rich_group(P, n=48):
    """Low-complexity targets (three letters, repeats of period 1-3) cut from a low-complexity
    query of 300 rows, with substitutions and short indels."""
    def make():
        rng = np.random.default_rng([13, len(P.tag), P.model])
        q = _low_complexity(rng, 300)
        seqs = []
        for k in range(n):
            ln = int(rng.integers(20, 140))
            a = int(rng.integers(0, 300 - ln)) if k % 3 else int(rng.integers(256 - ln + 8, 248))
            core = [int(c) for c in q[a:a + ln]]
            for _ in range(ln // 10):
                core[int(rng.integers(0, len(core)))] = int(rng.integers(0, 3))
            for _ in range(int(rng.integers(1, 4))):
                g, pos = int(rng.integers(1, 5)), int(rng.integers(0, len(core)))
                if rng.random() < 0.5:
                    core[pos:pos] = [int(c) for c in _low_complexity(rng, g)]
                else:
                    del core[pos:pos + g]
            seqs.append(np.concatenate([_low_complexity(rng, int(rng.integers(0, 12))),
                                        np.array(core, np.uint8),
                                        _low_complexity(rng, int(rng.integers(0, 12)))]))
        brute, refs = prepare(q, seqs, P)
        total = collections.Counter()
        other = 0
        for r in refs:
            if r is not None:
                total.update(r.ties)
                other += r.ties["dg"] + r.ties["lu"] > 0
        return Group(f"tierich-{P.tag}-{P.model}", q, seqs, list(range(n)), brute, refs,
                     [dict(total), other])
    return make()


# ---- scratch reuse -------------------------------------------------------------------------------
REUSE_HITS = 448


def i32_waves(n, scols, budget_bytes):
    """swk_i32_waves' rule (csrc/swbank_kaux.hip): a wave per hit, 4,096 at most, as many as
    the scratch budget holds two rows of `scols` 8-byte cells for, 4 at the least, in fours."""
    w = min(n, 256 * 16)
    w = min(w, max(4, budget_bytes // (max(scols, 1) * 2 * 8)))
    return (w + 3) // 4 * 4


def reuse_case(P):
    """(Group, second hit order): the seam family's targets (three strips each) alternating with
    1-40-letter targets (random ones and slices of the query) and empty ones, REUSE_HITS hits
    with repeats, in two different orders: in the first every wave (at a scratch budget of
    1 MiB) takes a long and a short hit by turns, the second is a random permutation."""
    def make():
        g = seam_family(P)
        rng = np.random.default_rng([17, len(P.tag), P.model])
        short = []
        for k in range(24):
            ln = int(rng.integers(1, 41))
            a = int(rng.integers(0, len(g.q) - ln))
            short.append(g.q[a:a + ln].copy() if k % 2 else
                         rng.integers(0, P.letters, ln).astype(np.uint8))
        short += [np.zeros(0, np.uint8)] * 2
        sb, sr = prepare(g.q, short, P)
        long_ = [k for k, t in enumerate(g.seqs) if len(t) > 600]  # the three-strip windows
        seqs = [g.seqs[k] for k in long_] + short
        nl, ns = len(long_), len(short)
        # wave w aligns hits w, w + waves, w + 2 waves, ...: long and short ones by turns
        waves = i32_waves(REUSE_HITS, max(len(t) for t in seqs), 1 << 20)
        hits = [(k // 2) % nl if (k + k // waves) % 2 == 0 else nl + (k // 2) % ns
                for k in range(REUSE_HITS)]
        order2 = [hits[k] for k in rng.permutation(REUSE_HITS)]
        order2 = [nl] + order2 + [0]  # (starts with a short hit, ends with a long one)
        return Group(f"reuse-{P.tag}-{P.model}", g.q, seqs, hits,
                     [g.brute[k] for k in long_] + sb, [g.refs[k] for k in long_] + sr,
                     None), order2
    return _cached(("reuse", P.tag, P.model), make)


# ---- the boundary and protein cases of tests/test_gpu_align.py ----------------------------------
QLENS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 300, 513]
TLENS = [0, 1, 63, 64, 65, 127, 128, 129, 200]


def planted(rng, q, L, alpha=4):
    """A slice of q with substitutions and 1-5-base insertions and deletions, in random flanks,
    L codes in all."""
    if L == 0:
        return np.zeros(0, np.uint8)
    n = min(len(q), L)
    a = int(rng.integers(0, len(q) - n + 1))
    core = [int(c) for c in q[a:a + n]]
    for _ in range(max(1, n // 12)):
        core[int(rng.integers(0, len(core)))] = int(rng.integers(0, alpha))
    for _ in range(int(rng.integers(1, 4))):
        k, pos = int(rng.integers(1, 6)), int(rng.integers(0, len(core) + 1))
        if rng.random() < 0.5:
            core[pos:pos] = [int(c) for c in rng.integers(0, alpha, k)]
        elif len(core) > k:
            del core[pos:pos + k]
    core = core[:L]
    flank = L - len(core)
    left = int(rng.integers(0, flank + 1))
    return np.concatenate([rng.integers(0, alpha, left), np.array(core, np.int64),
                           rng.integers(0, alpha, flank - left)]).astype(np.uint8)


def boundary_case(qlen, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 4, qlen).astype(np.uint8)
    lens = [int(x) for x in rng.choice(TLENS, 24)]
    lens[:len(TLENS)] = TLENS  # every length occurs
    seqs = [rng.integers(0, 4, L).astype(np.uint8) if k % 2 == 0 else planted(rng, q, L)
            for k, L in enumerate(lens)]
    hits = [int(x) for x in rng.permutation(24)]
    hits += [hits[3], hits[17]]  # two repeats
    return q, seqs, hits


def protein_case():
    rng = np.random.default_rng(33)
    q = rng.integers(0, 20, 300).astype(np.uint8)
    lens = [400, 1, 37, 256, 257, 399, 128, 300] * 2
    seqs = [rng.integers(0, 20, L).astype(np.uint8) if k % 2 == 0 else planted(rng, q, L, 20)
            for k, L in enumerate(lens)]
    return q, seqs, list(range(16))


def device_align(bank, seqs, hits, stride, ids=None):
    """sw_align_hits_device on torch buffers -> Alignment objects."""
    import swbank as S
    import torch
    res, offs, lens = S.pack_targets(seqs)
    dev = torch.device("cuda", 0)
    hv = np.asarray(hits, np.uint64)
    d_res = torch.from_numpy(res).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_hits = torch.from_numpy(hv.view(np.int64)).to(dev)
    d_ids = torch.from_numpy(np.asarray(ids, np.uint64).view(np.int64)).to(dev) \
        if ids is not None else None
    d_out = torch.full((len(hv) * S.ALIGNMENT_DTYPE.itemsize,), 0x3C, dtype=torch.uint8, device=dev)
    d_cig = torch.full((max(1, len(hv) * stride),), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    bank.align_hits_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), len(seqs),
                           max(int(lens.max()), 1), d_hits.data_ptr(), len(hv), d_out.data_ptr(),
                           d_cig.data_ptr() if stride else 0, stride,
                           d_ids=d_ids.data_ptr() if d_ids is not None else 0)
    bank.sync()
    rec = d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE)
    cig = d_cig.cpu().numpy().view(np.uint32)
    if stride:
        assert [int(r["cigar_offset"]) for r in rec] == [h * stride for h in range(len(hv))]
    return S.alignments_from(rec, cig)
