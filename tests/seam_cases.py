"""Seam inputs, the CPU mutant model and the parameter cases (a helper, not a test module).

The score kernels hand column and row state across many seams (LDS rings between waves, HBM
edge rows between query segments, DPP between lanes, split / segmented tails, balanced ranges,
the 256-row strips of the int32 and alignment kernels).  Each seam hands over H and a gap value.
Random targets, and exact copies of the query, hardly ever carry a live gap across a given row
or column, so a kernel that hands H over but loses the gap value passes them.  This module
builds the inputs that do, and the model that proves they do:

1. ``straddle_targets`` / ``tile_template``: targets made from the query with exactly one indel
   of 2-6 letters that straddles a requested cut.  A deletion target ``q[:c-a] + q[c-a+g:]``
   (0 < a < g) makes the optimal path run a vertical gap over query row c; an insertion target
   ``q[:c-a] + g random letters + q[c-a:]`` a horizontal gap over target column c.

2. ``scores_with_cut``: the oracle's recurrences (oracle/sw_oracle.c; merged: the first-column
   rule included) in numpy over a batch, which can drop the gap state alone (merged I, Gotoh F
   on a row, E on a column) on crossing one row or one column while H is kept: what a kernel
   computes that hands H over a seam and writes the initial value in place of the gap value.
   With no cut it is the oracle (every use asserts equality with ``O.score_batch``).

3. ``CASES``: the named scoring-parameter cases shared by tests/test_param_envelope.py and
   tests/test_gpu_params.py; ``SEAMS``: the seam shapes of tests/test_gpu_seams.py.

Measured with tests/test_param_envelope.py (share of a seam's deletion targets whose score the
row mutant changes / share of its insertion targets the column mutant changes; first and last
seam of each family that is not within 6 letters of an end, over every parameter set and gap
model the GPU test runs; "tight": the cuts within 6 letters of an end, at the free-extension
set, where alone their gap is paid; the test asserts >= 50 % for each; in brackets the number of
seams x sets x models):

    ring100         del 100-100 % (12)  ins 100-100 % (12)  tight 100-100 % ( 2)
    ring130         del 100-100 % (12)  ins 100-100 % (12)
    seg300          del 100-100 % (12)
    seg600          del 100-100 % ( 6)
    lane100         del 100-100 % (12)                        tight 100-100 % ( 4)
    lane300         del 100-100 % (12)
    lane600         del 100-100 % (12)
    lane1020        del 100-100 % (12)
    wseg1100        del 100-100 % ( 6)
    strip300        del 100-100 % (12)
    strip600        del 100-100 % (12)
    split8          del 100-100 % (12)
    half257         del 100-100 % (12)
    half512         del 100-100 % (12)
    wbal48                                ins  99-100 % ( 6)
    wbal64                                ins  98-100 % ( 6)
    wbal1000        del 100-100 % (12)  ins 100-100 % (12)
    tbal40x24       del 100-100 % ( 3)  ins  93-100 % ( 6)
    tbal40x64       del 100-100 % ( 3)  ins 100-100 % ( 6)
    tbal40x128      del 100-100 % ( 3)  ins 100-100 % ( 6)
    tbal100x24      del 100-100 % ( 6)  ins 100-100 % ( 6)  tight 100-100 % ( 1)
    tbal100x64      del 100-100 % ( 6)  ins 100-100 % ( 6)  tight 100-100 % ( 1)
    tbal100x128     del 100-100 % ( 6)  ins 100-100 % ( 6)  tight 100-100 % ( 1)
    stream100x120   del 100-100 % (12)  ins 100-100 % (12)  tight 100-100 % ( 2)
    rbal40          del 100-100 % ( 3)  ins 100-100 % ( 6)
    qset600         del 100-100 % ( 6)

Gap uptake of the large-gap cases (share of the straddle targets that score differently with
gaps than without) is 100 % at the larger query length of each case; transposing an asymmetric
matrix changes 85-98 % of a case's 260 scores.
"""
import collections

import numpy as np

GAP_MERGED, GAP_GOTOH = 0, 1
_NEG = -(1 << 40)
_PADS = -(1 << 20)  # substitution score of cells past a target's end


# ---------------------------------------------------------------------------------------
# inputs
def _substitute(t, keep_lo, keep_hi, letters, rng, rate=12):
    """Substitutions at about 1 in `rate` positions (never more than 1 in 9), none within 10
    letters of [keep_lo, keep_hi)."""
    pos = np.arange(0, len(t), rate) + rng.integers(0, rate - 9 + 1)
    pos = pos[(pos < len(t)) & ((pos < keep_lo - 10) | (pos >= keep_hi + 10))]
    t[pos] = (t[pos] + rng.integers(1, letters, len(pos))) % letters
    return t


def _fit(t, L, letters, rng, front=False):
    """t cut or padded with random letters to length L, at its end or (front) at its start."""
    if L is None:
        return t
    if len(t) >= L:
        return (t[len(t) - L:] if front else t[:L]).copy()
    pad = rng.integers(0, letters, L - len(t)).astype(np.uint8)
    return np.concatenate([pad, t] if front else [t, pad])


def deletion_target(q, c, g, a, letters, L, rng, flank=None):
    """q without rows [c-a, c-a+g): the vertical run covers query row c.  `flank` limits the
    copied stretch on either side (the target then starts inside the query)."""
    lo, hi = c - a, c - a + g
    assert 0 < a < g and lo > 0 and hi < len(q), (c, a, g, len(q))
    s = 0 if flank is None else max(0, lo - flank)
    e = len(q) if flank is None else min(len(q), hi + flank)
    t = np.concatenate([q[s:lo], q[hi:e]]).astype(np.uint8)
    t = _substitute(t, lo - s, lo - s, letters, rng)
    # a short tail flank (a cut near the query's end) stays the target's end: random padding
    # after it would offer the alignment other stretches to jump to where extension is free
    return _fit(t, L, letters, rng, front=e - hi < 8)


def insertion_target(q, c, g, a, letters, L, rng, flank=None):
    """g random letters at target columns [c-a, c-a+g): the horizontal run covers column c.
    The copied query stretch ends up around the insertion: target column j < c-a is query row
    r0 + j, with r0 = 0 when the query is long enough (`flank` None) and otherwise chosen so
    that both flanks lie inside the query; columns before the left flank are random."""
    lo = c - a
    assert 0 < a < g and lo > 0, (c, a, g)
    m = len(q)
    lf = min(lo, m // 2 if flank is None else min(flank, m // 2))
    if flank is None and lo < m - 8:
        lf = lo
    rf = m - lf if flank is None else min(flank, m - lf)
    r = 0 if lf == lo else int(rng.integers(0, m - lf - rf + 1))
    head = rng.integers(0, letters, lo - lf).astype(np.uint8)
    ins = rng.integers(0, letters, g).astype(np.uint8)
    # the inserted letters must not extend either flank's match
    ins[0] = (q[r + lf] + 1 + rng.integers(0, letters - 1)) % letters
    ins[-1] = (q[r + lf - 1] + 1 + rng.integers(0, letters - 1)) % letters
    left = _substitute(q[r:r + lf].astype(np.uint8).copy(), lf, lf, letters, rng)
    right = _substitute(q[r + lf:r + lf + rf].astype(np.uint8).copy(), 0, 0, letters, rng)
    return _fit(np.concatenate([head, left, ins, right]), L, letters, rng)


Straddle = collections.namedtuple("Straddle", "kind cut")  # kind: "del" (row) | "ins" (column)


MIN_EDGE = 3   # letters an indel keeps from either end at the very least
FULL_EDGE = 6  # with this many (or more) the flank pays for the gap at the usual penalties


def _indel_choices(c, limit, flank, pinned):
    """Every (g, a) (length 2-6, 0 < a < g) that puts an indel [c-a, c-a+g) over cut c inside
    [0, limit) with MIN_EDGE letters on both sides and a length of at most a third of the
    shorter side (2 at the least), narrowed to those with the longest shorter side (counted up
    to 8: past that every choice is as good)."""
    best, room = [], -1
    for g in range(2, 7):
        for a in range(1, g):
            lo, hi = c - a, c - a + g
            near = min(lo, limit - hi) if flank is None else min(lo, limit - hi, flank)
            if lo < MIN_EDGE or hi > limit - MIN_EDGE or g > max(2, near // 3):
                continue
            if pinned is not None and not pinned(lo, hi):
                continue
            r = min(near, 8)
            if r > room:
                best, room = [], r
            if r == room:
                best.append((g, a))
    return best


def cut_is_tight(c, limit):
    """A cut so close to an end (fewer than FULL_EDGE letters on the shorter side of even a
    2-letter indel) that its gap is paid for only where extension is free: the mutant share of
    such a cut is asserted at the free-extension set alone."""
    return min(c - 1, limit - (c + 1)) < FULL_EDGE


def straddle_targets(q, letters, cuts_rows, cuts_cols, L, rng, per=4, flank=None):
    """(targets, meta): exactly `per` deletion targets for every row cut and `per` insertion
    targets for every column cut, each with one indel of 2-6 letters straddling its cut, padded
    with random letters to length L (L None: left as long as they come; L = (lo, hi): a ragged
    batch, every target cut or padded to a random length in [lo, hi]).  meta[k] =
    Straddle(kind, cut).  An indel keeps at least MIN_EDGE letters from either end of the query
    (deletions) or of the target (insertions), and 8 where the cut allows.  A deletion is also
    pinned: the letters at its ends differ, so that the run cannot slide off the cut.  A cut for
    which no such indel exists raises ValueError: nothing is dropped silently."""
    q = np.asarray(q, np.uint8)
    out, meta = [], []

    def pinned(lo, hi):
        return 0 < lo and hi < len(q) and q[lo] != q[hi] and q[lo - 1] != q[hi - 1]

    for kind, cuts in (("del", cuts_rows), ("ins", cuts_cols)):
        for c in cuts:
            for k in range(per):
                Lk = L if L is None or isinstance(L, (int, np.integer)) else \
                    int(rng.integers(L[0], L[1] + 1))
                if kind == "del":
                    ch = _indel_choices(c, len(q), flank, pinned)
                else:
                    ch = _indel_choices(c, 1 << 30 if Lk is None else Lk, flank, None)
                if not ch:
                    raise ValueError(f"no {kind} indel fits over cut {c} "
                                     f"(query {len(q)}, target length {Lk})")
                g, a = ch[int(rng.integers(0, len(ch)))]
                make = deletion_target if kind == "del" else insertion_target
                out.append(make(q, c, g, a, letters, Lk, rng, flank))
                meta.append(Straddle(kind, int(c)))
    return out, meta


def tile_template(q, letters, L, rng, cols=None, rows=None):
    """Whole tiles (a multiple of 128 targets of length L) of straddle targets: insertions over
    every column cut (default: every 8-column chunk boundary 8k < L) and deletions over every
    row cut (default: every 16th query row), 4 of each, cycled to fill the last tile.  A uniform
    batch of any size is this template repeated, and its expected scores the template's oracle
    scores repeated, so every target of the batch is checked."""
    q = np.asarray(q, np.uint8)
    flank = max(10, min(len(q), L) // 2 - 4)
    cols = list(range(8, L, 8)) if cols is None else list(cols)
    rows = list(range(16, len(q), 16)) if rows is None else list(rows)
    base, meta = straddle_targets(q, letters, rows, cols, L, rng, per=4, flank=flank)
    want = -(-len(base) // 128) * 128
    k = 0
    while len(base) < want:  # cycle: fresh draws of the same cuts
        more, mm = straddle_targets(q, letters, rows, cols, L, rng, per=1, flank=flank)
        base.append(more[k % len(more)])
        meta.append(mm[k % len(more)])
        k += 1
    return np.stack(base), meta


def with_noise(straddles, meta, n, maxlen, letters, rng, every=4):
    """A batch of n targets: every `every`-th one a straddle target (cycled), the rest random
    of lengths 0..maxlen, an empty and a 1-letter target among them.  Returns (seqs, meta) with
    meta None for the random ones."""
    seqs, mt = [], []
    for k in range(n):
        if k % every == 0 and straddles:
            j = (k // every) % len(straddles)
            seqs.append(straddles[j])
            mt.append(meta[j])
        else:
            ln = 0 if k == 1 else 1 if k == 2 else int(rng.integers(0, maxlen + 1))
            seqs.append(rng.integers(0, letters, ln).astype(np.uint8))
            mt.append(None)
    return seqs, mt


# ---------------------------------------------------------------------------------------
# the model
def _accumulate(src, ge, col):
    """max_k<=j (src_k + ge (j - k)) along axis 1."""
    return np.maximum.accumulate(src - ge * col, axis=1) + ge * col


def scores_with_cut(q, targets, sub, go, ge, model, cut_row=None, cut_col=None):
    """int64 scores of q against every target under the oracle's recurrences.  cut_row: on
    computing query row cut_row the vertical gap state of row cut_row - 1 is dropped (merged: I
    of the row above; Gotoh: F), H and M are kept.  cut_col: on computing target column cut_col
    the horizontal gap state of column cut_col - 1 is dropped (merged: I of the cell to the
    left; Gotoh: E).  Neither: the oracle."""
    q = np.asarray(q, np.uint8)
    B = len(targets)
    lens = np.array([len(t) for t in targets], np.int64)
    n = int(lens.max()) if B else 0
    best = np.zeros(B, np.int64)
    if n == 0 or len(q) == 0:
        return best
    sub = np.asarray(sub, np.int64)
    A = sub.shape[0]
    subx = np.concatenate([sub, np.full((A, 1), _PADS, np.int64)], axis=1)
    T = np.full((B, n), A, np.intp)
    for k, t in enumerate(targets):
        T[k, :len(t)] = t
    valid = np.arange(n)[None, :] < lens[:, None]
    col = np.arange(n, dtype=np.int64)
    cc = cut_col if cut_col is not None and 0 < cut_col < n else None
    zero = np.zeros((B, 1), np.int64)

    def runs(src, first):
        """The horizontal running maximum of src, restarted at column cc with `first` as that
        column's own source (the state of the columns before it is dropped)."""
        if cc is None:
            return _accumulate(src, ge, col)
        right = src[:, cc:].copy()
        right[:, 0] = first
        return np.concatenate([_accumulate(src[:, :cc], ge, col[:cc]),
                               _accumulate(right, ge, col[:n - cc])], axis=1)

    if model == GAP_GOTOH:
        Hp = np.zeros((B, n), np.int64)
        Fp = np.full((B, n), _NEG, np.int64)
        for i in range(len(q)):
            if cut_row is not None and i == cut_row:
                Fp = np.full((B, n), _NEG, np.int64)
            S = subx[q[i]][T]
            F = np.maximum(Hp + go + ge, Fp + ge)
            diag = np.concatenate([zero, Hp[:, :-1]], axis=1)
            Ht = np.maximum(np.maximum(diag + S, 0), F)  # H without E
            # E(j) = max_k<j (H(k) + go + ge (j - k)); an E-derived H never opens a better E
            # (go <= 0), so Ht serves as H(k) -- except right after a dropped E, where the
            # kept H(cc - 1) is the only source and may itself be E-derived
            src = np.concatenate([zero, Ht[:, :-1]], axis=1) + go + ge  # H(i, -1) = 0
            if cc is None:
                E = _accumulate(src, ge, col)
            else:
                E1 = _accumulate(src[:, :cc], ge, col[:cc])
                hl = np.maximum(Ht[:, cc - 1], E1[:, cc - 1])
                right = src[:, cc:].copy()
                right[:, 0] = hl + go + ge
                E = np.concatenate([E1, _accumulate(right, ge, col[:n - cc])], axis=1)
            h = np.maximum(Ht, E)
            best = np.maximum(best, np.where(valid, h, 0).max(axis=1))
            Hp, Fp = h, F
        return best
    Mp = np.zeros((B, n), np.int64)
    Ip = np.zeros((B, n), np.int64)
    for i in range(len(q)):
        diag = np.concatenate([zero, np.maximum(Mp, Ip)[:, :-1]], axis=1)  # H is kept
        if cut_row is not None and i == cut_row:
            Ip = np.full((B, n), _NEG, np.int64)
        S = subx[q[i]][T]
        Mr = np.maximum(diag + S, 0)
        a = np.empty((B, n), np.int64)
        a[:, 0] = max(go + ge, ge)  # first column: the neighbours are replaced by ZERO
        if n > 1:
            a[:, 1:] = np.maximum(np.maximum(Mp[:, 1:], Mr[:, :-1]) + go + ge, Ip[:, 1:] + ge)
        Ir = runs(a, a[:, cc] if cc is not None else None)
        best = np.maximum(best, np.where(valid, np.maximum(Mr, Ir), 0).max(axis=1))
        Mp, Ip = Mr, Ir
    return best


def mutant_shares(oracle, q, targets, meta, sub, go, ge, model, cut, chunk=64):
    """(share of the deletion targets of row `cut` whose score the row mutant changes, share of
    the insertion targets of column `cut` the column mutant changes); None where the batch has
    no such target.  Asserts that the model without a cut is the oracle on those targets."""
    shares = []
    for kind in ("del", "ins"):
        ts = [t for t, mt in zip(targets, meta) if mt is not None and mt == (kind, cut)]
        if not ts:
            shares.append(None)
            continue
        want = oracle_scores(oracle, q, ts, sub, go, ge, model)
        assert np.array_equal(scores_with_cut(q, ts, sub, go, ge, model), want), "model vs oracle"
        kw = {"cut_row": cut} if kind == "del" else {"cut_col": cut}
        got = scores_with_cut(q, ts, sub, go, ge, model, **kw)
        shares.append(float((got != want).mean()))
    return tuple(shares)


def oracle_scores(oracle, q, seqs, sub, go, ge, model):
    res, offs, lens = oracle.pack_residues(seqs)
    return oracle.score_batch(np.asarray(q, np.uint8), res, offs, lens, sub, go, ge, model)


# ---------------------------------------------------------------------------------------
# parameter cases
Case = collections.namedtuple("Case", "name alphabet matrix go ge qlens tags")
DNA, PROTEIN = 0, 1


def _dna_ref():
    m = np.full((5, 5), -4, np.int8)
    m[np.arange(4), np.arange(4)] = 5
    return m


def _blosum62():
    from oracle import oracle as O
    return O.BLOSUM62.copy()


def _asym_dna_pair():
    """Entries in [-8, 8] (one-byte f16 table), a uniform N column <= 0, the N row not."""
    m = np.array([[6, -3, -7, 1, -2],
                  [-5, 8, 2, -8, -2],
                  [-1, -6, 7, -4, -2],
                  [3, -2, -5, 5, -2],
                  [-3, -1, -4, -6, -2]], np.int8)
    assert (m != m.T).any() and (m[:, 4] == m[0, 4]).all()
    return m


def _asym_dna_odd():
    """Odd entries past 8: no one-byte f16 table, so the 2-byte profile."""
    m = np.array([[9, -9, -3, 2, -5],
                  [-7, 11, 1, -9, -5],
                  [-2, -5, 9, -8, -5],
                  [3, -1, -9, 11, -5],
                  [-4, -6, -2, -7, -5]], np.int8)
    return m


def _asym_dna_ncol():
    """A non-uniform N column and a positive N x N score (profile mode)."""
    m = _asym_dna_pair().copy()
    m[:, 4] = [-1, -3, 0, -2, 4]
    m[4, :4] = [-2, 1, -4, -1]
    return m


def _asym_protein():
    rng = np.random.default_rng(62)
    m = rng.integers(-8, 5, (24, 24)).astype(np.int8)
    m[np.arange(24), np.arange(24)] = rng.integers(4, 13, 24)
    m[3, 17], m[17, 3] = 12, -8
    assert (m != m.T).mean() > 0.8 and m.min() == -8 and m.max() == 12
    return m


def _nopos(top):
    rng = np.random.default_rng(7 - top)
    m = rng.integers(-9, top + 1, (5, 5)).astype(np.int8)
    m[2, 2] = top
    return m


def _wide():
    m = np.full((5, 5), -127, np.int8)
    m[np.arange(4), np.arange(4)] = 127
    return m


MATRICES = {
    "dna": _dna_ref, "blosum62": _blosum62, "asym-pair": _asym_dna_pair,
    "asym-odd": _asym_dna_odd, "asym-ncol": _asym_dna_ncol, "asym-prot": _asym_protein,
    "nopos0": lambda: _nopos(0), "nopos1": lambda: _nopos(-1), "wide": _wide,
}


def _cases():
    out = []

    def add(name, mat, go, ge, qlens, *tags):
        alpha = PROTEIN if mat in ("blosum62", "asym-prot") else DNA
        out.append(Case(name, alpha, mat, go, ge, qlens, frozenset(tags)))

    add("asym-pair", "asym-pair", -12, -4, (33, 300), "asym")
    add("asym-odd", "asym-odd", -14, -3, (33, 600), "asym")
    add("asym-ncol", "asym-ncol", -12, -4, (33, 300), "asym")
    add("asym-prot", "asym-prot", -11, -1, (33, 300), "asym")
    add("asym-pair-8-0", "asym-pair", -8, 0, (33, 300), "asym", "entry")
    add("asym-prot-100-10", "asym-prot", -100, -10, (33, 300), "asym", "entry", "uptake")
    add("nopos0", "nopos0", -12, -4, (33, 300), "nopos")
    add("nopos1", "nopos1", -12, -4, (33, 300), "nopos")
    add("wide", "wide", -12, -4, (33, 300), "wide")
    for mat in ("dna", "blosum62"):
        for go, ge in ((0, 0), (0, -3), (-8, 0), (-1, -30)):
            add(f"{mat}{go}/{ge}", mat, go, ge, (33, 300), "oddgap")
        add(f"{mat}-100/-10", mat, -100, -10, (33, 300), "uptake")
        add(f"{mat}-300/-40", mat, -300, -40, (33, 300), "uptake")
        add(f"{mat}-1000/-1", mat, -1000, -1, (33, 600), "uptake")
        # o + 2e + (S - smin) = 2047, 2048 (f16) and 2049 (u16)
        ge, span = (-4, 9) if mat == "dna" else (-1, 15)
        for tot in (2047, 2048, 2049):
            add(f"{mat}-neg{tot}", mat, -(tot - span + 2 * ge), ge, (33, 1100), "f16neg",
                "uptake", f"neg{tot}")
    add("merged-32767", "dna", -32767, -32767, (33, 300), "limit", "merged-only")
    add("gotoh-65535", "dna", -32767, -32763, (33, 300), "limit")  # o + e + S = 65535
    return out


CASES = _cases()
GOTOH_REFUSED = Case("gotoh-65536", DNA, "dna", -32767, -32764, (33,), frozenset())


def case_inputs(case, qlen, n=260):
    """(q, seqs, meta) of a case at one query length: n targets, one in four a straddle
    target (cuts near the middle of the query, both kinds), the rest random of lengths 0..qlen + 100,
    an empty and a 1-letter target included.  Deterministic in (case.name, qlen)."""
    seed = sum(ord(ch) * (k + 1) for k, ch in enumerate(case.name)) * 4096 + qlen
    rng = np.random.default_rng(seed)
    letters = 4 if case.alphabet == DNA else 20
    q = rng.integers(0, letters, qlen).astype(np.uint8)
    if case.alphabet == DNA and "f16neg" not in case.tags:
        q[rng.random(qlen) < 0.03] = 4
    # cuts near the middle: both flanks then outweigh the largest gap penalty of the table
    cuts = sorted({qlen // 2 - qlen // 32, qlen // 2, qlen // 2 + qlen // 32})
    st, mt = straddle_targets(q, letters, cuts, cuts, qlen + 100, rng, per=4)
    return (q,) + with_noise(st, mt, n, qlen + 100, letters if case.alphabet == PROTEIN else 5,
                             rng)


def expect_range_error(case, model):
    """The only refusals of the accepted envelope (include/swbank.h): a substitution range
    S - smin > 254, and Gotoh gaps with o + e + S > 65535."""
    m = MATRICES[case.matrix]().astype(np.int64)
    S = max(0, int(m.max()))
    return S - int(m.min()) > 254 or (model == GAP_GOTOH and -case.go - case.ge + S > 65535)


# ---------------------------------------------------------------------------------------
# seam families (tests/test_gpu_seams.py runs them; tests/test_param_envelope.py measures them)
Seam = collections.namedtuple("Seam", "name alphabet qlen rows cols L noise per",
                              defaults=(4,))


def _m16(qlen, *more, dead=()):
    """Every multiple of 16 below qlen, and `more`, without the cuts in `dead`."""
    return tuple(sorted((set(range(16, qlen, 16)) | set(more)) - set(dead)))


# rows / cols: the cuts; every one gets `per` targets or building the family fails.
# L None: a ragged batch (the straddle targets as long as they come, shuffled with `noise` random
# targets, an empty and a 1-letter one among them); L an int: whole tiles of equal-length
# targets (tile_template), repeated by the test; L (lo, hi): ragged straddle targets only.
# Cuts that cannot carry a live gap are left out by name, nowhere else: a run over row c needs
# row c + 1 inside it and then more letters after it than a gap costs, so row 128 of 130 (one
# letter left: 5 < 8, the cheapest gap of any set) and row 256 of 257 (none left) are dead.
SEAMS = {s.name: s for s in (
    # tile kernel, wave to wave through the LDS ring: every multiple of 16 rows (R = 16 and 32),
    # the short last wave's boundary included (96 of 100; 128 of 130 is dead)
    Seam("ring100", DNA, 100, _m16(100), (16, 64), None, 100),
    Seam("ring130", DNA, 130, _m16(130, dead=(128,)), (16, 64, 120), None, 100),
    # tile query segments through HBM edge rows
    Seam("seg300", DNA, 300, (64, 128, 192, 256), (), None, 124),
    Seam("seg600", DNA, 600, (512,), (), None, 124),
    # wave kernel lane rows, K = 4, 8, 16 rows per lane: every multiple of 16, and K and 2K
    # (4 and 8; 8 and 16; 16 and 32); 63K = 1008 in a query of its own
    Seam("lane100", DNA, 100, _m16(100, 4, 8), (), None, 40),
    Seam("lane300", DNA, 300, _m16(300, 8), (), None, 24),
    Seam("lane600", DNA, 600, _m16(600), (), None, 44),
    Seam("lane1020", DNA, 1020, (16, 32, 512, 1008), (), None, 24),
    # wave segments of 1024 rows
    Seam("wseg1100", DNA, 1100, (1024,), (), None, 24),
    # split tail rows 64 K / P, the 256-row strips of the int32 and alignment kernels
    Seam("strip300", DNA, 300, (128, 256), (), None, 54),
    Seam("strip600", DNA, 600, (256, 512), (), None, 54),
    Seam("split8", PROTEIN, 400, tuple(range(64, 400, 64)), (), None, 36),
    # two pairs per wave: lanes of 16 rows (256 of 257 is dead); 8 targets per cut
    Seam("half257", PROTEIN, 257, _m16(257, dead=(256,)), (), None, 213, 8),
    Seam("half512", PROTEIN, 512, _m16(512), (), None, 85, 8),
    # balanced ranges of the two-pairs wave kernel: 32-step blocks
    Seam("wbal48", PROTEIN, 512, (), (32,), 48, 0),
    Seam("wbal64", PROTEIN, 512, (), (32,), 64, 0),
    Seam("wbal1000", PROTEIN, 512, _m16(512), tuple(range(32, 1000, 32)), 1000, 0),
    # balanced chunk ranges of the tile kernel: 8-column chunks (cols None: every 8k < L)
    Seam("tbal40x24", DNA, 40, (16,), None, 24, 0),
    Seam("tbal40x64", DNA, 40, (16,), None, 64, 0),
    Seam("tbal40x128", DNA, 40, (16,), None, 128, 0),
    Seam("tbal100x24", DNA, 100, _m16(100), None, 24, 0),
    Seam("tbal100x64", DNA, 100, _m16(100), None, 64, 0),
    Seam("tbal100x128", DNA, 100, _m16(100), None, 128, 0),
    Seam("stream100x120", DNA, 100, _m16(100), None, 120, 0),
    # ragged balanced ranges: 4,098 targets of 30-61 letters, chunk boundaries inside every one
    Seam("rbal40", DNA, 40, (16,), (8, 16), (30, 61), 0, 1366),
    # query sets: the segment boundary (512) of the longest query
    Seam("qset600", DNA, 600, (512,), (), None, 124),
)}

_FAMILY_CACHE = {}


def _seam_cuts(s):
    """[(kind, cut, limit)] of a family: limit = the length the indel has to fit in."""
    cols = s.cols if s.cols is not None else tuple(range(8, s.L, 8))
    lim = s.L if isinstance(s.L, int) else s.L[0] if s.L is not None else 1 << 30
    return [("del", c, s.qlen) for c in s.rows] + [("ins", c, lim) for c in cols]


def _build_family(s, rng):
    letters = 4 if s.alphabet == DNA else 20
    q = rng.integers(0, letters, s.qlen).astype(np.uint8)
    if isinstance(s.L, int):
        tg, mt = tile_template(q, letters, s.L, rng, cols=s.cols, rows=s.rows)
    elif s.L is not None:
        tg, mt = straddle_targets(q, letters, s.rows, s.cols, s.L, rng, per=s.per, flank=14)
    else:
        ncuts = len(s.rows) + len(s.cols)
        st, sm = straddle_targets(q, letters, s.rows, s.cols, None, rng,
                                  per=max(s.per, -(-16 // ncuts)))
        noise = [rng.integers(0, letters + (s.alphabet == DNA),
                              k if k < 2 else int(rng.integers(0, s.qlen + 60))).astype(np.uint8)
                 for k in range(s.noise)]
        order = rng.permutation(len(st) + len(noise))
        both, bm = st + noise, sm + [None] * len(noise)
        tg, mt = [both[k] for k in order], [bm[k] for k in order]
    return q, tg, mt


def seam_family(name):
    """(q, targets, meta) of a family, deterministic: a list of ragged targets with meta None
    for the random ones, or a 2-D array of whole tiles for a uniform family.  The query is drawn
    again (a fixed sequence of seeds) until every cut of the family can be pinned; every cut
    then has at least `per` targets, or this raises."""
    if name in _FAMILY_CACHE:
        return _FAMILY_CACHE[name]
    s = SEAMS[name]
    err = None
    for attempt in range(64):
        rng = np.random.default_rng([sum(ord(ch) for ch in name), s.qlen, attempt])
        try:
            q, tg, mt = _build_family(s, rng)
            break
        except ValueError as e:
            err = e
    else:
        raise ValueError(f"{name}: {err}")
    count = collections.Counter(m for m in mt if m is not None)
    for kind, cut, _ in _seam_cuts(s):
        assert count[(kind, cut)] >= 4, (name, kind, cut, count[(kind, cut)])
    assert len(count) == len(_seam_cuts(s)), (name, sorted(count))
    _FAMILY_CACHE[name] = (q, tg, mt)
    return _FAMILY_CACHE[name]


def seam_params(alphabet, model):
    """[(tag, matrix name, open, extend)]: the path's usual penalties, free extension, and an
    asymmetric matrix.  Protein merged gaps take -12/0 for free extension: at -8/0 BLOSUM62's
    largest score exceeds open + extend, the first-column rule comes alive and the two-pairs
    wave kernel (whose seams these cases are for) does not run."""
    if alphabet == DNA:
        return [("ref", "dna", -12, -4), ("free", "dna", -8, 0), ("asym", "asym-pair", -12, -4)]
    free = -8 if model == GAP_GOTOH else -12
    return [("ref", "blosum62", -11, -1), ("free", "blosum62", free, 0),
            ("asym", "asym-prot", -11, -1)]


def tight_seams(name):
    """[(kind, cut)] of the family's cuts too close to an end for a gap to be paid at the usual
    penalties (cut_is_tight): measured at the free-extension set."""
    return [(k, c) for k, c, lim in _seam_cuts(SEAMS[name]) if cut_is_tight(c, lim)]


def first_last_seams(name):
    """[(kind, cut)] of the first and last cut of a family that is not tight, per kind."""
    tight = set(tight_seams(name))
    out = []
    for kind in ("del", "ins"):
        cuts = sorted(c for k, c, _ in _seam_cuts(SEAMS[name]) if k == kind and (k, c) not in tight)
        out += [(kind, c) for c in sorted({cuts[0], cuts[-1]})] if cuts else []
    return out
