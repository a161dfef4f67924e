"""Alignment checks shared by the alignment tests (a helper, not a test module).

Two things, both tied to the oracle (oracle/sw_oracle.c) so that neither stands alone:

1. ``brute_ends``: the full H matrix of a pair for either gap model, following the oracle's
   recurrences (merged: the first-column rule included), and the end / start tie rules of
   include/swbank.h applied by brute force: end = among the maximal cells the smallest t_end,
   then the smallest q_end; start = the same rule on the reversed prefixes q[q_end..0] x
   t[t_end..0].  Every use asserts ``H.max() == oracle.score_pair(...)``.

   The matrices are built row by row with numpy over a batch of pairs.  The one sequential
   dependency inside a row, the horizontal gap, is a running maximum: Gotoh's
   E(i,j) = max_k<j (H(i,k) + go + ge (j-k)) is ``maximum.accumulate`` over H~ - ge k, H~ being
   H without E (an E-derived H never opens a better E while go <= 0); the merged model's
   I(i,j) = max(a_j, I(i,j-1) + ge), a_j from the row above and this row's M, likewise.

2. ``check_alignment``: validates a record without knowing the path preference: bounds, the
   oracle's score of the window equals the score, the CIGAR's consumption counts, first and last
   op M, the re-scored CIGAR equals the score under the model's gap-run rule (Gotoh: a run is a
   maximal stretch of one code; merged: adjacent I and D stretches form one run; a run of k
   columns costs open + k * extend), n_columns / n_identities recomputed from the ops.
"""
import numpy as np

M, I, D = 0, 1, 2
GAP_MERGED, GAP_GOTOH = 0, 1
EMPTY, NO_PATH = 1, 2
_PADS = -(1 << 20)  # substitution score of padded cells (they never reach a valid cell)


def _h_batch(S, go, ge, model):
    """H matrices [B, m, n] (int64) of a batch of substitution tensors S [B, m, n]."""
    B, m, n = S.shape
    S = S.astype(np.int64)
    H = np.zeros((B, m, n), np.int64)
    col = np.arange(n, dtype=np.int64)
    if model == GAP_GOTOH:
        Hp = np.zeros((B, n), np.int64)
        Fp = np.full((B, n), -(1 << 40), np.int64)
        colx = np.arange(n + 1, dtype=np.int64)
        for i in range(m):
            F = np.maximum(Hp + go + ge, Fp + ge)
            diag = np.concatenate([np.zeros((B, 1), np.int64), Hp[:, :-1]], axis=1)
            Ht = np.maximum(np.maximum(diag + S[:, i, :], 0), F)
            full = np.concatenate([np.zeros((B, 1), np.int64), Ht], axis=1)  # H(i, -1) = 0
            acc = np.maximum.accumulate(full - ge * colx, axis=1)
            E = acc[:, :n] + go + ge * (col + 1)
            h = np.maximum(Ht, E)
            H[:, i, :] = h
            Hp, Fp = h, F
        return H
    Mp = np.zeros((B, n), np.int64)
    Ip = np.zeros((B, n), np.int64)
    for i in range(m):
        diag = np.concatenate([np.zeros((B, 1), np.int64), np.maximum(Mp, Ip)[:, :-1]], axis=1)
        Mr = np.maximum(diag + S[:, i, :], 0)
        a = np.empty((B, n), np.int64)
        a[:, 0] = max(go + ge, ge)  # first column: the neighbours are replaced by ZERO
        if n > 1:
            a[:, 1:] = np.maximum(np.maximum(Mp[:, 1:], Mr[:, :-1]) + go + ge, Ip[:, 1:] + ge)
        Ir = np.maximum.accumulate(a - ge * col, axis=1) + ge * col
        H[:, i, :] = np.maximum(Mr, Ir)
        Mp, Ip = Mr, Ir
    return H


def _sub_tensor(pairs, sub):
    m = max(len(q) for q, _ in pairs)
    n = max(len(t) for _, t in pairs)
    S = np.full((len(pairs), m, n), _PADS, np.int64)
    sub = np.asarray(sub, np.int64)
    for k, (q, t) in enumerate(pairs):
        S[k, :len(q), :len(t)] = sub[np.asarray(q, np.intp)][:, np.asarray(t, np.intp)]
    return S


def _best_cell(H):
    """(value, row, column) of the maximal cell with the smallest column, then row."""
    v = H.max()
    rows, cols = np.nonzero(H == v)
    k = np.lexsort((rows, cols))[0]
    return int(v), int(rows[k]), int(cols[k])


def brute_ends_batch(oracle, q, targets, sub, go, ge, model):
    """[(score, q_start, q_end, t_start, t_end)] of q against every target (zeros for a pair
    scoring 0), by the tie rules of include/swbank.h on full H matrices."""
    q = np.asarray(q, np.uint8)
    out = [(0, 0, 0, 0, 0)] * len(targets)
    live = [k for k, t in enumerate(targets) if len(t) and len(q)]
    if not live:
        return out
    fw = [(q, np.asarray(targets[k], np.uint8)) for k in live]
    Hf = _h_batch(_sub_tensor(fw, sub), go, ge, model)
    ends = []
    for x, (qq, t) in enumerate(fw):
        H = Hf[x, :len(qq), :len(t)]
        assert int(H.max()) == oracle.score_pair(qq, t, sub, go, ge, model), "model vs oracle"
        ends.append(_best_cell(H))
    rv = [(x, (q[:qe + 1][::-1], fw[x][1][:te + 1][::-1]))
          for x, (s, qe, te) in enumerate(ends) if s > 0]
    if rv:
        Hr = _h_batch(_sub_tensor([p for _, p in rv], sub), go, ge, model)
        for y, (x, (qr, tr)) in enumerate(rv):
            H = Hr[y, :len(qr), :len(tr)]
            s, qe, te = ends[x]
            assert int(H.max()) == oracle.score_pair(qr, tr, sub, go, ge, model), "model vs oracle"
            rs, ri, rj = _best_cell(H)
            assert rs == s, "the reversed prefixes score what the pair scores"
            out[live[x]] = (s, qe - ri, qe, te - rj, te)
    return out


def brute_ends(oracle, q, t, sub, go, ge, model):
    return brute_ends_batch(oracle, q, [t], sub, go, ge, model)[0]


def parse_cigar(text):
    ops, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            ops.append(int(num) << 4 | "MID".index(ch))
            num = ""
    assert num == ""
    return tuple(ops)


def rescore(ops, q, t, qs, ts, sub, go, ge, model):
    """(score, query codes consumed, target codes consumed, columns, identities) of the ops
    applied from (qs, ts) under the model's gap-run rule."""
    i, j, score, cols, idn = qs, ts, 0, 0, 0
    prev = None  # code of the previous op
    for op in ops:
        ln, code = op >> 4, op & 15
        assert ln > 0 and code in (M, I, D), op
        assert code != prev, "adjacent equal codes are merged"
        if code == M:
            for _ in range(ln):
                score += int(sub[q[i]][t[j]])
                idn += int(q[i] == t[j])
                i += 1
                j += 1
        else:
            # merged: a gap that turns the corner does not re-open
            opens = not (model == GAP_MERGED and prev in (I, D))
            score += (go if opens else 0) + ln * ge
            if code == I:
                i += ln
            else:
                j += ln
        cols += ln
        prev = code
    return score, i - qs, j - ts, cols, idn


def check_alignment(oracle, q, t, sub, go, ge, model, a, want_path=True):
    """Validate record `a` (swbank.Alignment) of q against t; returns nothing, asserts."""
    q = np.asarray(q, np.uint8)
    t = np.asarray(t, np.uint8)
    want = oracle.score_pair(q, t, sub, go, ge, model) if len(q) and len(t) else 0
    assert a.score == want, (a, want)
    if want == 0:
        assert a.flags == EMPTY and not a.ops and a.cigar == ""
        assert (a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns, a.n_identities) == (0,) * 6
        return
    assert 0 <= a.q_start <= a.q_end < len(q) and 0 <= a.t_start <= a.t_end < len(t), a
    qw, tw = q[a.q_start:a.q_end + 1], t[a.t_start:a.t_end + 1]
    assert oracle.score_pair(qw, tw, sub, go, ge, model) == a.score, ("window", a)
    if not want_path:
        assert a.flags == NO_PATH and not a.ops and (a.n_columns, a.n_identities) == (0, 0), a
        return
    assert a.flags == 0 and a.ops, a
    assert a.ops[0] & 15 == M and a.ops[-1] & 15 == M, a.cigar
    s, dq, dt, cols, idn = rescore(a.ops, q, t, a.q_start, a.t_start, sub, go, ge, model)
    assert (dq, dt) == (len(qw), len(tw)), ("consumption", a)
    assert s == a.score, ("re-scored", s, a)
    assert (cols, idn) == (a.n_columns, a.n_identities), ("columns", cols, idn, a)
    assert parse_cigar(a.cigar) == tuple(a.ops)
