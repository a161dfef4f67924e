/* The alignments of global-local hits (include/swbank.h "alignments of global-local hits")
 * restated in plain C, for the tests: full rows with a real -infinity, no device, no library.
 * Built by tests/glalign_cases.py with the host compiler and loaded with ctypes.
 *
 * One pair per call, in the library's four steps: the score, end and strand of the search; the
 * start by the reversed anchored walk; the anchored matrix of the window; the walk back through
 * it by the documented preference.
 *
 * drops[3][2] = {kind, at} for the steps A (the search), B (the reversed walk, in ITS rows and
 * columns) and C (the window, in ITS rows and columns) make the mutants the seam tests need: what
 * a kernel computes that loses a gap state where it is handed over.  Kind 1 drops F between rows
 * at - 1 and at (F(at - 1, j) reads as -infinity), kind 2 drops E between columns at - 1 and at
 * (E(i, at - 1) reads as -infinity), 0 is the definition.  A mutant of step C whose walked path
 * no longer scores `score` has no path (flag 2), as the library's own re-scoring decides. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG (-(INT64_C(1) << 50))
#define NONE UINT32_MAX
enum { F_EMPTY = 1, F_NO_PATH = 2, F_REVERSE = 8 };

typedef struct glalign_rec {
  int32_t score;
  uint32_t flags, q_start, q_end, t_start, t_end, n_columns, n_identities, n_ops;
  uint32_t tie_diag, tie_left, tie_open; /* path cells with a co-optimal alternative */
} glalign_rec;

static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }

/* rows[m] against cols[L]; qb / tb: the row / column boundary is penalised; res 1: the best of
 * the last row (columns -1 .. L-1, the smallest), 2: of the last column (rows -1 .. m-1, the
 * smallest), 3: the corner.  *pos: that index, NONE for -1. */
static int64_t walk(const uint8_t *rows, size_t m, const uint8_t *cols, size_t L,
                    const int8_t *sub, int alpha, int64_t o, int64_t e, int qb, int tb, int res,
                    int drop_kind, size_t drop_at, uint32_t *pos) {
  int64_t *Hp = malloc((L + 1) * sizeof *Hp), *Hc = malloc((L + 1) * sizeof *Hc);
  int64_t *Fp = malloc((L + 1) * sizeof *Fp), *Fc = malloc((L + 1) * sizeof *Fc);
  int64_t best = 0;
  uint32_t at = NONE;
  Hp[0] = 0;
  Fp[0] = NEG;
  for (size_t j = 0; j < L; ++j) {
    Hp[j + 1] = tb ? o + (int64_t)j * e : 0;
    Fp[j + 1] = NEG;
  }
  if (res == 2) best = Hp[L];
  for (size_t i = 0; i < m; ++i) {
    Hc[0] = qb ? o + (int64_t)i * e : 0;
    Fc[0] = NEG;
    int64_t E = NEG;
    for (size_t j = 0; j < L; ++j) {
      const int64_t M = sub[(size_t)rows[i] * alpha + cols[j]] + Hp[j];
      E = max2(Hc[j] + o, (drop_kind == 2 && j == drop_at ? NEG : E) + e);
      const int64_t Fu = drop_kind == 1 && i == drop_at ? NEG : Fp[j + 1];
      const int64_t F = max2(Hp[j + 1] + o, Fu + e);
      Fc[j + 1] = F;
      Hc[j + 1] = max2(max2(M, E), F);
    }
    if (res == 2 && Hc[L] > best) {
      best = Hc[L];
      at = (uint32_t)i;
    }
    int64_t *x = Hp;
    Hp = Hc;
    Hc = x;
    x = Fp;
    Fp = Fc;
    Fc = x;
  }
  if (res == 1) {
    best = Hp[0];
    for (size_t j = 0; j < L; ++j)
      if (Hp[j + 1] > best) {
        best = Hp[j + 1];
        at = (uint32_t)j;
      }
  } else if (res == 3) {
    best = Hp[L];
  }
  free(Hp);
  free(Hc);
  free(Fp);
  free(Fc);
  *pos = at;
  return best;
}

static uint32_t push(uint32_t *ops, uint32_t cap, uint32_t n, uint32_t code, uint32_t len) {
  if (len == 0) return n;
  if (n && n <= cap && (ops[n - 1] & 15u) == code) {
    ops[n - 1] += len << 4;
    return n;
  }
  if (n < cap) ops[n] = len << 4 | code;
  return n + 1;
}

/* Steps C and D: the anchored matrix of rows[Q] x cols[C] and the walk back; qc[Q]: the query's
 * own codes (identities).  Returns the score of the walked path; ops are written backwards. */
static int64_t window_path(const uint8_t *rows, size_t Q, const uint8_t *cols, size_t C,
                           const int8_t *sub, int alpha, int64_t o, int64_t e, int drop_kind,
                           size_t drop_at, glalign_rec *r, uint32_t *ops, uint32_t cap) {
  const size_t W = C + 1;
  int64_t *H = malloc((Q + 1) * W * sizeof *H), *E = malloc((Q + 1) * W * sizeof *E);
  int64_t *F = malloc((Q + 1) * W * sizeof *F);
#define AT(X, i, j) X[((size_t)((i) + 1)) * W + (size_t)((j) + 1)]
  for (long j = -1; j < (long)C; ++j) {
    AT(H, -1, j) = j < 0 ? 0 : o + j * e;
    AT(E, -1, j) = AT(F, -1, j) = NEG;
  }
  for (long i = 0; i < (long)Q; ++i) {
    AT(H, i, -1) = o + i * e;
    AT(E, i, -1) = AT(F, i, -1) = NEG;
    for (long j = 0; j < (long)C; ++j) {
      const int64_t Ml = sub[(size_t)rows[i] * alpha + cols[j]] + AT(H, i - 1, j - 1);
      const int64_t El = drop_kind == 2 && (size_t)j == drop_at ? NEG : AT(E, i, j - 1);
      const int64_t Fu = drop_kind == 1 && (size_t)i == drop_at ? NEG : AT(F, i - 1, j);
      AT(E, i, j) = max2(AT(H, i, j - 1) + o, El + e);
      AT(F, i, j) = max2(AT(H, i - 1, j) + o, Fu + e);
      AT(H, i, j) = max2(max2(Ml, AT(E, i, j)), AT(F, i, j));
    }
  }
  long i = (long)Q - 1, j = (long)C - 1;
  int state = 3; /* 0 M, 1 E, 2 F, 3 H */
  int64_t acc = 0;
  uint32_t n = 0, cols_n = 0, idn = 0;
  while (i >= 0 && j >= 0) {
    if (state == 3) {
      const int64_t Ml = sub[(size_t)rows[i] * alpha + cols[j]] + AT(H, i - 1, j - 1);
      const int64_t h = AT(H, i, j);
      state = Ml == h ? 0 : AT(E, i, j) == h ? 1 : 2;
      if (state == 0 && (AT(E, i, j) == h || AT(F, i, j) == h)) ++r->tie_diag;
      if (state == 1 && AT(F, i, j) == h) ++r->tie_left;
    }
    if (state == 0) {
      n = push(ops, cap, n, 0, 1);
      idn += rows[i] == cols[j];
      acc += sub[(size_t)rows[i] * alpha + cols[j]];
      --i;
      --j;
      state = 3;
    } else if (state == 1) {
      const int64_t El = drop_kind == 2 && (size_t)j == drop_at ? NEG : AT(E, i, j - 1);
      const int64_t op = AT(H, i, j - 1) + o, ex = El + e;
      n = push(ops, cap, n, 2, 1);
      r->tie_open += op == ex;
      acc += ex > op ? e : o;
      state = ex > op ? 1 : 3;
      --j;
    } else {
      const int64_t Fu = drop_kind == 1 && (size_t)i == drop_at ? NEG : AT(F, i - 1, j);
      const int64_t op = AT(H, i - 1, j) + o, ex = Fu + e;
      n = push(ops, cap, n, 1, 1);
      r->tie_open += op == ex;
      acc += ex > op ? e : o;
      state = ex > op ? 2 : 3;
      --i;
    }
    ++cols_n;
  }
  if (j >= 0) {
    n = push(ops, cap, n, 2, (uint32_t)j + 1);
    acc += o + j * e;
    cols_n += (uint32_t)j + 1;
  } else if (i >= 0) {
    n = push(ops, cap, n, 1, (uint32_t)i + 1);
    acc += o + i * e;
    cols_n += (uint32_t)i + 1;
  }
#undef AT
  free(H);
  free(E);
  free(F);
  r->n_ops = n;
  r->n_columns = cols_n;
  r->n_identities = idn;
  return acc;
}

static uint8_t *reversed(const uint8_t *s, size_t from, size_t n) { /* s[from], s[from-1], ... */
  uint8_t *r = malloc(n ? n : 1);
  for (size_t k = 0; k < n; ++k) r[k] = s[from - k];
  return r;
}

/* q[m] against t[L] (codes < alpha; both: DNA codes).  ops[cap] receives the CIGAR (len << 4 |
 * code) when it fits; else the record has no path. */
void glalign_model(const uint8_t *q, size_t m, const uint8_t *t, size_t L, const int8_t *sub,
                   int alpha, int32_t gap_open, int32_t gap_extend, int ends, int both,
                   const uint32_t *drops, glalign_rec *r, uint32_t *ops, uint32_t cap) {
  const int64_t o = (int64_t)gap_open + gap_extend, e = gap_extend;
  const int qb = ends != 2, tb = ends != 1;
  uint32_t fp = NONE, rp = NONE;
  uint8_t *rc = malloc(L ? L : 1);
  for (size_t k = 0; k < L; ++k) {
    const uint8_t v = t[L - 1 - k];
    rc[k] = v < 4 ? (uint8_t)(v ^ 2) : v;
  }
  *r = (glalign_rec){0};
  const int64_t fw = walk(q, m, t, L, sub, alpha, o, e, qb, tb, ends, (int)drops[0], drops[1], &fp);
  int64_t rv = fw;
  if (both) rv = walk(q, m, rc, L, sub, alpha, o, e, qb, tb, ends, (int)drops[0], drops[1], &rp);
  const int rev = both && rv > fw;
  const uint8_t *c = rev ? rc : t;
  const uint32_t pos = rev ? rp : fp;
  r->score = (int32_t)(rev ? rv : fw);
  r->flags = F_EMPTY;
  if (m == 0 || (ends == 3 ? L == 0 : pos == NONE)) {
    free(rc);
    return;
  }
  size_t qs = 0, qe = m - 1, ts = 0, te = L - 1;
  if (ends != 3) {
    if (ends == 1) te = pos; else qe = pos;
    uint8_t *rr = reversed(q, qe, qe + 1), *cc = reversed(c, te, te + 1);
    uint32_t sp = NONE;
    (void)walk(rr, qe + 1, cc, te + 1, sub, alpha, o, e, 1, 1, ends, (int)drops[2], drops[3], &sp);
    const size_t back = sp == NONE ? 0 : sp;
    if (ends == 1) ts = te - (back < te ? back : te); else qs = qe - (back < qe ? back : qe);
    free(rr);
    free(cc);
  }
  r->flags = rev ? F_REVERSE : 0;
  r->q_start = (uint32_t)qs;
  r->q_end = (uint32_t)qe;
  r->t_start = (uint32_t)(rev ? L - 1 - te : ts);
  r->t_end = (uint32_t)(rev ? L - 1 - ts : te);
  const int64_t acc = window_path(q + qs, qe - qs + 1, c + ts, te - ts + 1, sub, alpha, o, e,
                                  (int)drops[4], drops[5], r, ops, cap);
  if (acc != r->score || r->n_ops > cap) {
    r->flags |= F_NO_PATH;
    r->n_ops = r->n_columns = r->n_identities = 0;
  } else {
    for (uint32_t x = 0; x < r->n_ops / 2; ++x) {
      const uint32_t v = ops[x];
      ops[x] = ops[r->n_ops - 1 - x];
      ops[r->n_ops - 1 - x] = v;
    }
  }
  free(rc);
}
