/* Alignments of frameshift hits (include/swbank.h "alignments of frameshift hits") restated in
 * plain C, for the tests: end, start (the reversed local pass), the anchored matrix over the
 * window and the walk, over plain arrays, no device, no library.  Built by tests/fsalign_cases.py
 * with the host compiler and loaded with ctypes. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG (-(INT64_C(1) << 40))
#define X_CODE 22
enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_SKIP = 3, OP_BACK = 4 };
enum { F_EMPTY = 1, F_NO_PATH = 2, F_REVERSE = 8, F_FRAME_SHIFT = 4 };

static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }

/* The best cell of the local matrix of rows q[m] against the amino acids a[P] of the codon starts
 * 0 .. P - 1: the highest H, then the smallest p, then the smallest i.  A mutant (the tests'
 * liveness check, mrow / mcol >= 0) loses the gap state at a seam: F does not extend into row
 * mrow, E does not extend into the columns of codon index mcol.  cells (optional): how many
 * cells hold the best H. */
static int64_t local_best(const uint8_t *q, size_t m, const uint8_t *a, size_t P,
                          const int8_t *sub, int alpha, int64_t o, int64_t e, int64_t fs,
                          ptrdiff_t mrow, ptrdiff_t mcol, size_t *bi, size_t *bp,
                          size_t *cells) {
  int64_t *Hp = calloc(P + 4, sizeof *Hp), *Hc = calloc(P + 4, sizeof *Hc);
  int64_t *Fp = malloc((P + 4) * sizeof *Fp), *Fc = malloc((P + 4) * sizeof *Fc);
  int64_t *E = malloc((P + 4) * sizeof *E);
  int64_t best = 0;
  size_t n_best = 0;
  *bi = *bp = 0;
  for (size_t p = 0; p < P + 4; ++p) Fp[p] = NEG;
  for (size_t i = 0; i < m; ++i) {
    for (size_t p = 0; p < 4; ++p) {
      Hc[p] = 0;
      E[p] = NEG;
      Fc[p] = NEG;
    }
    for (size_t p = 0; p < P; ++p) {
      const size_t x = p + 4; /* columns -4 .. -1 hold the outside */
      const int64_t s = sub[(size_t)q[i] * alpha + a[p]];
      const int64_t M = s + max2(max2(0, Hp[x - 3]), max2(Hp[x - 2], Hp[x - 4]) + fs);
      E[x] = max2(Hc[x - 3] + o, ((ptrdiff_t)(p / 3) == mcol ? NEG : E[x - 3]) + e);
      Fc[x] = max2(Hp[x] + o, ((ptrdiff_t)i == mrow ? NEG : Fp[x]) + e);
      Hc[x] = max2(max2(0, M), max2(E[x], Fc[x]));
      n_best = Hc[x] > best ? 1 : n_best + (Hc[x] == best && best > 0);
      if (Hc[x] > best || (Hc[x] == best && best > 0 && (p < *bp || (p == *bp && i < *bi)))) {
        best = Hc[x];
        *bi = i;
        *bp = p;
      }
    }
    int64_t *t = Hp;
    Hp = Hc;
    Hc = t;
    t = Fp;
    Fp = Fc;
    Fc = t;
  }
  free(Hp);
  free(Hc);
  free(Fp);
  free(Fc);
  free(E);
  if (cells) *cells = n_best;
  return best;
}

static void translate(const uint8_t *c, size_t L, const uint8_t *table, uint8_t *a) {
  for (size_t p = 0; p + 2 < L; ++p) {
    const uint8_t c0 = c[p], c1 = c[p + 1], c2 = c[p + 2];
    a[p] = (c0 < 4 && c1 < 4 && c2 < 4) ? table[c0 * 16 + c1 * 4 + c2] : X_CODE;
  }
}

/* One pair; mpass = 0: the model.  mpass = 'A', 'B' or 'C': the mutant of that pass, in the pass's
 * own row and column numbering.  rec[9]: score, flags, q_start, q_end, t_start, t_end, n_columns, n_identities,
 * cigar_len; ops[ops_cap] (more ops than that: F_NO_PATH; ops_cap == 0: coordinates only, also
 * F_NO_PATH).  Returns the value of the anchored matrix at the end cell (the score, or the test
 * fails). */
int64_t fsalign_mutant(const uint8_t *q, size_t m, const uint8_t *t, size_t L, const int8_t *sub,
                       int alpha, const uint8_t *table, int32_t gap_open, int32_t gap_extend,
                       int32_t fshift, uint32_t *rec, uint32_t *ops, size_t ops_cap, int mpass,
                       ptrdiff_t mrow, ptrdiff_t mcol) {
  const ptrdiff_t ar = mpass == 'A' ? mrow : -1, ac = mpass == 'A' ? mcol : -1;
  const ptrdiff_t br = mpass == 'B' ? mrow : -1, bc = mpass == 'B' ? mcol : -1;
  const ptrdiff_t cr = mpass == 'C' ? mrow : -1, cc = mpass == 'C' ? mcol : -1;
  const int64_t o = (int64_t)gap_open + gap_extend, e = gap_extend, fs = fshift;
  for (int i = 0; i < 9; ++i) rec[i] = 0;
  rec[1] = F_EMPTY;
  if (L < 3 || m == 0) return 0;
  const size_t P = L - 2;
  uint8_t *c[2] = {malloc(L), malloc(L)}, *a[2] = {malloc(P), malloc(P)};
  for (size_t i = 0; i < L; ++i) {
    const uint8_t v = t[L - 1 - i];
    c[0][i] = t[i];
    c[1][i] = v < 4 ? (uint8_t)(v ^ 2) : v;
  }
  size_t ei[2], ep[2];
  int64_t sc[2];
  for (int s = 0; s < 2; ++s) {
    translate(c[s], L, table, a[s]);
    sc[s] = local_best(q, m, a[s], P, sub, alpha, o, e, fs, ar, ac, &ei[s], &ep[s], NULL);
  }
  const int rev = sc[1] > sc[0];
  const int64_t score = sc[rev];
  int64_t at_end = 0;
  if (score > 0) {
    const size_t q_end = ei[rev], p_end = ep[rev];
    /* start: the same rule on rows q[q_end..0], columns p_end..0 */
    uint8_t *rq = malloc(q_end + 1), *ra = malloc(p_end + 1);
    for (size_t i = 0; i <= q_end; ++i) rq[i] = q[q_end - i];
    for (size_t p = 0; p <= p_end; ++p) ra[p] = a[rev][p_end - p];
    size_t si, sp;
    const int64_t back =
        local_best(rq, q_end + 1, ra, p_end + 1, sub, alpha, o, e, fs, br, bc, &si, &sp, NULL);
    free(rq);
    free(ra);
    if (back != score && !mpass) abort(); /* the reversal argument failed */
    const size_t q_start = q_end - si, p_start = p_end - sp;
    /* the anchored matrix over the window: no floor, a 0 diagonal at the first cell only */
    const size_t R = si + 1, C = sp + 1;
    int64_t *H = malloc(R * C * sizeof *H), *E = malloc(R * C * sizeof *E);
    int64_t *F = malloc(R * C * sizeof *F);
    uint8_t *dir = malloc(R * C); /* src | link << 2 | eext << 4 | fext << 5 */
#define AT(X, i, p) ((i) < 0 || (p) < 0 ? NEG : X[(size_t)(i) * C + (size_t)(p)])
    for (ptrdiff_t i = 0; i < (ptrdiff_t)R; ++i)
      for (ptrdiff_t p = 0; p < (ptrdiff_t)C; ++p) {
        const int64_t s = sub[(size_t)q[q_start + i] * alpha + a[rev][p_start + p]];
        const int64_t d3 = AT(H, i - 1, p - 3), d2 = AT(H, i - 1, p - 2), d4 = AT(H, i - 1, p - 4);
        int64_t via;
        unsigned link;
        if (i == 0 && p == 0) {
          via = 0;
          link = 0;
        } else if (d3 >= max2(d2, d4) + fs) {
          via = d3;
          link = 1;
        } else if (d2 >= d4) {
          via = d2 + fs;
          link = 2;
        } else {
          via = d4 + fs;
          link = 3;
        }
        const int64_t M = s + via;
        const int64_t eo = AT(H, i, p - 3) + o, ex = (p / 3 == cc ? NEG : AT(E, i, p - 3)) + e;
        const int64_t fo = AT(H, i - 1, p) + o, fx = (i == cr ? NEG : AT(F, i - 1, p)) + e;
        const int64_t Ev = max2(eo, ex), Fv = max2(fo, fx), Hv = max2(M, max2(Ev, Fv));
        const size_t x = (size_t)i * C + (size_t)p;
        H[x] = Hv;
        E[x] = Ev;
        F[x] = Fv;
        dir[x] = (uint8_t)((Hv == M ? 0u : Hv == Ev ? 1u : 2u) | link << 2 |
                           (ex > eo ? 16u : 0u) | (fx > fo ? 32u : 0u));
        if (i == (ptrdiff_t)R - 1 && p == (ptrdiff_t)C - 1) at_end = M;
      }
    /* the walk: the end cell as an M cell; ops backwards, then reversed */
    size_t n_ops = 0, cols = 0, ids = 0;
    int ok = ops_cap > 0 && at_end == score, state = 0; /* 0 M, 1 E, 2 F, 3 H */
    ptrdiff_t i = (ptrdiff_t)R - 1, p = (ptrdiff_t)C - 1;
    for (size_t step = 0; ok; ++step) {
      if (step > R + C + 2 || i < 0 || p < 0) abort();
      const unsigned d = dir[(size_t)i * C + (size_t)p];
      if (state == 3) state = (int)(d & 3);
      unsigned op, shift = 0;
      int done = 0;
      if (state == 0) {
        op = OP_M;
        ++cols;
        ids += q[q_start + i] == a[rev][p_start + p];
        const unsigned link = d >> 2 & 3;
        done = link == 0;
        shift = link == 2 ? OP_BACK : link == 3 ? OP_SKIP : 0;
        p -= link == 2 ? 2 : link == 3 ? 4 : 3;
        --i;
        state = 3;
      } else if (state == 1) {
        op = OP_D;
        ++cols;
        state = d & 16 ? 1 : 3;
        p -= 3;
      } else {
        op = OP_I;
        ++cols;
        state = d & 32 ? 2 : 3;
        --i;
      }
      for (int k = 0; k < 2; ++k) { /* the op, then the shift that leads into its M run */
        const unsigned code = k ? shift : op;
        if (k && !shift) break;
        if (n_ops && (ops[n_ops - 1] & 15u) == code && code < OP_SKIP)
          ops[n_ops - 1] += 16;
        else if (n_ops < ops_cap)
          ops[n_ops++] = 16 | code;
        else
          ok = 0;
      }
      if (done) break;
    }
    free(H);
    free(E);
    free(F);
    free(dir);
    rec[0] = (uint32_t)score;
    rec[1] = (rev ? F_REVERSE : 0u) | (uint32_t)(p_start % 3) << F_FRAME_SHIFT;
    rec[2] = (uint32_t)q_start;
    rec[3] = (uint32_t)q_end;
    rec[4] = (uint32_t)(rev ? L - 1 - (p_end + 2) : p_start);
    rec[5] = (uint32_t)(rev ? L - 1 - p_start : p_end + 2);
    if (ok) {
      for (size_t k = 0; k < n_ops / 2; ++k) {
        const uint32_t x = ops[k];
        ops[k] = ops[n_ops - 1 - k];
        ops[n_ops - 1 - k] = x;
      }
      rec[6] = (uint32_t)cols;
      rec[7] = (uint32_t)ids;
      rec[8] = (uint32_t)n_ops;
    } else {
      rec[1] |= F_NO_PATH;
    }
  }
  for (int s = 0; s < 2; ++s) {
    free(c[s]);
    free(a[s]);
  }
  return at_end;
}

int64_t fsalign_model(const uint8_t *q, size_t m, const uint8_t *t, size_t L, const int8_t *sub,
                      int alpha, const uint8_t *table, int32_t gap_open, int32_t gap_extend,
                      int32_t fshift, uint32_t *rec, uint32_t *ops, size_t ops_cap) {
  return fsalign_mutant(q, m, t, L, sub, alpha, table, gap_open, gap_extend, fshift, rec, ops,
                        ops_cap, 0, -1, -1);
}

/* How many cells of the winning strand's local matrix hold the score (0 when nothing scores):
 * more than one means the tie rule decided where the hit ends. */
size_t fsalign_best_cells(const uint8_t *q, size_t m, const uint8_t *t, size_t L,
                          const int8_t *sub, int alpha, const uint8_t *table, int32_t gap_open,
                          int32_t gap_extend, int32_t fshift) {
  if (L < 3 || m == 0) return 0;
  const size_t P = L - 2;
  uint8_t *c = malloc(L), *a = malloc(P);
  int64_t sc[2];
  size_t cells[2], bi, bp;
  for (int s = 0; s < 2; ++s) {
    for (size_t i = 0; i < L; ++i) {
      const uint8_t v = t[L - 1 - i];
      c[i] = s ? (v < 4 ? (uint8_t)(v ^ 2) : v) : t[i];
    }
    translate(c, L, table, a);
    sc[s] = local_best(q, m, a, P, sub, alpha, (int64_t)gap_open + gap_extend, gap_extend, fshift,
                       -1, -1, &bi, &bp, &cells[s]);
  }
  free(c);
  free(a);
  return cells[sc[1] > sc[0]];
}
