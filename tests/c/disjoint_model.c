/* The non-intersecting local alignments of a pair (include/swbank.h "non-intersecting local
 * alignments") restated in plain C, for the tests: the recurrence over full rows in int64 with a
 * real -infinity, one byte per cell for the walk back and the used set, no device, no library.
 * Built by tests/disjoint_cases.py with the host compiler and loaded with ctypes.
 *
 * kind / at make the mutants the seam tests need, what a kernel computes that loses something
 * where it is handed over: 1 drops F between rows at - 1 and at (F(at - 1, j) reads as -infinity),
 * 2 drops E between columns at - 1 and at (E(i, at - 1) reads as -infinity), 3 forgets the used
 * cells of row at, 4 forgets the used cells of column at.  0 is the definition. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NEG (-(INT64_C(1) << 50))
enum { SRC_M = 0, SRC_E = 1, SRC_F = 2, SRC_ZERO = 3, E_EXT = 16, F_EXT = 32, USED = 128 };
enum { EMPTY = 1, NO_PATH = 2 };
enum { OP_M = 0, OP_I = 1, OP_D = 2 };

typedef struct disjoint_rec {
  int32_t score;
  uint32_t flags, q_start, q_end, t_start, t_end, n_columns, n_identities, n_ops;
} disjoint_rec;

static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }

/* recs[rounds]; the ops of round r at ops + r * cap, at most cap of them (more: no path).
 * sub[q * alpha + t].  Returns 0, or -1 without memory. */
int disjoint_model(const uint8_t *q, size_t m, const uint8_t *t, size_t L, const int8_t *sub,
                   int alpha, int32_t gap_open, int32_t gap_extend, uint32_t rounds,
                   int32_t min_score, int kind, uint32_t at, disjoint_rec *recs, uint32_t *ops,
                   uint32_t cap) {
  const int64_t o = (int64_t)gap_open + gap_extend, e = gap_extend;
  memset(recs, 0, rounds * sizeof *recs);
  for (uint32_t r = 0; r < rounds; ++r) recs[r].flags = EMPTY;
  if (m == 0 || L == 0) return 0;
  uint8_t *dir = calloc(m * L, 1); /* the used flags of round 0: none */
  int64_t *Hp = malloc(L * sizeof *Hp), *Hc = malloc(L * sizeof *Hc);
  int64_t *Fp = malloc(L * sizeof *Fp), *Fc = malloc(L * sizeof *Fc);
  uint32_t *back = malloc((m + L) * sizeof *back);
  if (!dir || !Hp || !Hc || !Fp || !Fc || !back) return -1;
  for (uint32_t r = 0; r < rounds; ++r) {
    int64_t best = 0;
    size_t bi = 0, bj = 0;
    for (size_t i = 0; i < m; ++i) {
      int64_t E = NEG, Hl = 0; /* E(i,j-1), H(i,j-1) */
      for (size_t j = 0; j < L; ++j) {
        uint8_t *d = dir + i * L + j;
        const int forget = (kind == 3 && i == at) || (kind == 4 && j == at);
        const int64_t Hd = i && j ? Hp[j - 1] : 0, Hu = i ? Hp[j] : 0;
        const int64_t Eb = kind == 2 && j == at ? NEG : E;
        const int64_t Fb = !i || (kind == 1 && i == at) ? NEG : Fp[j];
        if ((*d & USED) && !forget) {
          *d = USED | SRC_ZERO;
          Hc[j] = Hl = 0;
          Fc[j] = E = NEG;
          continue;
        }
        const int64_t M = sub[(size_t)q[i] * alpha + t[j]] + Hd;
        const int64_t En = max2(Hl + o, Eb + e), Fn = max2(Hu + o, Fb + e);
        const int64_t H = max2(max2(0, M), max2(En, Fn));
        *d = (uint8_t)((*d & USED) | (H == 0 ? SRC_ZERO : M == H ? SRC_M : En == H ? SRC_E : SRC_F) |
                       (Eb + e > Hl + o ? E_EXT : 0) | (Fb + e > Hu + o ? F_EXT : 0));
        E = En;
        Fc[j] = Fn;
        Hc[j] = Hl = H;
        if (H > best || (H == best && H > 0 && j < bj)) { /* smallest t_end, then q_end */
          best = H;
          bi = i;
          bj = j;
        }
      }
      int64_t *x = Hp;
      Hp = Hc;
      Hc = x;
      x = Fp;
      Fp = Fc;
      Fc = x;
    }
    if (best < min_score) break;
    /* the walk back */
    size_t i = bi, j = bj, n = 0, qs = bi, ts = bj;
    uint32_t idn = 0;
    int64_t acc = 0;
    int state = 3, over = 0;
    for (;;) {
      uint8_t *d = dir + i * L + j;
      if (state == 3) {
        state = *d & 3;
        if (state == SRC_ZERO) break;
      }
      const uint8_t bits = *d;
      *d |= USED;
      qs = i;
      ts = j;
      if (state == SRC_M) {
        back[n++] = OP_M;
        acc += sub[(size_t)q[i] * alpha + t[j]];
        idn += q[i] == t[j];
        state = 3;
        if (i == 0 || j == 0) break;
        --i;
        --j;
      } else if (state == SRC_E) {
        back[n++] = OP_D;
        acc += bits & E_EXT ? e : o;
        state = bits & E_EXT ? SRC_E : 3;
        if (j == 0) { over = 1; break; }
        --j;
      } else {
        back[n++] = OP_I;
        acc += bits & F_EXT ? e : o;
        state = bits & F_EXT ? SRC_F : 3;
        if (i == 0) { over = 1; break; }
        --i;
      }
    }
    disjoint_rec *x = recs + r;
    x->score = (int32_t)best;
    x->q_start = (uint32_t)qs;
    x->q_end = (uint32_t)bi;
    x->t_start = (uint32_t)ts;
    x->t_end = (uint32_t)bj;
    x->flags = NO_PATH;
    /* the ops forwards, equal codes merged */
    uint32_t nops = 0, *slot = ops + (size_t)r * cap;
    for (size_t k = n; k-- > 0;) {
      if (k + 1 < n && back[k + 1] == back[k]) {
        if (nops <= cap) slot[nops - 1] += 16;
        continue;
      }
      if (nops < cap) slot[nops] = 1u << 4 | back[k];
      ++nops;
    }
    if (!over && acc == best && nops <= cap && nops) {
      x->flags = 0;
      x->n_columns = (uint32_t)n;
      x->n_identities = idn;
      x->n_ops = nops;
    }
  }
  free(dir);
  free(Hp);
  free(Hc);
  free(Fp);
  free(Fc);
  free(back);
  return 0;
}
