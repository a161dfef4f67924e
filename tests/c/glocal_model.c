/* The global-local search (include/swbank.h "global-local search") restated in plain C, for the
 * tests: the four lines of the definition over full rows with a real -infinity, no device, no
 * library.  Built by tests/glocal_cases.py with the host compiler and loaded with ctypes.
 *
 * drop_kind / drop_at make the mutants the seam tests need: what a kernel computes that loses a
 * gap state where it is handed over.  1 drops F between rows drop_at - 1 and drop_at (F(drop_at - 1,
 * j) reads as -infinity: a run of query residues against gaps must open again there), 2 drops E
 * between columns drop_at - 1 and drop_at (E(i, drop_at - 1) reads as -infinity).  0 is the
 * definition. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG (-(INT64_C(1) << 50))
#define END_NONE UINT32_MAX

static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }

/* One strand: q[m], t[L] (already reverse-complemented for the reverse strand), sub[alpha * alpha]
 * with sub[q * alpha + t].  *end: the end index, END_NONE for the boundary. */
static int64_t strand_score(const uint8_t *q, size_t m, const uint8_t *t, size_t L,
                            const int8_t *sub, int alpha, int64_t o, int64_t e, int ends,
                            int drop_kind, size_t drop_at, uint32_t *end) {
  const int qb = ends != 2, tb = ends != 1; /* which boundaries are penalised */
  /* index j + 1: column -1 is index 0 */
  int64_t *Hp = malloc((L + 1) * sizeof *Hp), *Hc = malloc((L + 1) * sizeof *Hc);
  int64_t *Fp = malloc((L + 1) * sizeof *Fp), *Fc = malloc((L + 1) * sizeof *Fc);
  int64_t best = 0;
  uint32_t at = END_NONE;
  Hp[0] = 0; /* H(-1,-1) */
  Fp[0] = NEG;
  for (size_t j = 0; j < L; ++j) {
    Hp[j + 1] = tb ? o + (int64_t)j * e : 0; /* H(-1,j) */
    Fp[j + 1] = NEG;
  }
  if (ends == 2) { /* column L - 1, rows -1 .. m - 1 */
    best = Hp[L];
    at = END_NONE;
  }
  for (size_t i = 0; i < m; ++i) {
    Hc[0] = qb ? o + (int64_t)i * e : 0; /* H(i,-1) */
    Fc[0] = NEG;
    int64_t E = NEG;
    for (size_t j = 0; j < L; ++j) {
      const int64_t s = sub[(size_t)q[i] * alpha + t[j]];
      const int64_t M = s + Hp[j];
      E = max2(Hc[j] + o, (drop_kind == 2 && j == drop_at ? NEG : E) + e);
      const int64_t Fu = drop_kind == 1 && i == drop_at ? NEG : Fp[j + 1];
      const int64_t F = max2(Hp[j + 1] + o, Fu + e);
      Fc[j + 1] = F;
      Hc[j + 1] = max2(max2(M, E), F);
    }
    if (ends == 2 && Hc[L] > best) {
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
  /* Hp is row m - 1 (the boundary row when m == 0) */
  if (ends == 1) {
    best = Hp[0];
    at = END_NONE;
    for (size_t j = 0; j < L; ++j)
      if (Hp[j + 1] > best) {
        best = Hp[j + 1];
        at = (uint32_t)j;
      }
  } else if (ends == 3) {
    best = Hp[L];
    at = END_NONE;
  }
  free(Hp);
  free(Hc);
  free(Fp);
  free(Fc);
  *end = at;
  return best;
}

/* scores[k], ends_out[k], strands[k] of q against the n targets res + offs[k], lens[k] codes
 * each; both: the reverse strand too (DNA codes), its QUERY end given on the forward target. */
void glocal_model(const uint8_t *q, size_t m, const uint8_t *res, const uint64_t *offs,
                  const uint32_t *lens, size_t n, const int8_t *sub, int alpha, int32_t gap_open,
                  int32_t gap_extend, int ends, int both, int drop_kind, uint32_t drop_at,
                  int32_t *scores, uint32_t *ends_out, uint8_t *strands) {
  const int64_t o = (int64_t)gap_open + gap_extend, e = gap_extend;
  for (size_t k = 0; k < n; ++k) {
    const uint8_t *c = res + offs[k];
    const size_t L = lens[k];
    uint32_t fe = END_NONE, re = END_NONE;
    const int64_t fw = strand_score(q, m, c, L, sub, alpha, o, e, ends, drop_kind, drop_at, &fe);
    int64_t rv = fw;
    if (both) {
      uint8_t *rc = malloc(L ? L : 1);
      for (size_t i = 0; i < L; ++i) {
        const uint8_t v = c[L - 1 - i];
        rc[i] = v < 4 ? (uint8_t)(v ^ 2) : v;
      }
      rv = strand_score(q, m, rc, L, sub, alpha, o, e, ends, drop_kind, drop_at, &re);
      free(rc);
      if (ends == 1 && re != END_NONE) re = (uint32_t)(L - 1 - re);
    }
    const int r = both && rv > fw;
    scores[k] = (int32_t)(r ? rv : fw);
    ends_out[k] = r ? re : fe;
    strands[k] = (uint8_t)r;
  }
}
