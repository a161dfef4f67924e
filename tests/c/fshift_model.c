/* The frameshift-tolerant translated search (include/swbank.h) restated in plain C, for the
 * tests: the four lines of the definition over full matrices, no device, no library.  Built by
 * tests/fshift_cases.py with the host compiler and loaded with ctypes. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG (-(INT64_C(1) << 40))
#define X_CODE 22

static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }

/* The score of one strand: q[m] protein codes, c[L] DNA codes (already reverse-complemented for
 * the reverse strand), sub[alpha * alpha] with sub[q * alpha + a], table[64] protein codes. */
static int64_t strand_score(const uint8_t *q, size_t m, const uint8_t *c, size_t L,
                            const int8_t *sub, int alpha, const uint8_t *table, int64_t o,
                            int64_t e, int64_t fs) {
  if (L < 3 || m == 0) return 0;
  const size_t P = L - 2; /* columns p = 0 .. L - 3 */
  uint8_t *a = malloc(P);
  /* rows i - 1 and i of H and F; E runs along the row.  Index p + 4: columns -4 .. -1 hold the
   * outside (H = 0, E = F = -infinity). */
  int64_t *Hp = calloc(P + 4, sizeof *Hp), *Hc = calloc(P + 4, sizeof *Hc);
  int64_t *Fp = malloc((P + 4) * sizeof *Fp), *Fc = malloc((P + 4) * sizeof *Fc);
  int64_t *E = malloc((P + 4) * sizeof *E);
  int64_t best = 0;
  for (size_t p = 0; p < P; ++p) {
    const uint8_t c0 = c[p], c1 = c[p + 1], c2 = c[p + 2];
    a[p] = (c0 < 4 && c1 < 4 && c2 < 4) ? table[c0 * 16 + c1 * 4 + c2] : X_CODE;
  }
  for (size_t p = 0; p < P + 4; ++p) Fp[p] = NEG;
  for (size_t i = 0; i < m; ++i) {
    for (size_t p = 0; p < 4; ++p) {
      Hc[p] = 0;
      E[p] = NEG;
      Fc[p] = NEG;
    }
    for (size_t p = 0; p < P; ++p) {
      const size_t x = p + 4;
      const int64_t s = sub[(size_t)q[i] * alpha + a[p]];
      const int64_t M = s + max2(max2(0, Hp[x - 3]), max2(Hp[x - 2], Hp[x - 4]) + fs);
      E[x] = max2(Hc[x - 3] + o, E[x - 3] + e);
      Fc[x] = max2(Hp[x] + o, Fp[x] + e);
      Hc[x] = max2(max2(0, M), max2(E[x], Fc[x]));
      best = max2(best, Hc[x]);
    }
    int64_t *t = Hp;
    Hp = Hc;
    Hc = t;
    t = Fp;
    Fp = Fc;
    Fc = t;
  }
  free(a);
  free(Hp);
  free(Hc);
  free(Fp);
  free(Fc);
  free(E);
  return best;
}

/* scores[k], strands[k] of q against the n targets res + offs[k], lens[k] codes each. */
void fshift_model(const uint8_t *q, size_t m, const uint8_t *res, const uint64_t *offs,
                  const uint32_t *lens, size_t n, const int8_t *sub, int alpha,
                  const uint8_t *table, int32_t gap_open, int32_t gap_extend, int32_t fs,
                  int32_t *scores, uint8_t *strands) {
  const int64_t o = (int64_t)gap_open + gap_extend, e = gap_extend;
  for (size_t k = 0; k < n; ++k) {
    const uint8_t *c = res + offs[k];
    const size_t L = lens[k];
    uint8_t *rc = malloc(L ? L : 1);
    for (size_t i = 0; i < L; ++i) {
      const uint8_t v = c[L - 1 - i];
      rc[i] = v < 4 ? (uint8_t)(v ^ 2) : v;
    }
    const int64_t fw = strand_score(q, m, c, L, sub, alpha, table, o, e, fs);
    const int64_t rv = strand_score(q, m, rc, L, sub, alpha, table, o, e, fs);
    free(rc);
    scores[k] = (int32_t)(rv > fw ? rv : fw);
    strands[k] = rv > fw;
  }
}
