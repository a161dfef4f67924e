/* align_set_client.c — a plain C99 client of the query-set calls of libswbank.so, for
 * tests/test_c_align_set.py.
 *
 *   align_set_client host               the new constants from C (no device), prints "host ok"
 *   align_set_client align Q0 Q1 T...   loads the DNA set {Q0, Q1}, aligns every query against
 *                                       every target T... (ASCII) with the reference penalties
 *                                       through sw_align_set_hits in the hits_per_query form
 *                                       (lines "A h ..."), takes the best query of every target
 *                                       from those scores with sw_best_queries (with a threshold
 *                                       of 1) and aligns each target against it in the
 *                                       hit_queries form (lines "B k query ..."); a record is
 *                                       "index score flags q_start q_end t_start t_end columns
 *                                       identities cigar" (cigar "-" when there are no ops).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_ALIGN_SET
#error "swbank.h without the query-set alignment calls"
#endif

#define CHECK(cond, msg)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, msg); \
      return 1;                                                     \
    }                                                               \
  } while (0)

#define MAXT 16
#define MAXLEN 512
#define MAXOPS 4096

static int host_checks(void) {
  CHECK(SW_QUERY_NONE == 0xFFFFFFFFu, "SW_QUERY_NONE");
  CHECK(SW_ALIGN_NO_HIT == 4 && (SW_ALIGN_NO_HIT & (SW_ALIGN_EMPTY | SW_ALIGN_NO_PATH)) == 0,
        "SW_ALIGN_NO_HIT is a flag of its own");
  CHECK(SWBANK_ABI_VERSION == 6, "the ABI version stays 6");
  printf("host ok\n");
  return 0;
}

static void print_record(const sw_alignment *a, const uint32_t *cig) {
  char text[256] = "-";
  if (a->cigar_len) sw_cigar_string(cig + a->cigar_offset, a->cigar_len, text, sizeof text);
  printf("%lld %d %u %u %u %u %u %u %u %s\n", (long long)a->index, a->score, a->flags, a->q_start,
         a->q_end, a->t_start, a->t_end, a->n_columns, a->n_identities, text);
}

static int align(int nt, char **q, char **t) {
  static uint8_t qcodes[2 * MAXLEN], res[MAXT * MAXLEN];
  uint64_t qoffs[2], offs[MAXT];
  uint32_t qlens[2], lens[MAXT];
  size_t total = 0;
  CHECK(nt >= 1 && nt <= MAXT, "1..16 targets");
  for (int i = 0; i < 2; ++i) {
    CHECK(strlen(q[i]) <= MAXLEN, "query too long");
    qlens[i] = (uint32_t)strlen(q[i]);
    qoffs[i] = total;
    sw_encode_ascii(SW_ALPHABET_DNA, q[i], qlens[i], qcodes + total);
    total += qlens[i];
  }
  total = 0;
  for (int k = 0; k < nt; ++k) {
    CHECK(strlen(t[k]) <= MAXLEN, "target too long");
    lens[k] = (uint32_t)strlen(t[k]);
    offs[k] = total;
    sw_encode_ascii(SW_ALPHABET_DNA, t[k], lens[k], res + total);
    total += lens[k];
  }
  sw_config cfg;
  sw_config_default(&cfg);
  sw_bank *bank = NULL;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  static sw_alignment al[2 * MAXT];
  static uint32_t cig[MAXOPS];
  uint64_t hits[2 * MAXT];
  size_t used = 0;
  const size_t n = (size_t)nt;
  for (size_t h = 0; h < 2 * n; ++h) hits[h] = h % n;
  CHECK(sw_set_penalties(bank, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_align_set_hits(bank, res, total, offs, lens, NULL, n, NULL, n, hits, 2 * n, al, cig,
                          MAXOPS, &used) == SW_ERR_STATE, "no query yet: SW_ERR_STATE");
  CHECK(sw_load_queries(bank, 2, NULL, qcodes, qoffs, qlens) == SW_OK, "query set");
  CHECK(sw_query_count(bank) == 2, "two queries");
  /* A: the nq x k layout, k = n */
  if (sw_align_set_hits(bank, res, total, offs, lens, NULL, n, NULL, n, hits, 2 * n, al, cig,
                        MAXOPS, &used) != SW_OK) {
    fprintf(stderr, "FAIL sw_align_set_hits: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  int32_t scores[2 * MAXT], best_score[MAXT];
  uint32_t best_query[MAXT];
  for (size_t h = 0; h < 2 * n; ++h) {
    scores[h] = al[h].score;
    printf("A %zu ", h);
    print_record(&al[h], cig);
  }
  /* the best query of every target; a target no query hits (score 0) names none */
  CHECK(sw_best_queries(bank, scores, n, 2, 1, NULL, NULL) == SW_ERR_ARG, "no output: SW_ERR_ARG");
  if (sw_best_queries(bank, scores, n, 2, 1, best_query, best_score) != SW_OK) {
    fprintf(stderr, "FAIL sw_best_queries: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  /* B: one hit per target against its best query */
  CHECK(sw_align_set_hits(bank, res, total, offs, lens, NULL, n, best_query, 1, NULL, n, al, cig,
                          MAXOPS, &used) == SW_ERR_ARG, "both forms at once: SW_ERR_ARG");
  if (sw_align_set_hits(bank, res, total, offs, lens, NULL, n, best_query, 0, NULL, n, al, cig,
                        MAXOPS, &used) != SW_OK) {
    fprintf(stderr, "FAIL sw_align_set_hits: %s\n", sw_last_error(bank));
    return 1;
  }
  for (size_t k = 0; k < n; ++k) {
    printf("B %zu %lld %d ", k, best_query[k] == SW_QUERY_NONE ? -1LL : (long long)best_query[k],
           best_score[k]);
    print_record(&al[k], cig);
  }
  sw_bank_destroy(bank);
  printf("align ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc >= 5 && strcmp(argv[1], "align") == 0) return align(argc - 4, argv + 2, argv + 4);
  fprintf(stderr, "usage: %s host | align Q0 Q1 T0 [T1 ...]\n", argv[0]);
  return 2;
}
