/* stats_client.c — a plain C99 client of the hit-statistics calls of libswbank.so, for
 * tests/test_c_stats.py.
 *
 *   stats_client host                  the macros, the struct, sw_fit_statistics and
 *                                      sw_hit_significance on the host, the NULL-bank errors;
 *                                      prints the reference's two hits' bits and E, then "host ok"
 *   stats_client gpu q.fa lib.fa R S   estimates lambda and K of q.fa against R seeded shuffles
 *                                      (seed S) of lib.fa with sw_estimate_statistics and prints
 *                                      "kernel ...", "lambda K n_samples", then "stats ok".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#ifndef SWBANK_HAS_STATS
#error "swbank.h without the hit-statistics calls"
#endif

#define CHECK(cond, msg)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, msg); \
      return 1;                                                     \
    }                                                               \
  } while (0)

#define MAXREC 512
static char names[MAXREC][32], seqs[MAXREC][512];

/* one-record-per-two-lines FASTA (the layout of the reference's data files) */
static int read_fa(const char *path, char nm[][32], char sq[][512], int cap) {
  FILE *f = fopen(path, "r");
  if (!f) return -1;
  char line[1024];
  int n = -1;
  while (fgets(line, sizeof line, f)) {
    line[strcspn(line, "\r\n")] = 0;
    if (!line[0]) continue;
    if (line[0] == '>') {
      if (++n >= cap) break;
      size_t k = strlen(line + 1);
      if (k > 31) k = 31;
      memcpy(nm[n], line + 1, k);
      nm[n][k] = 0;
      sq[n][0] = 0;
    } else if (n >= 0) {
      const size_t have = strlen(sq[n]), add = strlen(line);
      const size_t take = add < 511 - have ? add : 511 - have;
      memcpy(sq[n] + have, line, take);
      sq[n][have + take] = 0;
    }
  }
  fclose(f);
  return n + 1 < cap ? n + 1 : cap;
}

static int host_checks(void) {
  CHECK(SWBANK_HAS_STATS == 1 && SWBANK_ABI_VERSION == 6, "additive: the ABI version stays 6");
  CHECK(SW_STAT_BINS == 4096 && SW_STAT_DEGENERATE == 1 && SW_STAT_CLAMPED == 2, "constants");
  CHECK(sizeof(sw_statistics) == 48, "sw_statistics is 48 bytes");
  static uint64_t counts[SW_STAT_BINS], sums[SW_STAT_BINS];
  sw_statistics st;
  CHECK(sw_fit_statistics(counts, sums, 128, &st) == SW_OK && st.flags == SW_STAT_DEGENERATE &&
            st.lambda == 0.0 && st.K == 0.0 && st.n_samples == 0, "an empty histogram");
  counts[30] = 6, sums[30] = 6 * 128, counts[40] = 3, sums[40] = 3 * 128;
  CHECK(sw_fit_statistics(counts, sums, 128, &st) == SW_OK && st.flags == 0 && st.lambda > 0.0 &&
            st.K > 0.0 && st.n_samples == 9 && st.min_score == 30 && st.max_score == 40 &&
            st.query_len == 128, "two bins");
  CHECK(sw_fit_statistics(NULL, sums, 128, &st) == SW_ERR_ARG, "NULL counts: SW_ERR_ARG");
  /* the reference's Lambda and K (data/alignments500.txt:13) on its two hits (:20-21) */
  memset(&st, 0, sizeof st);
  st.lambda = 0.1840, st.K = 0.1293, st.query_len = 128;
  const int32_t scores[2] = {78, 72};
  const uint32_t lens[2] = {128, 128};
  double bits[2], ev[2];
  CHECK(sw_hit_significance(&st, scores, lens, 2, 499, bits, ev) == SW_OK, "significance");
  printf("%.1f %.2g\n%.1f %.2g\n", bits[0], ev[0], bits[1], ev[1]);
  CHECK(sw_hit_significance(&st, scores, lens, 2, 499, NULL, NULL) == SW_ERR_ARG, "no output");
  st.flags = SW_STAT_DEGENERATE;
  CHECK(sw_hit_significance(&st, scores, lens, 2, 499, bits, ev) == SW_ERR_ARG, "degenerate");
  uint8_t res[4] = {0, 1, 2, 3};
  const uint64_t offs[1] = {0};
  const uint32_t tl[1] = {4};
  CHECK(sw_shuffle_batch_device(NULL, res, offs, tl, 1, 4, 1, res, NULL) == SW_ERR_ARG &&
            sw_score_histogram_device(NULL, scores, NULL, 2, 1, counts, NULL, NULL, NULL) ==
                SW_ERR_ARG &&
            sw_estimate_statistics_device(NULL, res, offs, tl, 1, 0, 4, 1, 1, &st, NULL) ==
                SW_ERR_ARG &&
            sw_estimate_statistics(NULL, res, 4, offs, tl, 1, 1, 1, &st) == SW_ERR_ARG &&
            sw_hit_significance_device(NULL, &st, scores, offs, tl, 2, 1, 499, bits, ev, NULL) ==
                SW_ERR_ARG,
        "a NULL bank: SW_ERR_ARG");
  printf("host ok\n");
  return 0;
}

static int estimate(const char *qpath, const char *lpath, uint32_t rounds, uint64_t seed) {
  static char qn[1][32], qs[1][512];
  CHECK(read_fa(qpath, qn, qs, 1) == 1, "query file");
  const int n = read_fa(lpath, names, seqs, MAXREC);
  CHECK(n > 0, "library file");
  static uint8_t res[MAXREC * 512], qc[512];
  static uint64_t offs[MAXREC];
  static uint32_t lens[MAXREC];
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    lens[i] = (uint32_t)strlen(seqs[i]);
    offs[i] = total;
    sw_encode_ascii(SW_ALPHABET_DNA, seqs[i], lens[i], res + total);
    total += lens[i];
  }
  const uint32_t qlen = (uint32_t)strlen(qs[0]);
  sw_encode_ascii(SW_ALPHABET_DNA, qs[0], qlen, qc);
  sw_config cfg;
  sw_config_default(&cfg);
  sw_bank *bank = NULL;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  sw_statistics st;
  CHECK(sw_estimate_statistics(bank, res, total, offs, lens, (size_t)n, seed, rounds, &st) ==
            SW_ERR_STATE, "no penalties, no query: SW_ERR_STATE");
  CHECK(sw_set_penalties(bank, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_load_query(bank, 0, qc, qlen) == SW_OK, "query");
  CHECK(sw_estimate_statistics(bank, res, total, offs, lens, (size_t)n, seed, 0, &st) ==
            SW_ERR_ARG, "rounds == 0: SW_ERR_ARG");
  if (sw_estimate_statistics(bank, res, total, offs, lens, (size_t)n, seed, rounds, &st) != SW_OK) {
    fprintf(stderr, "FAIL sw_estimate_statistics: %s\n", sw_last_error(bank));
    return 1;
  }
  CHECK(st.flags == 0 && st.query_len == qlen && st.n_samples == (uint64_t)n * rounds, "the fit");
  printf("kernel %s\n", sw_last_kernel(bank));
  printf("%.17g %.17g %llu\n", st.lambda, st.K, (unsigned long long)st.n_samples);
  sw_bank_destroy(bank);
  printf("stats ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc == 6 && strcmp(argv[1], "gpu") == 0)
    return estimate(argv[2], argv[3], (uint32_t)strtoul(argv[4], NULL, 10),
                    (uint64_t)strtoull(argv[5], NULL, 10));
  fprintf(stderr, "usage: %s host | gpu query.fa library.fa rounds seed\n", argv[0]);
  return 2;
}
