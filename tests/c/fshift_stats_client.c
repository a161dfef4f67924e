/* fshift_stats_client.c — a plain C99 client of the frameshift search's statistics of
 * libswbank.so, for tests/test_c_fshift_stats.py.
 *
 *   fshift_stats_client host                  the macro and the NULL-bank errors from C (no
 *                                             device), prints "host ok"
 *   fshift_stats_client gpu FS R S Q T...     loads the protein query Q, estimates lambda and K
 *                                             against R seeded shuffles (seed S) of the DNA
 *                                             targets T... (ASCII) with BLOSUM62 -11/-1 and the
 *                                             frameshift penalty FS through
 *                                             sw_estimate_fshift_statistics; prints "kernel ...",
 *                                             "lambda K n_samples min max clamped", the bits and E
 *                                             of the best hit of sw_score_fshift, then "stats ok"
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_FSHIFT_STATS
#error "swbank.h without the statistics of frameshift hits"
#endif

#define CHECK(cond, msg)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, msg); \
      return 1;                                                     \
    }                                                               \
  } while (0)

#define MAXT 256
#define MAXLEN 512

static int host_checks(void) {
  CHECK(SWBANK_HAS_FSHIFT_STATS == 1 && SWBANK_HAS_FSHIFT == 1 && SWBANK_HAS_STATS == 1,
        "the macros");
  CHECK(SWBANK_ABI_VERSION == 6 && sw_abi_version() == 6, "additive: the ABI version stays 6");
  uint8_t res[6] = {0, 1, 2, 3, 0, 1};
  const uint64_t offs[1] = {0};
  const uint32_t lens[1] = {6};
  sw_statistics st;
  memset(&st, 0, sizeof st);
  CHECK(sw_estimate_fshift_statistics(NULL, res, 6, offs, lens, 1, NULL, -15, 1, 1, &st) ==
                SW_ERR_ARG &&
            sw_estimate_fshift_statistics_device(NULL, res, offs, lens, 1, 6, NULL, -15, 1, 1, &st,
                                                 NULL) == SW_ERR_ARG,
        "a NULL bank: SW_ERR_ARG");
  CHECK(st.n_samples == 0 && st.lambda == 0.0, "... and nothing is written");
  printf("host ok\n");
  return 0;
}

static int estimate(int32_t fs, uint32_t rounds, uint64_t seed, int nt, const char *q, char **t) {
  static uint8_t qcodes[MAXLEN], res[MAXT * MAXLEN];
  static uint64_t offs[MAXT];
  static uint32_t lens[MAXT];
  static int32_t scores[MAXT];
  size_t total = 0;
  CHECK(nt >= 1 && nt <= MAXT, "1..256 targets");
  CHECK(strlen(q) <= MAXLEN, "query too long");
  const uint32_t qlen = (uint32_t)strlen(q);
  sw_encode_ascii(SW_ALPHABET_PROTEIN, q, qlen, qcodes);
  for (int k = 0; k < nt; ++k) {
    CHECK(strlen(t[k]) <= MAXLEN, "target too long");
    lens[k] = (uint32_t)strlen(t[k]);
    offs[k] = total;
    sw_encode_ascii(SW_ALPHABET_DNA, t[k], lens[k], res + total);
    total += lens[k];
  }
  const size_t n = (size_t)nt;
  sw_config cfg;
  sw_config_default(&cfg);
  sw_bank *bank = NULL, *other = NULL;
  sw_statistics st;
  /* the refusals of sw_score_fshift come first */
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "DNA bank create");
  CHECK(sw_estimate_fshift_statistics(other, res, total, offs, lens, n, NULL, fs, seed, rounds,
                                      &st) == SW_ERR_UNSUPPORTED,
        "a DNA bank: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.alphabet = SW_ALPHABET_PROTEIN;
  cfg.gap_model = SW_GAP_GOTOH;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  CHECK(sw_estimate_fshift_statistics(bank, res, total, offs, lens, n, NULL, fs, seed, rounds,
                                      &st) == SW_ERR_STATE,
        "no query yet: SW_ERR_STATE");
  CHECK(sw_load_query(bank, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_estimate_fshift_statistics(bank, res, total, offs, lens, n, NULL, 1, seed, rounds,
                                      &st) == SW_ERR_ARG,
        "a positive penalty: SW_ERR_ARG");
  CHECK(sw_estimate_fshift_statistics(bank, res, total, offs, lens, n, NULL, fs, seed, 0, &st) ==
            SW_ERR_ARG,
        "rounds == 0: SW_ERR_ARG");
  CHECK(sw_estimate_fshift_statistics(bank, res, total, offs, lens, n, NULL, fs, seed, rounds,
                                      NULL) == SW_ERR_ARG,
        "no out: SW_ERR_ARG");
  if (sw_estimate_fshift_statistics(bank, res, total, offs, lens, n, NULL, fs, seed, rounds,
                                    &st) != SW_OK) {
    fprintf(stderr, "FAIL sw_estimate_fshift_statistics: %s\n", sw_last_error(bank));
    return 1;
  }
  CHECK(st.flags == 0 && st.query_len == qlen, "the fit");
  printf("kernel %s\n", sw_last_kernel(bank));
  printf("%.17g %.17g %llu %d %d %llu\n", st.lambda, st.K, (unsigned long long)st.n_samples,
         st.min_score, st.max_score, (unsigned long long)st.n_clamped);
  /* the significance of the search's best hit: lengths in nucleotides, db_size the targets */
  CHECK(sw_score_fshift(bank, res, total, offs, lens, n, NULL, fs, scores, NULL) == SW_OK,
        "the search itself");
  size_t best = 0;
  for (size_t k = 1; k < n; ++k)
    if (scores[k] > scores[best]) best = k;
  double bits, ev;
  CHECK(sw_hit_significance(&st, &scores[best], &lens[best], 1, (uint64_t)n, &bits, &ev) == SW_OK,
        "significance");
  printf("H %zu %d %.17g %.17g\n", best, scores[best], bits, ev);
  sw_bank_destroy(bank);
  printf("stats ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc >= 7 && strcmp(argv[1], "gpu") == 0)
    return estimate((int32_t)strtol(argv[2], NULL, 10), (uint32_t)strtoul(argv[3], NULL, 10),
                    (uint64_t)strtoull(argv[4], NULL, 10), argc - 6, argv[5], argv + 6);
  fprintf(stderr, "usage: %s host | gpu FS rounds seed Q T0 [T1 ...]\n", argv[0]);
  return 2;
}
