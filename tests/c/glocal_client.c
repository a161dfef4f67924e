/* glocal_client.c — a plain C99 client of the global-local search of libswbank.so, for
 * tests/test_c_glocal.py.
 *
 *   glocal_client host               the new constants from C (no device), prints "host ok"
 *   glocal_client search ENDS Q T... loads the DNA query Q and scores every DNA target T...
 *                                    (ASCII) with 5 / -4 and -12 / -4 on both strands through
 *                                    sw_score_glocal: lines "S k score end strand"
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_GLOCAL
#error "swbank.h without the global-local search"
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

static int host_checks(void) {
  CHECK(SW_GLOCAL_MAX_QUERY == 1024, "queries of 1,024 rows");
  CHECK(SW_ENDS_QUERY == 1 && SW_ENDS_TARGET == 2 && SW_ENDS_BOTH == 3, "the three modes");
  CHECK(SW_END_NONE == UINT32_MAX, "the boundary's end position");
  CHECK(SWBANK_ABI_VERSION == 6 && sw_abi_version() == 6, "the ABI version stays 6");
  CHECK(SWBANK_HAS_FSHIFT == 1 && SWBANK_HAS_STRANDS == 1, "the earlier searches are still there");
  CHECK(sw_score_glocal(NULL, NULL, 0, NULL, NULL, 1, SW_ENDS_QUERY, 0, NULL, NULL, NULL) ==
            SW_ERR_ARG,
        "a NULL bank: SW_ERR_ARG");
  printf("host ok\n");
  return 0;
}

static int search(int32_t ends, int nt, const char *q, char **t) {
  static uint8_t qcodes[MAXLEN], res[MAXT * MAXLEN];
  uint64_t offs[MAXT];
  uint32_t lens[MAXT];
  size_t total = 0;
  CHECK(nt >= 1 && nt <= MAXT, "1..16 targets");
  CHECK(strlen(q) <= MAXLEN, "query too long");
  const uint32_t qlen = (uint32_t)strlen(q);
  sw_encode_ascii(SW_ALPHABET_DNA, q, qlen, qcodes);
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
  int32_t scores[MAXT], again[MAXT];
  uint32_t end_pos[MAXT];
  uint8_t strands[MAXT];
  /* a merged-gap bank refuses; so does a protein bank asked for both strands */
  cfg.gap_model = SW_GAP_MERGED;
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "merged bank create");
  CHECK(sw_set_penalties(other, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_load_query(other, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_score_glocal(other, res, total, offs, lens, n, ends, 1, scores, end_pos, strands) ==
            SW_ERR_UNSUPPORTED,
        "merged gaps: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.gap_model = SW_GAP_GOTOH;
  cfg.alphabet = SW_ALPHABET_PROTEIN;
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "protein bank create");
  CHECK(sw_score_glocal(other, res, total, offs, lens, n, ends, 1, scores, end_pos, strands) ==
            SW_ERR_UNSUPPORTED,
        "both strands of a protein bank: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.alphabet = SW_ALPHABET_DNA;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  CHECK(sw_score_glocal(bank, res, total, offs, lens, n, ends, 1, scores, end_pos, strands) ==
            SW_ERR_STATE,
        "no query yet: SW_ERR_STATE");
  CHECK(sw_set_penalties(bank, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_load_query(bank, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_score_glocal(bank, res, total, offs, lens, n, ends, 1, NULL, end_pos, strands) ==
            SW_ERR_ARG,
        "no scores: SW_ERR_ARG");
  CHECK(sw_score_glocal(bank, res, total, offs, lens, n, 0, 1, scores, end_pos, strands) ==
            SW_ERR_ARG,
        "ends = 0: SW_ERR_ARG");
  CHECK(sw_score_glocal(bank, res, total, offs, lens, n, 4, 1, scores, end_pos, strands) ==
            SW_ERR_ARG,
        "ends = 4: SW_ERR_ARG");
  CHECK(sw_score_glocal(bank, res, total, offs, lens, 0, ends, 1, NULL, NULL, NULL) == SW_OK,
        "an empty batch is fine");
  if (sw_score_glocal(bank, res, total, offs, lens, n, ends, 1, scores, end_pos, strands) !=
      SW_OK) {
    fprintf(stderr, "FAIL sw_score_glocal: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  for (size_t k = 0; k < n; ++k) {
    if (end_pos[k] == SW_END_NONE)
      printf("S %zu %d none %u\n", k, scores[k], strands[k]);
    else
      printf("S %zu %d %u %u\n", k, scores[k], end_pos[k], strands[k]);
  }
  CHECK(sw_score_glocal(bank, res, total, offs, lens, n, ends, 1, again, NULL, NULL) == SW_OK,
        "end_pos_out and strands_out may be NULL");
  CHECK(memcmp(again, scores, n * sizeof(int32_t)) == 0, "... and the scores are the same");
  sw_bank_destroy(bank);
  printf("search ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc >= 5 && strcmp(argv[1], "search") == 0)
    return search((int32_t)strtol(argv[2], NULL, 10), argc - 4, argv[3], argv + 4);
  fprintf(stderr, "usage: %s host | search ENDS Q T0 [T1 ...]\n", argv[0]);
  return 2;
}
