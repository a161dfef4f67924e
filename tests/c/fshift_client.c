/* fshift_client.c — a plain C99 client of the frameshift-tolerant translated search of
 * libswbank.so, for tests/test_c_fshift.py.
 *
 *   fshift_client host              the new constants from C (no device), prints "host ok"
 *   fshift_client search FS Q T...  loads the protein query Q and scores every DNA target T...
 *                                   (ASCII) with BLOSUM62 -11/-1 and the frameshift penalty FS
 *                                   through sw_score_fshift: lines "S k score strand"
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_FSHIFT
#error "swbank.h without the frameshift-tolerant search"
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
  CHECK(SW_FSHIFT_MAX_QUERY >= 1024, "queries of at least 1,024 rows");
  CHECK(SWBANK_ABI_VERSION == 6 && sw_abi_version() == 6, "the ABI version stays 6");
  CHECK(SWBANK_HAS_FRAMES == 1 && SW_FRAME_COUNT == 6, "the six-frame search is still there");
  printf("host ok\n");
  return 0;
}

static int search(int32_t fs, int nt, const char *q, char **t) {
  static uint8_t qcodes[MAXLEN], res[MAXT * MAXLEN];
  uint64_t offs[MAXT];
  uint32_t lens[MAXT];
  size_t total = 0;
  CHECK(nt >= 1 && nt <= MAXT, "1..16 targets");
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
  int32_t scores[MAXT], again[MAXT];
  uint8_t strands[MAXT];
  /* a DNA bank and a merged-gap protein bank refuse */
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "DNA bank create");
  CHECK(sw_score_fshift(other, res, total, offs, lens, n, NULL, fs, scores, strands) ==
            SW_ERR_UNSUPPORTED,
        "a DNA bank: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.alphabet = SW_ALPHABET_PROTEIN;
  cfg.gap_model = SW_GAP_MERGED;
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "merged bank create");
  CHECK(sw_load_query(other, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_score_fshift(other, res, total, offs, lens, n, NULL, fs, scores, strands) ==
            SW_ERR_UNSUPPORTED,
        "merged gaps: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.gap_model = SW_GAP_GOTOH;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  CHECK(sw_score_fshift(bank, res, total, offs, lens, n, NULL, fs, scores, strands) == SW_ERR_STATE,
        "no query yet: SW_ERR_STATE");
  CHECK(sw_load_query(bank, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_score_fshift(bank, res, total, offs, lens, n, NULL, fs, NULL, strands) == SW_ERR_ARG,
        "no scores: SW_ERR_ARG");
  CHECK(sw_score_fshift(bank, res, total, offs, lens, n, NULL, 1, scores, strands) == SW_ERR_ARG,
        "a positive penalty: SW_ERR_ARG");
  CHECK(sw_score_fshift(bank, res, total, offs, lens, n, NULL, -32768, scores, strands) ==
            SW_ERR_ARG,
        "a penalty below -32767: SW_ERR_ARG");
  CHECK(sw_score_fshift(bank, res, total, offs, lens, 0, NULL, fs, NULL, NULL) == SW_OK,
        "an empty batch is fine");
  if (sw_score_fshift(bank, res, total, offs, lens, n, NULL, fs, scores, strands) != SW_OK) {
    fprintf(stderr, "FAIL sw_score_fshift: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  for (size_t k = 0; k < n; ++k) printf("S %zu %d %u\n", k, scores[k], strands[k]);
  CHECK(sw_score_fshift(bank, res, total, offs, lens, n, NULL, fs, again, NULL) == SW_OK,
        "strands_out may be NULL");
  CHECK(memcmp(again, scores, n * sizeof(int32_t)) == 0, "... and the scores are the same");
  sw_bank_destroy(bank);
  printf("search ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc >= 5 && strcmp(argv[1], "search") == 0)
    return search((int32_t)strtol(argv[2], NULL, 10), argc - 4, argv[3], argv + 4);
  fprintf(stderr, "usage: %s host | search FS Q T0 [T1 ...]\n", argv[0]);
  return 2;
}
