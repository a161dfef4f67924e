/* strand_client.c — a plain C99 client of the both-strand calls of libswbank.so, for
 * tests/test_c_strands.py.
 *
 *   strand_client host            the new constants and sw_revcomp_codes from C (no device),
 *                                 prints "host ok"
 *   strand_client search Q T...   loads the DNA query Q, scores every target T... (ASCII) on both
 *                                 strands with the reference penalties through sw_score_strands
 *                                 (lines "S k score strand") and aligns every target on its
 *                                 strand through sw_align_strand_hits (lines "A k ..."); a record
 *                                 is "index score flags q_start q_end t_start t_end columns
 *                                 identities cigar" (cigar "-" when there are no ops).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_STRANDS
#error "swbank.h without the both-strand calls"
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
#define MAXOPS 8192

static int host_checks(void) {
  CHECK(SW_ALIGN_REVERSE == 8 &&
            (SW_ALIGN_REVERSE & (SW_ALIGN_EMPTY | SW_ALIGN_NO_PATH | SW_ALIGN_NO_HIT)) == 0,
        "SW_ALIGN_REVERSE is a flag of its own");
  CHECK(SWBANK_ABI_VERSION == 6, "the ABI version stays 6");
  uint8_t in[7], out[7], want[7] = {SW_DNA_N, SW_DNA_C, SW_DNA_T, SW_DNA_G, SW_DNA_A, 9, SW_DNA_A};
  /* T 9 T C A G N  ->  N C T G A 9 A */
  in[0] = SW_DNA_T, in[1] = 9, in[2] = SW_DNA_T, in[3] = SW_DNA_C, in[4] = SW_DNA_A;
  in[5] = SW_DNA_G, in[6] = SW_DNA_N;
  CHECK(sw_revcomp_codes(in, 7, out) == 7 && memcmp(out, want, 7) == 0, "sw_revcomp_codes");
  CHECK(sw_revcomp_codes(in, 7, in) == 7 && memcmp(in, want, 7) == 0, "... in place");
  CHECK(sw_revcomp_codes(NULL, 7, out) == 0, "... a NULL argument");
  printf("host ok\n");
  return 0;
}

static void print_record(const sw_alignment *a, const uint32_t *cig) {
  char text[512] = "-";
  if (a->cigar_len) sw_cigar_string(cig + a->cigar_offset, a->cigar_len, text, sizeof text);
  printf("%lld %d %u %u %u %u %u %u %u %s\n", (long long)a->index, a->score, a->flags, a->q_start,
         a->q_end, a->t_start, a->t_end, a->n_columns, a->n_identities, text);
}

static int search(int nt, const char *q, char **t) {
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
  sw_bank *bank = NULL;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  int32_t scores[MAXT];
  uint8_t strands[MAXT];
  static sw_alignment al[MAXT];
  static uint32_t cig[MAXOPS];
  size_t used = 0;
  CHECK(sw_set_penalties(bank, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_score_strands(bank, res, total, offs, lens, n, scores, strands) == SW_ERR_STATE,
        "no query yet: SW_ERR_STATE");
  CHECK(sw_load_query(bank, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_score_strands(bank, res, total, offs, lens, n, NULL, strands) == SW_ERR_ARG,
        "no scores: SW_ERR_ARG");
  if (sw_score_strands(bank, res, total, offs, lens, n, scores, strands) != SW_OK) {
    fprintf(stderr, "FAIL sw_score_strands: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  for (size_t k = 0; k < n; ++k) printf("S %zu %d %u\n", k, scores[k], strands[k]);
  /* every target on its strand: one query, the [1, n] layout, no hit list */
  if (sw_align_strand_hits(bank, res, total, offs, lens, NULL, n, strands, NULL, n, NULL, n, al,
                           cig, MAXOPS, &used) != SW_OK) {
    fprintf(stderr, "FAIL sw_align_strand_hits: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  for (size_t k = 0; k < n; ++k) {
    printf("A %zu ", k);
    print_record(&al[k], cig);
  }
  sw_bank_destroy(bank);
  printf("search ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc >= 4 && strcmp(argv[1], "search") == 0) return search(argc - 3, argv[2], argv + 3);
  fprintf(stderr, "usage: %s host | search Q T0 [T1 ...]\n", argv[0]);
  return 2;
}
