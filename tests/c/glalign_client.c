/* glalign_client.c — a plain C99 client of the alignments of global-local hits of libswbank.so,
 * for tests/test_c_glalign.py.
 *
 *   glalign_client host               what the header promises without a device, prints "host ok"
 *   glalign_client align ENDS Q T...  loads the DNA query Q, scores every DNA target T... (ASCII)
 *                                     with 5 / -4 at -12 / -4 on both strands through
 *                                     sw_score_glocal and aligns all of them through
 *                                     sw_align_glocal_hits: lines
 *                                     "A k score flags q_start q_end t_start t_end cols ids cigar"
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_GLOCAL_ALIGN
#error "swbank.h without the alignments of global-local hits"
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
#define CAP (MAXT * 2 * MAXLEN)

static int host_checks(void) {
  const uint32_t ops[3] = {3u << 4 | SW_CIGAR_I, 40u << 4 | SW_CIGAR_M, 2u << 4 | SW_CIGAR_D};
  char text[32];
  CHECK(SWBANK_ABI_VERSION == 6 && sw_abi_version() == 6, "the ABI version stays 6");
  CHECK(SWBANK_HAS_GLOCAL == 1 && SW_GLOCAL_MAX_QUERY == 1024, "the search is still there");
  CHECK(sw_cigar_string(ops, 3, text, sizeof(text)) == 7 && strcmp(text, "3I40M2D") == 0,
        "a CIGAR may begin and end with a gap");
  CHECK(SW_ALIGN_EMPTY == 1 && SW_ALIGN_NO_PATH == 2 && SW_ALIGN_NO_HIT == 4 &&
            SW_ALIGN_REVERSE == 8,
        "the record's flags");
  printf("host ok\n");
  return 0;
}

static int align(int32_t ends, int nt, const char *q, char **t) {
  static uint8_t qcodes[MAXLEN], res[MAXT * MAXLEN];
  static uint32_t cigar[CAP];
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
  sw_alignment out[MAXT], bare[MAXT];
  int32_t scores[MAXT];
  uint32_t endpos[MAXT];
  uint8_t strands[MAXT];
  size_t used = 99;
  /* a merged-gap bank refuses */
  cfg.gap_model = SW_GAP_MERGED;
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "merged bank create");
  CHECK(sw_align_glocal_hits(other, res, total, offs, lens, NULL, n, ends, 1, NULL, n, NULL, n, out,
                             cigar, CAP, &used) == SW_ERR_UNSUPPORTED,
        "merged gaps: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.gap_model = SW_GAP_GOTOH;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  CHECK(sw_set_penalties(bank, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_align_glocal_hits(bank, res, total, offs, lens, NULL, n, ends, 1, NULL, n, NULL, n, out,
                             cigar, CAP, &used) == SW_ERR_STATE,
        "no query yet: SW_ERR_STATE");
  CHECK(sw_load_query(bank, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_align_glocal_hits(bank, res, total, offs, lens, NULL, n, 0, 1, NULL, n, NULL, n, out,
                             cigar, CAP, &used) == SW_ERR_ARG,
        "ends = 0: SW_ERR_ARG");
  CHECK(sw_align_glocal_hits(bank, res, total, offs, lens, NULL, n, ends, 1, NULL, 0, NULL, n, out,
                             cigar, CAP, &used) == SW_ERR_ARG,
        "neither hit_queries nor hits_per_query: SW_ERR_ARG");
  CHECK(sw_align_glocal_hits(bank, res, total, offs, lens, NULL, n, ends, 1, NULL, n, NULL, n, NULL,
                             cigar, CAP, &used) == SW_ERR_ARG,
        "no records: SW_ERR_ARG");
  CHECK(used == 0, "a refused call resets cigar_used");
  CHECK(sw_score_glocal(bank, res, total, offs, lens, n, ends, 1, scores, endpos, strands) == SW_OK,
        "the score call");
  /* one query, every target: the best-query layout with hits_per_query = n */
  if (sw_align_glocal_hits(bank, res, total, offs, lens, NULL, n, ends, 1, NULL, n, NULL, n, out,
                           cigar, CAP, &used) != SW_OK) {
    fprintf(stderr, "FAIL sw_align_glocal_hits: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  size_t ops = 0;
  for (size_t k = 0; k < n; ++k) {
    const sw_alignment *a = &out[k];
    char text[4 * MAXLEN];
    const int empty = (a->flags & SW_ALIGN_EMPTY) != 0, rev = (a->flags & SW_ALIGN_REVERSE) != 0;
    CHECK(a->index == k && a->id == k, "the record names its target");
    CHECK(a->score == scores[k], "the record's score is the score call's");
    CHECK(rev == (strands[k] != 0), "the strand flag is the score call's strand");
    if (ends == SW_ENDS_QUERY)
      CHECK(empty ? endpos[k] == SW_END_NONE : (rev ? a->t_start : a->t_end) == endpos[k],
            "the record ends where the score call ends (QUERY)");
    if (ends == SW_ENDS_TARGET)
      CHECK(empty ? endpos[k] == SW_END_NONE : a->q_end == endpos[k],
            "the record ends where the score call ends (TARGET)");
    CHECK(a->cigar_offset == (a->cigar_len ? ops : 0), "the ops are packed in hit order");
    ops += a->cigar_len;
    sw_cigar_string(cigar + a->cigar_offset, a->cigar_len, text, sizeof(text));
    printf("A %zu %d %u %u %u %u %u %u %u %s\n", k, a->score, a->flags, a->q_start, a->q_end,
           a->t_start, a->t_end, a->n_columns, a->n_identities, a->cigar_len ? text : "*");
  }
  CHECK(used == ops, "cigar_used counts the ops");
  /* coordinates only */
  CHECK(sw_align_glocal_hits(bank, res, total, offs, lens, NULL, n, ends, 1, NULL, n, NULL, n, bare,
                             NULL, 0, NULL) == SW_OK,
        "cigar may be NULL");
  for (size_t k = 0; k < n; ++k) {
    CHECK(bare[k].score == out[k].score && bare[k].t_start == out[k].t_start &&
              bare[k].t_end == out[k].t_end && bare[k].q_start == out[k].q_start &&
              bare[k].q_end == out[k].q_end,
          "... and the coordinates are the same");
    CHECK(bare[k].cigar_len == 0 &&
              bare[k].flags == ((out[k].flags & SW_ALIGN_EMPTY) ? out[k].flags
                                                                : out[k].flags | SW_ALIGN_NO_PATH),
          "... without a path");
  }
  sw_bank_destroy(bank);
  printf("align ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc >= 5 && strcmp(argv[1], "align") == 0)
    return align((int32_t)strtol(argv[2], NULL, 10), argc - 4, argv[3], argv + 4);
  fprintf(stderr, "usage: %s host | align ENDS Q T0 [T1 ...]\n", argv[0]);
  return 2;
}
