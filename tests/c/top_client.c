/* top_client.c — a plain C99 client of the top-hits calls of libswbank.so, for
 * tests/test_c_top.py.
 *
 *   top_client host               the macros and the argument errors that need no device, prints
 *                                 "host ok"
 *   top_client gpu q.fa lib.fa K  scores lib.fa against q.fa with the reference penalties through
 *                                 sw_score_batch, picks the K best with sw_top_hits and prints
 *                                 "name score" per hit, then "top ok".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#ifndef SWBANK_HAS_TOPK
#error "swbank.h without the top-hits calls"
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
  CHECK(SWBANK_HAS_TOPK == 1 && SWBANK_ABI_VERSION == 6, "additive: the ABI version stays 6");
  CHECK(SW_TOP_MAX_K == 4096, "SW_TOP_MAX_K");
  CHECK(SW_HIT_NONE == UINT64_MAX && sizeof(SW_HIT_NONE) == 8, "SW_HIT_NONE");
  const int32_t scores[3] = {3, 9, 9};
  uint64_t hits[2] = {7, 7};
  CHECK(sw_top_hits(NULL, scores, NULL, 3, 1, 2, INT32_MIN, hits, NULL, NULL, NULL) == SW_ERR_ARG,
        "a NULL bank: SW_ERR_ARG");
  CHECK(sw_top_hits_device(NULL, scores, NULL, 3, 1, 2, INT32_MIN, hits, NULL, NULL, NULL, NULL) ==
            SW_ERR_ARG,
        "a NULL bank: SW_ERR_ARG (device call)");
  CHECK(hits[0] == 7 && hits[1] == 7, "nothing written");
  printf("host ok\n");
  return 0;
}

static int top(const char *qpath, const char *lpath, size_t k) {
  static char qn[1][32], qs[1][512];
  CHECK(k >= 1 && k <= 64, "K in 1..64");
  CHECK(read_fa(qpath, qn, qs, 1) == 1, "query file");
  const int n = read_fa(lpath, names, seqs, MAXREC);
  CHECK(n > 0, "library file");
  static uint8_t res[MAXREC * 512], qc[512];
  static uint64_t offs[MAXREC];
  static uint32_t lens[MAXREC];
  static int32_t scores[MAXREC];
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
  uint64_t hits[64], hit_ids[64];
  int32_t hit_scores[64];
  uint32_t count = 0;
  /* the argument errors; the call needs neither penalties nor a query */
  CHECK(sw_top_hits(bank, scores, NULL, (size_t)n, 1, 0, INT32_MIN, hits, NULL, NULL, NULL) ==
            SW_ERR_ARG, "k == 0: SW_ERR_ARG");
  CHECK(sw_top_hits(bank, scores, NULL, (size_t)n, 1, SW_TOP_MAX_K + 1, INT32_MIN, hits, NULL,
                    NULL, NULL) == SW_ERR_ARG, "k > SW_TOP_MAX_K: SW_ERR_ARG");
  CHECK(sw_top_hits(bank, scores, NULL, (size_t)n, 1, k, INT32_MIN, NULL, NULL, NULL, NULL) ==
            SW_ERR_ARG, "NULL hits: SW_ERR_ARG");
  CHECK(sw_set_penalties(bank, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_load_query(bank, 0, qc, qlen) == SW_OK, "query");
  CHECK(sw_score_batch(bank, res, total, offs, lens, NULL, (size_t)n, scores) == SW_OK, "scores");
  if (sw_top_hits(bank, scores, NULL, (size_t)n, 1, k, INT32_MIN, hits, hit_scores, hit_ids,
                  &count) != SW_OK) {
    fprintf(stderr, "FAIL sw_top_hits: %s\n", sw_last_error(bank));
    return 1;
  }
  CHECK(count == (k < (size_t)n ? k : (size_t)n), "count");
  printf("kernel %s\n", sw_last_kernel(bank));
  for (uint32_t j = 0; j < count; ++j) {
    CHECK(hits[j] < (uint64_t)n && hit_ids[j] == hits[j] && hit_scores[j] == scores[hits[j]],
          "hit record");
    printf("%s %d\n", names[hits[j]], hit_scores[j]);
  }
  uint64_t best_id = 0;
  int32_t best = 0;
  CHECK(sw_best_hit(bank, scores, NULL, (size_t)n, &best_id, &best) == SW_OK && best_id == hits[0],
        "the first hit is sw_best_hit's");
  sw_bank_destroy(bank);
  printf("top ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc == 5 && strcmp(argv[1], "gpu") == 0)
    return top(argv[2], argv[3], (size_t)strtoul(argv[4], NULL, 10));
  fprintf(stderr, "usage: %s host | gpu query.fa library.fa K\n", argv[0]);
  return 2;
}
