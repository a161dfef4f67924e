/* align_client.c — a plain C99 client of the alignment calls of libswbank.so, for
 * tests/test_c_align.py.
 *
 *   align_client host                     sw_cigar_string from C (no device), prints "host ok"
 *   align_client align q.fa lib.fa NAME   aligns record NAME of lib.fa (and the record before
 *                                         it) against q.fa with the reference penalties through
 *                                         sw_align_hits and prints NAME's record as
 *                                         "score q_start q_end t_start t_end columns identities
 *                                         cigar", then "align ok".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#ifndef SWBANK_HAS_ALIGN
#error "swbank.h without the alignment calls"
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
  const uint32_t ops[5] = {15u << 4 | SW_CIGAR_M, 2u << 4 | SW_CIGAR_I, 17u << 4 | SW_CIGAR_M,
                           4u << 4 | SW_CIGAR_D, 13u << 4 | SW_CIGAR_M};
  char buf[32];
  CHECK(sw_cigar_string(ops, 5, NULL, 0) == 13, "needed length");
  CHECK(sw_cigar_string(ops, 5, buf, sizeof buf) == 13 && strcmp(buf, "15M2I17M4D13M") == 0,
        "cigar text");
  CHECK(sw_cigar_string(ops, 5, buf, 4) == 13 && strcmp(buf, "15M") == 0, "truncation");
  CHECK(sizeof(sw_alignment) == 56, "sw_alignment is 56 bytes");
  printf("host ok\n");
  return 0;
}

static int align(const char *qpath, const char *lpath, const char *want) {
  static char qn[1][32], qs[1][512];
  CHECK(read_fa(qpath, qn, qs, 1) == 1, "query file");
  const int n = read_fa(lpath, names, seqs, MAXREC);
  CHECK(n > 0, "library file");
  int at = -1;
  for (int k = 0; k < n; ++k)
    if (strcmp(names[k], want) == 0) at = k;
  CHECK(at > 0, "record not found (or first)");
  static uint8_t res[MAXREC * 512], qc[512];
  static uint64_t offs[MAXREC];
  static uint32_t lens[MAXREC];
  size_t total = 0;
  for (int k = 0; k < n; ++k) {
    lens[k] = (uint32_t)strlen(seqs[k]);
    offs[k] = total;
    sw_encode_ascii(SW_ALPHABET_DNA, seqs[k], lens[k], res + total);
    total += lens[k];
  }
  const uint32_t qlen = (uint32_t)strlen(qs[0]);
  sw_encode_ascii(SW_ALPHABET_DNA, qs[0], qlen, qc);
  sw_config cfg;
  sw_config_default(&cfg);
  sw_bank *bank = NULL;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  const uint64_t hits[2] = {(uint64_t)at - 1, (uint64_t)at};
  sw_alignment al[2];
  uint32_t cig[1024];
  size_t used = 0;
  CHECK(sw_align_hits(bank, res, total, offs, lens, NULL, (size_t)n, hits, 2, al, cig, 1024,
                      &used) == SW_ERR_STATE, "no penalties yet: SW_ERR_STATE");
  CHECK(sw_set_penalties(bank, 5, -4, -12, -4) == SW_OK, "penalties");
  CHECK(sw_load_query(bank, 0, qc, qlen) == SW_OK, "query");
  const uint64_t bad[1] = {(uint64_t)n};
  CHECK(sw_align_hits(bank, res, total, offs, lens, NULL, (size_t)n, bad, 1, al, cig, 1024,
                      &used) == SW_ERR_ARG, "a hit >= n: SW_ERR_ARG");
  if (sw_align_hits(bank, res, total, offs, lens, NULL, (size_t)n, hits, 2, al, cig, 1024,
                    &used) != SW_OK) {
    fprintf(stderr, "FAIL sw_align_hits: %s\n", sw_last_error(bank));
    return 1;
  }
  const sw_alignment *a = &al[1];
  CHECK(a->index == (uint64_t)at && a->id == (uint64_t)at && a->flags == 0, "record");
  CHECK(used == (size_t)al[0].cigar_len + a->cigar_len && a->cigar_offset == al[0].cigar_len,
        "ops packed back to back");
  char text[256];
  CHECK(sw_cigar_string(cig + a->cigar_offset, a->cigar_len, text, sizeof text) < sizeof text,
        "cigar text");
  printf("kernel %s\n", sw_last_kernel(bank));
  printf("%d %u %u %u %u %u %u %s\n", a->score, a->q_start, a->q_end, a->t_start, a->t_end,
         a->n_columns, a->n_identities, text);
  sw_bank_destroy(bank);
  printf("align ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc == 5 && strcmp(argv[1], "align") == 0) return align(argv[2], argv[3], argv[4]);
  fprintf(stderr, "usage: %s host | align query.fa library.fa NAME\n", argv[0]);
  return 2;
}
