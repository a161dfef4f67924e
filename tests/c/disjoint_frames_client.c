/* disjoint_frames_client.c — a plain C99 client of the non-intersecting alignments over reading
 * frames of libswbank.so, for tests/test_c_disjoint_frames.py.
 *
 *   disjoint_frames_client host              what the header promises without a device, "host ok"
 *   disjoint_frames_client align ROUNDS MIN Q T...
 *                                            loads the protein query Q, scores every DNA target
 *                                            T... (ASCII) with BLOSUM62 -11/-1 through
 *                                            sw_score_frames and aligns all of them through
 *                                            sw_align_disjoint_frame_hits: lines "A k r score
 *                                            flags q_start q_end t_start t_end cols ids cigar"
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_DISJOINT_FRAMES
#error "swbank.h without the non-intersecting alignments over reading frames"
#endif

#define CHECK(cond, msg)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, msg); \
      return 1;                                                     \
    }                                                               \
  } while (0)

#define MAXT 8
#define MAXR 8
#define MAXLEN 1024
#define CAP (MAXT * MAXR * MAXLEN)

static int host_checks(void) {
  CHECK(SWBANK_ABI_VERSION == 6 && sw_abi_version() == 6, "the ABI version stays 6");
  CHECK(SWBANK_HAS_DISJOINT_ALIGN && SW_DISJOINT_MAX_QUERY == 1024 && SW_DISJOINT_MAX_ROUNDS == 64,
        "the disjoint call's limits apply");
  CHECK(SW_FRAME_COUNT == 6 && SW_ALIGN_FRAME_SHIFT == 4 && SW_ALIGN_FRAME_MASK == 0x30 &&
            SW_ALIGN_REVERSE == 8,
        "the frame's flags");
  CHECK(sw_align_disjoint_frame_hits(NULL, NULL, 0, NULL, NULL, NULL, 0, NULL, 1, 1, NULL, 0, NULL,
                                     0, NULL, NULL, 0, NULL) == SW_ERR_ARG,
        "no bank: SW_ERR_ARG");
  CHECK(sw_align_disjoint_frame_hits_device(NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, 1, 1, NULL, 0,
                                            NULL, 0, NULL, NULL, 0, NULL) == SW_ERR_ARG,
        "no bank: SW_ERR_ARG (device form)");
  printf("host ok\n");
  return 0;
}

static int align(uint32_t rounds, int32_t min_score, int nt, const char *q, char **t) {
  static uint8_t qcodes[MAXLEN], res[MAXT * MAXLEN];
  static uint32_t cigar[CAP];
  static sw_alignment out[MAXT * MAXR], bare[MAXT * MAXR];
  uint64_t offs[MAXT];
  uint32_t lens[MAXT];
  size_t total = 0;
  CHECK(nt >= 1 && nt <= MAXT, "1..8 targets");
  CHECK(rounds >= 1 && rounds <= MAXR, "1..8 rounds");
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
  int32_t scores[MAXT];
  uint8_t frames[MAXT], bad_table[64];
  size_t used = 99;
  memset(bad_table, 0, sizeof(bad_table));
  bad_table[63] = SW_PROTEIN_ALPHA;
  /* a DNA bank refuses, and so does a merged-gap protein bank */
  cfg.gap_model = SW_GAP_GOTOH;
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "DNA bank create");
  CHECK(sw_align_disjoint_frame_hits(other, res, total, offs, lens, NULL, n, NULL, rounds,
                                     min_score, NULL, n, NULL, n, out, cigar, CAP,
                                     &used) == SW_ERR_UNSUPPORTED,
        "a DNA bank: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.alphabet = SW_ALPHABET_PROTEIN;
  cfg.gap_model = SW_GAP_MERGED;
  CHECK(sw_bank_create(&other, &cfg) == SW_OK, "merged bank create");
  CHECK(sw_align_disjoint_frame_hits(other, res, total, offs, lens, NULL, n, NULL, rounds,
                                     min_score, NULL, n, NULL, n, out, cigar, CAP,
                                     &used) == SW_ERR_UNSUPPORTED,
        "merged gaps: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(other);
  cfg.gap_model = SW_GAP_GOTOH;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  CHECK(sw_align_disjoint_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, rounds,
                                     min_score, NULL, n, NULL, n, out, cigar, CAP,
                                     &used) == SW_ERR_STATE,
        "no query yet: SW_ERR_STATE");
  CHECK(sw_load_query(bank, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_align_disjoint_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, 0, min_score,
                                     NULL, n, NULL, n, out, cigar, CAP, &used) == SW_ERR_ARG,
        "rounds = 0: SW_ERR_ARG");
  CHECK(sw_align_disjoint_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, rounds, 0, NULL,
                                     n, NULL, n, out, cigar, CAP, &used) == SW_ERR_ARG,
        "min_score = 0: SW_ERR_ARG");
  CHECK(sw_align_disjoint_frame_hits(bank, res, total, offs, lens, NULL, n, bad_table, rounds,
                                     min_score, NULL, n, NULL, n, out, cigar, CAP,
                                     &used) == SW_ERR_ARG,
        "a codon table entry of 24: SW_ERR_ARG");
  CHECK(sw_align_disjoint_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, rounds,
                                     min_score, NULL, n, NULL, n, NULL, cigar, CAP,
                                     &used) == SW_ERR_ARG,
        "no records: SW_ERR_ARG");
  CHECK(used == 0, "a refused call resets cigar_used");
  CHECK(sw_score_frames(bank, res, total, offs, lens, n, NULL, scores, frames) == SW_OK,
        "the six-frame search");
  /* one query, every target: hits_per_query = n, no hit list */
  if (sw_align_disjoint_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, rounds, min_score,
                                   NULL, n, NULL, n, out, cigar, CAP, &used) != SW_OK) {
    fprintf(stderr, "FAIL sw_align_disjoint_frame_hits: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  size_t ops = 0;
  for (size_t k = 0; k < n; ++k) {
    for (uint32_t r = 0; r < rounds; ++r) {
      const sw_alignment *a = &out[k * rounds + r];
      char text[4 * MAXLEN];
      const uint32_t f = ((a->flags & SW_ALIGN_FRAME_MASK) >> SW_ALIGN_FRAME_SHIFT) +
                         ((a->flags & SW_ALIGN_REVERSE) ? 3u : 0u);
      CHECK(a->index == k && a->id == k, "the record names its DNA target");
      if (r == 0 && scores[k] >= min_score)
        CHECK(a->score == scores[k] && f == frames[k],
              "record 0 has the search's score and frame");
      if (r == 0 && scores[k] < min_score) CHECK(a->score == 0, "record 0 under min_score is empty");
      if (r > 0) CHECK(a->score <= a[-1].score, "scores never increase");
      if (a->flags & SW_ALIGN_EMPTY)
        CHECK(a->flags == SW_ALIGN_EMPTY && a->score == 0 && a->t_end == 0,
              "an empty record has no frame bits");
      else
        CHECK(a->t_end < lens[k] && a->t_start <= a->t_end && (a->t_end - a->t_start) % 3 == 2,
              "whole codons on the forward target");
      CHECK(a->cigar_offset == (a->cigar_len ? ops : 0), "the ops are packed in record order");
      ops += a->cigar_len;
      sw_cigar_string(cigar + a->cigar_offset, a->cigar_len, text, sizeof(text));
      printf("A %zu %u %d %u %u %u %u %u %u %u %s\n", k, r, a->score, a->flags, a->q_start, a->q_end,
             a->t_start, a->t_end, a->n_columns, a->n_identities, a->cigar_len ? text : "*");
    }
  }
  CHECK(used == ops, "cigar_used counts the ops");
  /* coordinates only */
  CHECK(sw_align_disjoint_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, rounds,
                                     min_score, NULL, n, NULL, n, bare, NULL, 0, NULL) == SW_OK,
        "cigar may be NULL");
  for (size_t x = 0; x < n * rounds; ++x) {
    CHECK(bare[x].score == out[x].score && bare[x].t_start == out[x].t_start &&
              bare[x].t_end == out[x].t_end && bare[x].q_start == out[x].q_start &&
              bare[x].q_end == out[x].q_end,
          "... and the coordinates are the same");
    CHECK(bare[x].cigar_len == 0 &&
              bare[x].flags == ((out[x].flags & SW_ALIGN_EMPTY) ? out[x].flags
                                                                : out[x].flags | SW_ALIGN_NO_PATH),
          "... without a path");
  }
  sw_bank_destroy(bank);
  printf("align ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "host") == 0) return host_checks();
  if (argc >= 6 && strcmp(argv[1], "align") == 0)
    return align((uint32_t)strtoul(argv[2], NULL, 10), (int32_t)strtol(argv[3], NULL, 10), argc - 5,
                 argv[4], argv + 5);
  fprintf(stderr, "usage: %s host | align ROUNDS MIN Q T0 [T1 ...]\n", argv[0]);
  return 2;
}
