/* frame_client.c — a plain C99 client of the translated-search calls of libswbank.so, for
 * tests/test_c_frames.py.
 *
 *   frame_client host            the new constants and sw_translate_codes from C (no device),
 *                                prints "host ok"
 *   frame_client search Q T...   loads the protein query Q, scores the six frames of every DNA
 *                                target T... (ASCII) with BLOSUM62 -11/-1 through sw_score_frames
 *                                (lines "S k score frame") and aligns every target on its frame
 *                                through sw_align_frame_hits (lines "A k ..."); a record is "index
 *                                score flags q_start q_end t_start t_end columns identities cigar"
 *                                (cigar "-" when there are no ops).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swbank.h"

#if !SWBANK_HAS_FRAMES
#error "swbank.h without the translated-search calls"
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
  CHECK(SW_ALIGN_FRAME_SHIFT == 4 && SW_ALIGN_FRAME_MASK == 0x30 && SW_FRAME_COUNT == 6,
        "the frame constants");
  CHECK((SW_ALIGN_FRAME_MASK &
         (SW_ALIGN_EMPTY | SW_ALIGN_NO_PATH | SW_ALIGN_NO_HIT | SW_ALIGN_REVERSE)) == 0,
        "the frame bits are flags of their own");
  CHECK(SWBANK_ABI_VERSION == 6, "the ABI version stays 6");
  const char *dna = "ATGGCCTAANN";
  uint8_t codes[11], out[4], want[3], tab[64];
  sw_encode_ascii(SW_ALPHABET_DNA, dna, 11, codes);
  sw_encode_ascii(SW_ALPHABET_PROTEIN, "MA*", 3, want);
  CHECK(sw_translate_codes(codes, 11, 0, NULL, out) == 3 && memcmp(out, want, 3) == 0,
        "ATGGCCTAANN in frame 0 is MA*");
  /* frame 5: rc = NNTTAGGCCAT, from its third code: TTA GGC CAT = L G H */
  sw_encode_ascii(SW_ALPHABET_PROTEIN, "LGH", 3, want);
  CHECK(sw_translate_codes(codes, 11, 5, NULL, out) == 3 && memcmp(out, want, 3) == 0,
        "... in frame 5 is LGH");
  /* frame 3: NNT TAG GCC = X * A */
  sw_encode_ascii(SW_ALPHABET_PROTEIN, "X*A", 3, want);
  CHECK(sw_translate_codes(codes, 11, 3, NULL, out) == 3 && memcmp(out, want, 3) == 0,
        "... in frame 3 is X*A");
  CHECK(sw_translate_codes(codes, 2, 0, NULL, out) == 0, "no codon: an empty frame");
  CHECK(sw_translate_codes(codes, 4, 2, NULL, out) == 0, "L < f + 3: an empty frame");
  CHECK(sw_translate_codes(codes, 11, 6, NULL, out) == 0, "a frame above 5");
  CHECK(sw_translate_codes(NULL, 11, 0, NULL, out) == 0, "a NULL argument");
  memset(tab, 7, sizeof tab); /* every codon is G */
  CHECK(sw_translate_codes(codes, 11, 0, tab, out) == 3 && out[0] == 7 && out[2] == 7,
        "a caller's table");
  tab[5] = SW_PROTEIN_ALPHA;
  CHECK(sw_translate_codes(codes, 11, 0, tab, out) == 0, "a table entry of 24");
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
  sw_bank *bank = NULL, *dna = NULL;
  int32_t scores[MAXT];
  uint8_t frames[MAXT];
  static sw_alignment al[MAXT];
  static uint32_t cig[MAXOPS];
  size_t used = 0;
  /* a DNA bank refuses */
  CHECK(sw_bank_create(&dna, &cfg) == SW_OK, "DNA bank create");
  CHECK(sw_score_frames(dna, res, total, offs, lens, n, NULL, scores, frames) ==
            SW_ERR_UNSUPPORTED,
        "a DNA bank: SW_ERR_UNSUPPORTED");
  sw_bank_destroy(dna);
  cfg.alphabet = SW_ALPHABET_PROTEIN;
  cfg.gap_model = SW_GAP_GOTOH;
  CHECK(sw_bank_create(&bank, &cfg) == SW_OK, "bank create");
  CHECK(sw_score_frames(bank, res, total, offs, lens, n, NULL, scores, frames) == SW_ERR_STATE,
        "no query yet: SW_ERR_STATE");
  CHECK(sw_load_query(bank, 0, qcodes, qlen) == SW_OK, "query");
  CHECK(sw_score_frames(bank, res, total, offs, lens, n, NULL, NULL, frames) == SW_ERR_ARG,
        "no scores: SW_ERR_ARG");
  if (sw_score_frames(bank, res, total, offs, lens, n, NULL, scores, frames) != SW_OK) {
    fprintf(stderr, "FAIL sw_score_frames: %s\n", sw_last_error(bank));
    return 1;
  }
  printf("kernel %s\n", sw_last_kernel(bank));
  for (size_t k = 0; k < n; ++k) printf("S %zu %d %u\n", k, scores[k], frames[k]);
  CHECK(sw_align_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, NULL, NULL, n, NULL, n,
                            al, cig, MAXOPS, &used) == SW_ERR_ARG,
        "no frames: SW_ERR_ARG");
  /* every target on its frame: one query, the [1, n] layout, no hit list */
  if (sw_align_frame_hits(bank, res, total, offs, lens, NULL, n, NULL, frames, NULL, n, NULL, n, al,
                          cig, MAXOPS, &used) != SW_OK) {
    fprintf(stderr, "FAIL sw_align_frame_hits: %s\n", sw_last_error(bank));
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
