/*
 * swbank_host.c — host-side helpers of libswbank.so (no device needed).
 *
 * Encoding follows the reference's two encoders:
 *   ConvertToBase  ScoreBank/ScoreBank_v1_tb.sv:44-52        (A=10b G=11b T=00b C=01b)
 *   charTo2bit     capi_sample_aligner/software-C,C++/include/aligner_Header.c:14-47
 *                  (2 bits per base, LSB first, 4 bases per byte; 'N' and other bytes -> 00b)
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "swbank.h"
#include "swbank_internal.h"

int32_t sw_abi_version(void) { return SWBANK_ABI_VERSION; }

const char *sw_status_string(sw_status s) {
  switch (s) {
    case SW_OK: return "ok";
    case SW_ERR_ARG: return "invalid argument";
    case SW_ERR_NO_DEVICE: return "no usable gfx950 HIP device";
    case SW_ERR_HIP: return "HIP runtime error";
    case SW_ERR_RANGE: return "substitution or gap range outside the kernels";
    case SW_ERR_STATE: return "penalties or query not loaded";
    case SW_ERR_NOMEM: return "out of memory";
    case SW_ERR_IO: return "I/O or parse error";
    case SW_ERR_UNSUPPORTED: return "unsupported configuration";
    case SW_ERR_TIMEOUT: return "device-side hand-off wait timed out (scores invalid)";
    default: return "unknown status";
  }
}

uint32_t sw_max_query_len(void) { return SWB_MAX_QUERY; }

sw_status sw_config_default(sw_config *cfg) {
  if (!cfg) return SW_ERR_ARG;
  memset(cfg, 0, sizeof(*cfg));
  cfg->device = -1;
  cfg->alphabet = SW_ALPHABET_DNA;
  cfg->gap_model = SW_GAP_MERGED;
  cfg->max_query_len = 0;
  return SW_OK;
}

static const char kProtLetters[SW_PROTEIN_ALPHA + 1] = "ARNDCQEGHILKMFPSTWYVBZX*";

static uint8_t dna_code(unsigned char c) {
  switch (c) {
    case 'T': case 't': return SW_DNA_T;
    case 'C': case 'c': return SW_DNA_C;
    case 'A': case 'a': return SW_DNA_A;
    case 'G': case 'g': return SW_DNA_G;
    default: return SW_DNA_N;
  }
}

static uint8_t prot_code(unsigned char c) {
  if (c >= 'a' && c <= 'z') c = (unsigned char)(c - 'a' + 'A');
  for (int i = 0; i < SW_PROTEIN_ALPHA; ++i)
    if ((unsigned char)kProtLetters[i] == c) return (uint8_t)i;
  return 22; /* X */
}

size_t sw_encode_ascii(int32_t alphabet, const char *ascii, size_t n, uint8_t *codes) {
  if (!ascii || !codes) return 0;
  if (alphabet == SW_ALPHABET_PROTEIN) {
    for (size_t i = 0; i < n; ++i) codes[i] = prot_code((unsigned char)ascii[i]);
  } else {
    for (size_t i = 0; i < n; ++i) codes[i] = dna_code((unsigned char)ascii[i]);
  }
  return n;
}

size_t sw_pack_2bit(const char *ascii, size_t n, uint8_t *out) {
  if (!ascii || !out) return 0;
  for (size_t i = 0; i < n; ++i) {
    uint8_t c = dna_code((unsigned char)ascii[i]);
    if (c > 3) c = 0; /* charTo2bit: unknown bases -> 00b */
    out[i >> 2] |= (uint8_t)(c << ((i & 3) * 2));
  }
  return (n + 3) / 4;
}

size_t sw_unpack_2bit(const uint8_t *packed, size_t n, uint8_t *codes) {
  if (!packed || !codes) return 0;
  for (size_t i = 0; i < n; ++i) codes[i] = (uint8_t)((packed[i >> 2] >> ((i & 3) * 2)) & 3u);
  return n;
}

/* T <-> A (0 <-> 2), C <-> G (1 <-> 3); N and anything past it stays.  out may be codes. */
size_t sw_revcomp_codes(const uint8_t *codes, size_t n, uint8_t *out) {
  if (!codes || !out) return 0;
  for (size_t i = 0, j = n; i < j; ++i) {
    --j;
    const uint8_t a = codes[i], b = codes[j];
    out[i] = (uint8_t)(b < 4 ? b ^ 2 : b);
    out[j] = (uint8_t)(a < 4 ? a ^ 2 : a);
  }
  return n;
}

/* The genetic code a call uses, as 64 protein codes indexed c0 * 16 + c1 * 4 + c2 over the DNA
 * codes T, C, A, G: the caller's table, or for NULL the standard code.  0 (nothing usable) when
 * an entry is no protein code.  Shared with swbank_frame.hip and swbank_align.hip. */
int swbank_codon_table(const uint8_t *user, uint8_t out[64]) {
  static const char kStandard[] =
      "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
  static const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBZX*";
  for (int i = 0; i < 64; ++i) {
    if (user) {
      if (user[i] >= SW_PROTEIN_ALPHA) return 0;
      out[i] = user[i];
    } else {
      out[i] = (uint8_t)(strchr(kLetters, kStandard[i]) - kLetters);
    }
  }
  return 1;
}

size_t sw_translate_codes(const uint8_t *codes, size_t n, uint32_t frame,
                          const uint8_t *codon_table, uint8_t *out) {
  uint8_t tab[64];
  if (!codes || !out || frame >= SW_FRAME_COUNT || !swbank_codon_table(codon_table, tab)) return 0;
  const size_t o = frame % 3, nc = n >= o + 3 ? (n - o) / 3 : 0;
  for (size_t j = 0; j < nc; ++j) {
    uint8_t c[3];
    for (size_t i = 0; i < 3; ++i) {
      const size_t s = o + 3 * j + i;
      const uint8_t x = frame < 3 ? codes[s] : codes[n - 1 - s];
      c[i] = (uint8_t)(frame >= 3 && x < 4 ? x ^ 2 : x); /* the reverse frames: rc, read in place */
    }
    out[j] = (c[0] | c[1] | c[2]) < 4 ? tab[c[0] * 16 + c[1] * 4 + c[2]] : 22; /* X */
  }
  return nc;
}

/* BLOSUM62 in NCBI order ARNDCQEGHILKMFPSTWYVBZX*. */
static const int8_t kBlosum62[SW_PROTEIN_ALPHA][SW_PROTEIN_ALPHA] = {
    {4, -1, -2, -2, 0, -1, -1, 0, -2, -1, -1, -1, -1, -2, -1, 1, 0, -3, -2, 0, -2, -1, 0, -4},
    {-1, 5, 0, -2, -3, 1, 0, -2, 0, -3, -2, 2, -1, -3, -2, -1, -1, -3, -2, -3, -1, 0, -1, -4},
    {-2, 0, 6, 1, -3, 0, 0, 0, 1, -3, -3, 0, -2, -3, -2, 1, 0, -4, -2, -3, 3, 0, -1, -4},
    {-2, -2, 1, 6, -3, 0, 2, -1, -1, -3, -4, -1, -3, -3, -1, 0, -1, -4, -3, -3, 4, 1, -1, -4},
    {0, -3, -3, -3, 9, -3, -4, -3, -3, -1, -1, -3, -1, -2, -3, -1, -1, -2, -2, -1, -3, -3, -2, -4},
    {-1, 1, 0, 0, -3, 5, 2, -2, 0, -3, -2, 1, 0, -3, -1, 0, -1, -2, -1, -2, 0, 3, -1, -4},
    {-1, 0, 0, 2, -4, 2, 5, -2, 0, -3, -3, 1, -2, -3, -1, 0, -1, -3, -2, -2, 1, 4, -1, -4},
    {0, -2, 0, -1, -3, -2, -2, 6, -2, -4, -4, -2, -3, -3, -2, 0, -2, -2, -3, -3, -1, -2, -1, -4},
    {-2, 0, 1, -1, -3, 0, 0, -2, 8, -3, -3, -1, -2, -1, -2, -1, -2, -2, 2, -3, 0, 0, -1, -4},
    {-1, -3, -3, -3, -1, -3, -3, -4, -3, 4, 2, -3, 1, 0, -3, -2, -1, -3, -1, 3, -3, -3, -1, -4},
    {-1, -2, -3, -4, -1, -2, -3, -4, -3, 2, 4, -2, 2, 0, -3, -2, -1, -2, -1, 1, -4, -3, -1, -4},
    {-1, 2, 0, -1, -3, 1, 1, -2, -1, -3, -2, 5, -1, -3, -1, 0, -1, -3, -2, -2, 0, 1, -1, -4},
    {-1, -1, -2, -3, -1, 0, -2, -3, -2, 1, 2, -1, 5, 0, -2, -1, -1, -1, -1, 1, -3, -1, -1, -4},
    {-2, -3, -3, -3, -2, -3, -3, -3, -1, 0, 0, -3, 0, 6, -4, -2, -2, 1, 3, -1, -3, -3, -1, -4},
    {-1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4, 7, -1, -1, -4, -3, -2, -2, -1, -2, -4},
    {1, -1, 1, 0, -1, 0, 0, 0, -1, -2, -2, 0, -1, -2, -1, 4, 1, -3, -2, -2, 0, 0, 0, -4},
    {0, -1, 0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1, 1, 5, -2, -2, 0, -1, -1, 0, -4},
    {-3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1, 1, -4, -3, -2, 11, 2, -3, -4, -3, -2, -4},
    {-2, -2, -2, -3, -2, -1, -2, -3, 2, -1, -1, -2, -1, 3, -3, -2, -2, 2, 7, -1, -3, -2, -1, -4},
    {0, -3, -3, -3, -1, -2, -2, -3, -3, 3, 1, -2, 1, -1, -2, -2, 0, -3, -1, 4, -3, -2, -1, -4},
    {-2, -1, 3, 4, -3, 0, 1, -1, 0, -3, -4, 0, -3, -3, -2, 0, -1, -4, -3, -3, 4, 1, -1, -4},
    {-1, 0, 0, 1, -3, 3, 4, -2, 0, -3, -3, 1, -1, -3, -1, 0, -1, -3, -2, -2, 1, 4, -1, -4},
    {0, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, 0, 0, -2, -1, -1, -1, -1, -1, -4},
    {-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, 1},
};

sw_status sw_fill_matrix(int32_t alphabet, int32_t match, int32_t mismatch, int8_t *m) {
  if (!m) return SW_ERR_ARG;
  if (alphabet == SW_ALPHABET_PROTEIN) {
    memcpy(m, kBlosum62, sizeof(kBlosum62));
    return SW_OK;
  }
  if (alphabet != SW_ALPHABET_DNA) return SW_ERR_ARG;
  if (match < -128 || match > 127 || mismatch < -128 || mismatch > 127) return SW_ERR_ARG;
  for (int a = 0; a < SW_DNA_ALPHA; ++a)
    for (int b = 0; b < SW_DNA_ALPHA; ++b)
      m[a * SW_DNA_ALPHA + b] = (int8_t)((a == b && a < 4) ? match : mismatch);
  return SW_OK;
}

size_t sw_cigar_string(const uint32_t *ops, size_t n_ops, char *buf, size_t cap) {
  size_t need = 0;
  for (size_t k = 0; ops && k < n_ops; ++k) {
    char tmp[16];
    const uint32_t code = ops[k] & 15u;
    const int w = snprintf(tmp, sizeof(tmp), "%u%c", (unsigned)(ops[k] >> 4),
                           code == SW_CIGAR_M ? 'M' : code == SW_CIGAR_I ? 'I'
                           : code == SW_CIGAR_D ? 'D' : code == SW_CIGAR_FS_SKIP ? '/'
                           : code == SW_CIGAR_FS_BACK ? '\\' : '?');
    for (int c = 0; c < w; ++c, ++need)
      if (buf && need + 1 < cap) buf[need] = tmp[c];
  }
  if (buf && cap) buf[need < cap ? need : cap - 1] = 0;
  return need;
}

/* ---- hit statistics (swbank.h "hit significance") --------------------------------------- */
/* f(lambda) of the likelihood equations over the occupied bins [lo, hi], the exponent shifted
 * by lo so nothing underflows; *sum receives sum A_s e^(-lambda (s - lo)). */
static double stat_f(const uint64_t *counts, const uint64_t *len_sums, double m, int lo, int hi,
                     double mean, double lambda, double *sum) {
  double sa = 0.0, ssa = 0.0;
  for (int s = lo; s <= hi; ++s) {
    if (!counts[s]) continue;
    const double w = m * (double)len_sums[s] * exp(-lambda * (double)(s - lo));
    sa += w;
    ssa += (double)s * w;
  }
  *sum = sa;
  return 1.0 / lambda - mean + ssa / sa;
}

sw_status sw_fit_statistics(const uint64_t *counts, const uint64_t *len_sums, uint32_t query_len,
                            sw_statistics *out) {
  if (!counts || !len_sums || !out) return SW_ERR_ARG;
  memset(out, 0, sizeof(*out));
  out->query_len = query_len;
  int lo = -1, hi = -1, bins = 0;
  uint64_t N = 0;
  double ssum = 0.0, wsum = 0.0;
  for (int s = 0; s < SW_STAT_BINS; ++s) {
    if (!counts[s]) continue;
    if (lo < 0) lo = s;
    hi = s;
    ++bins;
    N += counts[s];
    ssum += (double)s * (double)counts[s];
    wsum += (double)len_sums[s];
  }
  out->n_samples = N;
  if (bins) {
    out->min_score = lo;
    out->max_score = hi;
  }
  /* (an occupied lowest bin without lengths has no weight: f need not change sign then) */
  if (bins < 2 || query_len == 0 || wsum == 0.0 || len_sums[lo] == 0) {
    out->flags = SW_STAT_DEGENERATE;
    return SW_OK;
  }
  const double m = (double)query_len, mean = ssum / (double)N;
  /* f is strictly decreasing from +inf to lo - mean < 0: bracket the root, then bisect */
  double b = 1.0, sum;
  while (b < 0x1p64 && stat_f(counts, len_sums, m, lo, hi, mean, b, &sum) > 0.0) b *= 2.0;
  double a = 0.5 * b;
  while (a > 0x1p-1000 && stat_f(counts, len_sums, m, lo, hi, mean, a, &sum) < 0.0) a *= 0.5;
  if (b >= 0x1p64 || a <= 0x1p-1000) { /* no sign change found */
    out->flags = SW_STAT_DEGENERATE;
    return SW_OK;
  }
  for (int it = 0; it < 200 && b - a > 1e-13 * a; ++it) {
    const double mid = 0.5 * (a + b);
    if (stat_f(counts, len_sums, m, lo, hi, mean, mid, &sum) > 0.0) a = mid;
    else b = mid;
  }
  const double lambda = 0.5 * (a + b);
  (void)stat_f(counts, len_sums, m, lo, hi, mean, lambda, &sum);
  out->lambda = lambda;
  out->K = (double)N * exp(lambda * (double)lo) / sum;
  return SW_OK;
}

sw_status sw_hit_significance(const sw_statistics *st, const int32_t *scores,
                              const uint32_t *target_lens, size_t n_hits, uint64_t db_size,
                              double *bits, double *evalues) {
  if (!st || !scores || !target_lens || (!bits && !evalues)) return SW_ERR_ARG;
  if ((st->flags & SW_STAT_DEGENERATE) || !(st->lambda > 0.0) || !(st->K > 0.0)) return SW_ERR_ARG;
  const double ln_k = log(st->K);
  for (size_t h = 0; h < n_hits; ++h) {
    const double ls = st->lambda * (double)scores[h];
    if (bits) bits[h] = (ls - ln_k) / 0.693147180559945309417232121458;
    if (evalues)
      evalues[h] = (double)db_size * st->K * (double)st->query_len * (double)target_lens[h] *
                   exp(-ls);
  }
  return SW_OK;
}
