/*
 * swbank — command-line host for libswbank.so.
 *
 * Mirrors the reference's two hosts:
 *   - the CAPI sample host's flags  -q query -l library  (capi_sample_aligner/software-C,C++/
 *     src/main_test.c:231-279), without the libcxl/AFU plumbing;
 *   - the ScoreBank testbench's transcript lines ">name score: S" (ScoreBank/ScoreBank_v1_tb.sv:
 *     271-285), one per library record, in library order (the RTL printed completion order).
 *
 * Usage: swbank -q query.fa -l library.fa [-p match,mismatch,open,extend] [-P] [-g]
 *               [-d device[,device...]] [-o out.txt] [-T] [-R scores.txt] [-b] [-A k]
 *               [-E rounds[,seed]] [-S lambda,K] [-B] [-X [-F frameshift]] [-G q|t|b]
 *               [-N rounds[,min]]
 *   -p  penalties (default 5,-4,-12,-4: ScoreBank_v1_tb.sv:16-19, data/smith-waterman.py:6-10)
 *   -P  protein mode (BLOSUM62; -p gives only open,extend)      -g  Gotoh gap model
 *   -T  testbench transcript format "@     0ns: %10s score: \t%d"
 *   -R  also write an ssearch36 "-R" score file (data/score500.txt layout: one line per
 *       library record with name, length, score, record index and byte offset)
 *   -d  HIP device, or a comma list for a multi-device bank (the library is dealt over the
 *       devices, length-balanced, and the scores gathered back with RCCL; ScoreBank_v2.v:76-148
 *       spreads targets over MODULES the same way)
 *   -A  after the score lines, the alignments of the k best library records (score descending,
 *       ties in library order, chosen on the host from the scores; sw_align_hits), each as
 *       ssearch36 reports a hit (data/alignments500.txt): ">>name (len nt)", " s-w opt: S", the
 *       summary line "Smith-Waterman score: S; P% identity (P% similar) in N nt overlap
 *       (qs-qe:ts-te)" with 1-based coordinates ("aa" with -P), then "cigar: ..." (a record
 *       scoring 0 prints the first two lines only)
 *   -E  estimate lambda and K from `rounds` seeded shuffles of the library (seed 0 unless
 *       given; sw_estimate_statistics, ≙ ssearch36's "Statistics: (shuffled [500]) MLE
 *       statistics" line, data/alignments500.txt:13)      -S  take lambda and K as given
 *       Either prints "Statistics: Lambda= L;  K=K (n samples)" after the score lines and extends
 *       every hit's " s-w opt: S" line of -A to " s-w opt: S  bits: B E(n): E" with n = the
 *       library's record count (data/alignments500.txt:24); without them nothing changes
 *   -B  search both DNA strands (sw_score_strands; what ssearch36 does without its -3 switch,
 *       which the reference's runs set, data/alignments500.txt:1): every score is the better of
 *       the forward score and the score against the record's reverse complement, and " [f]" or
 *       " [r]" (the reverse score strictly greater) follows it on every score line.  -A aligns
 *       each hit on its strand (sw_align_strand_hits), prints the strand after ">>name (len nt)"
 *       and, for [r], the overlap's target range high to low on the forward record: the
 *       alignment runs down it.  With -E / -S the E-values take db_size = 2 x the record count
 *       (two strands are a library twice the size; the reference, run with -3, pins no such
 *       convention), printed as E(2n); -E still fits lambda and K on forward shuffles.  The -R
 *       file keeps its layout (scores only).  Not with -P.
 *   -X  translated search (sw_score_frames; the FASTA suite's tfastx without frameshifts): -q is
 *       a protein, -l a DNA library; every record is translated in its three forward and three
 *       reverse reading frames, each frame is scored with BLOSUM62 (-X implies -P's matrix and
 *       its -11,-1 default; -p gives open,extend), and the best frame's score is printed with
 *       " [+1]", " [+2]", " [+3]", " [-1]", " [-2]" or " [-3]" after it (a tie: the first of
 *       these).  -A aligns each hit on its frame (sw_align_frame_hits), prints the frame after
 *       ">>name (len nt)" and the overlap in aa columns with the record's 1-based nucleotide
 *       range, high to low for a reverse frame.  With -E / -S the E-values take db_size = 6 x
 *       the record count and the frame's length in codons, printed as E(6n); -E fits lambda and K
 *       on shuffles of the library's six translations (made here with sw_translate_codes and
 *       handed to sw_estimate_statistics as the protein batch they are).  Not with -B (the
 *       reverse frames are already searched).
 *   -F  with -X: the frameshift-tolerant search (sw_score_fshift; this library's own definition,
 *       include/swbank.h): the three frames of a strand are scored in one matrix whose cells may
 *       step to another frame (one base re-read or skipped) at the price `frameshift`, 0 to
 *       -32767, so a hit is followed across a single-base insertion or deletion.  Every score is
 *       the better strand's and " [f]" or " [r]" (the reverse strand strictly better) follows
 *       it, as with -B.  The call knows the Gotoh gap model only, so -F implies -g.  Alignments
 *       and statistics of shifted hits do not exist yet: not with -A, -E or -S; and not with -B
 *       (both strands are searched already).
 *   -G  q, t or b: the global-local search (sw_score_glocal; this library's own definition,
 *       include/swbank.h): the query end to end against a piece of each record (q, what the FASTA
 *       suite's glsearch36 scores), each record end to end against a piece of the query (t), or
 *       both end to end (b, ggsearch36).  No floor: scores may be negative.  The call knows the
 *       Gotoh gap model only, so -G implies -g.  With -B both strands are searched and " [f]" or
 *       " [r]" follows every score, as above.  Alignments and statistics of global-local hits do
 *       not exist yet: not with -A, -E or -S; and not with -X or -F (the translated searches are
 *       local).
 *   -N  with -A: up to `rounds` (1 to 64) non-intersecting alignments per reported hit
 *       (sw_align_disjoint_hits; what the FASTA suite's lalign36 reports): the best local
 *       alignment, then the best one that shares no matrix cell with it, and so on, while they
 *       score at least `min` (default 1).  The hit's own lines are round 0 of that call (the score
 *       and the end of -A; the path by that call's own rule); every further alignment follows as
 *       "#r " and the summary line, then its "cigar: ..." line, r counting from 2.  The call knows
 *       the Gotoh gap model only, so -N implies -g.  One strand, no translation: not with -B, -X,
 *       -F or -G.
 *   -b  also print the bank's best hit ("best: >name score: S", ≙ max / vld_max) to stderr
 * FASTA: '>' starts a record (name = first token); sequence lines are concatenated; CR/LF,
 * blank lines and lower case are accepted; bytes outside the alphabet encode to N (DNA) or X
 * (protein), which score as mismatches (the testbench left them undefined, the CAPI host
 * mapped them to T: unpinned by any fixture).
 * Exit status: 0 ok, 1 usage, 2 I/O, 3 library/device error.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "swbank.h"

typedef struct {
  char **names;
  char **seqs;
  long *offs; /* byte offset of each record's '>' line */
  size_t n, cap;
} fasta_t;

static int fasta_push(fasta_t *f, char *name, long off) {
  if (f->n == f->cap) {
    size_t nc = f->cap ? 2 * f->cap : 64;
    char **nn = realloc(f->names, nc * sizeof(char *));
    if (nn) f->names = nn;
    char **ns = realloc(f->seqs, nc * sizeof(char *));
    if (ns) f->seqs = ns;
    long *no = realloc(f->offs, nc * sizeof(long));
    if (no) f->offs = no;
    if (!nn || !ns || !no) return -1;
    f->cap = nc;
  }
  f->offs[f->n] = off;
  f->names[f->n] = name;
  f->seqs[f->n] = calloc(1, 1);
  if (!f->seqs[f->n]) return -1;
  f->n++;
  return 0;
}

/* '>' starts a record (name = first token); sequence lines are concatenated (the testbench
 * read exactly one token per record, ScoreBank_v1_tb.sv:185-212; multi-line is a superset). */
static int read_fasta(const char *path, fasta_t *f) {
  FILE *fp = fopen(path, "r");
  if (!fp) return -1;
  char *line = NULL;
  size_t cap = 0;
  ssize_t len;
  long pos = 0, here;
  while ((here = pos, len = getline(&line, &cap, fp)) >= 0) {
    pos += (long)len;
    while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r' || line[len - 1] == ' '))
      line[--len] = 0;
    if (len == 0) continue;
    if (line[0] == '>') {
      char *p = line + 1;
      size_t k = strcspn(p, " \t");
      char *name = strndup(p, k);
      if (!name || fasta_push(f, name, here)) goto fail;
    } else {
      if (f->n == 0) { /* bare sequence file (the CAPI host's build/query) */
        char *name = strdup("seq");
        if (!name || fasta_push(f, name, here)) goto fail;
      }
      char **s = &f->seqs[f->n - 1];
      size_t old = strlen(*s);
      char *ns = realloc(*s, old + (size_t)len + 1);
      if (!ns) goto fail;
      memcpy(ns + old, line, (size_t)len + 1);
      *s = ns;
    }
  }
  free(line);
  fclose(fp);
  return 0;
fail:
  free(line);
  fclose(fp);
  return -1;
}

static void usage(const char *argv0) {
  fprintf(stderr,
          "usage: %s -q query.fa -l library.fa [-p match,mismatch,open,extend] [-P] [-g]\n"
          "          [-d device[,device...]] [-o out.txt] [-T] [-R scores.txt] [-b] [-A k]\n"
          "          [-E rounds[,seed]] [-S lambda,K] [-B] [-X [-F frameshift]] [-G q|t|b]\n"
          "          [-N rounds[,min]]\n"
          "  -X: protein query against a DNA library in six reading frames; not with -B\n"
          "  -F: with -X, follow hits across frameshifts at this penalty (0 .. -32767; implies -g);\n"
          "      not with -A, -E, -S or -B\n"
          "  -G: global-local search, end to end in the query (q), the record (t) or both (b);\n"
          "      implies -g; not with -A, -E, -S, -X or -F\n"
          "  -N: with -A, up to `rounds` (1 .. 64) non-intersecting alignments per hit that score at\n"
          "      least `min` (default 1); implies -g; not with -B, -X, -F or -G\n",
          argv0);
}

/* The k best records (score descending, ties in library order), aligned and printed: picked on
 * the device by sw_top_hits, or, for k past SW_TOP_MAX_K, by a sort of the whole library here. */
static const int32_t *g_sort_scores;
static int by_score(const void *a, const void *b) {
  const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
  if (g_sort_scores[x] != g_sort_scores[y]) return g_sort_scores[x] > g_sort_scores[y] ? -1 : 1;
  return x < y ? -1 : x > y;
}

static const char *const kFrameTag[SW_FRAME_COUNT] = {" [+1]", " [+2]", " [+3]",
                                                      " [-1]", " [-2]", " [-3]"};

/* The summary line and the CIGAR of a record that is not empty. */
static void print_overlap(FILE *out, const sw_alignment *a, const uint32_t *cig, const char *unit) {
  const int rev = (a->flags & SW_ALIGN_REVERSE) != 0;
  /* the target range of a reverse hit runs high to low on the forward record */
  const uint32_t t_from = rev ? a->t_end + 1 : a->t_start + 1;
  const uint32_t t_to = rev ? a->t_start + 1 : a->t_end + 1;
  if ((a->flags & ~(uint32_t)(SW_ALIGN_REVERSE | SW_ALIGN_FRAME_MASK)) == 0) {
    const double pct = 100.0 * a->n_identities / a->n_columns;
    fprintf(out,
            "Smith-Waterman score: %d; %.1f%% identity (%.1f%% similar) in %u %s overlap "
            "(%u-%u:%u-%u)\n",
            a->score, pct, pct, a->n_columns, unit, a->q_start + 1, a->q_end + 1, t_from, t_to);
    const size_t need = sw_cigar_string(cig + a->cigar_offset, a->cigar_len, NULL, 0);
    char *text = malloc(need + 1);
    if (text) {
      sw_cigar_string(cig + a->cigar_offset, a->cigar_len, text, need + 1);
      fprintf(out, "cigar: %s\n", text);
      free(text);
    }
  } else { /* coordinates without a path (a window past SWBANK_ALIGN_MB) */
    fprintf(out, "Smith-Waterman score: %d; no path (%u-%u:%u-%u)\ncigar: *\n", a->score,
            a->q_start + 1, a->q_end + 1, t_from, t_to);
  }
}

static int print_alignments(FILE *out, sw_bank *bank, const uint8_t *res, size_t total,
                            const uint64_t *offs, const uint32_t *lens, const int32_t *scores,
                            const fasta_t *lib, size_t asked, const char *unit,
                            const sw_statistics *stats, const uint8_t *strands,
                            const uint8_t *frames, uint32_t rounds, int32_t min_score) {
  const size_t k = asked < lib->n ? asked : lib->n;
  const int on_device = asked <= SW_TOP_MAX_K; /* (what -A asked for picks the path) */
  uint64_t *order = malloc((on_device ? k : lib->n) * sizeof(uint64_t));
  const size_t per = rounds ? rounds : 1; /* records per hit (-N: its rounds) */
  sw_alignment *al = malloc(k * per * sizeof(sw_alignment));
  size_t cap = k * per, used = 0;
  if (!order || !al) {
    free(order);
    free(al);
    return 3;
  }
  sw_status st = SW_OK;
  if (on_device) { /* k <= lib->n and no threshold: every slot is a hit */
    st = sw_top_hits(bank, scores, NULL, lib->n, 1, k, INT32_MIN, order, NULL, NULL, NULL);
  } else {
    for (size_t i = 0; i < lib->n; ++i) order[i] = i;
    g_sort_scores = scores;
    qsort(order, lib->n, sizeof(uint64_t), by_score);
  }
  uint32_t *cig = NULL;
  if (st == SW_OK) {
    for (size_t i = 0; i < k; ++i) cap += per * 2 * (size_t)lens[order[i]]; /* ops a path can have */
    cig = malloc(cap * sizeof(uint32_t));
    if (!cig)
      st = SW_ERR_NOMEM;
    else if (rounds) /* -N: one query, the [1, k] layout, `rounds` records per hit */
      st = sw_align_disjoint_hits(bank, res, total, offs, lens, NULL, lib->n, rounds, min_score,
                                  NULL, k, order, k, al, cig, cap, &used);
    else if (frames) /* -X: one query, the [1, k] layout */
      st = sw_align_frame_hits(bank, res, total, offs, lens, NULL, lib->n, NULL, frames, NULL, k,
                               order, k, al, cig, cap, &used);
    else if (strands) /* -B: one query, the [1, k] layout */
      st = sw_align_strand_hits(bank, res, total, offs, lens, NULL, lib->n, strands, NULL, k, order,
                                k, al, cig, cap, &used);
    else
      st = sw_align_hits(bank, res, total, offs, lens, NULL, lib->n, order, k, al, cig, cap, &used);
  }
  if (st != SW_OK) {
    fprintf(stderr, "swbank: %s: %s\n", sw_status_string(st), sw_last_error(bank));
  } else {
    for (size_t i = 0; i < k; ++i) {
      const sw_alignment *a = &al[i * per];
      const int rev = (a->flags & SW_ALIGN_REVERSE) != 0;
      /* two strands: twice the library; six frames: six times */
      const size_t db = frames ? SW_FRAME_COUNT * lib->n : strands ? 2 * lib->n : lib->n;
      const uint32_t fo = (a->flags & SW_ALIGN_FRAME_MASK) >> SW_ALIGN_FRAME_SHIFT;
      /* the length the statistics see: the record's, or (-X) its frame's in codons */
      const uint32_t slen = frames ? (lens[a->index] - fo) / 3 : lens[a->index];
      fprintf(out, ">>%s (%u %s)%s\n s-w opt: %d", lib->names[a->index], lens[a->index],
              frames ? "nt" : unit,
              frames ? kFrameTag[fo + (rev ? 3 : 0)] : strands ? (rev ? " [r]" : " [f]") : "",
              a->score);
      double bits, ev;
      if (stats && sw_hit_significance(stats, &a->score, &slen, 1, db, &bits, &ev) == SW_OK)
        fprintf(out, "  bits: %.1f E(%zu): %.2g", bits, db, ev);
      fputc('\n', out);
      if (a->flags & SW_ALIGN_EMPTY) continue;
      print_overlap(out, a, cig, unit);
      for (size_t r = 1; r < per && !(a[r].flags & SW_ALIGN_EMPTY); ++r) { /* -N: the next best */
        fprintf(out, "#%zu ", r + 1);
        print_overlap(out, a + r, cig, unit);
      }
    }
  }
  free(order);
  free(al);
  free(cig);
  return st == SW_OK ? 0 : 3;
}

int main(int argc, char **argv) {
  const char *qpath = NULL, *lpath = NULL, *opath = NULL, *pen = NULL, *rpath = NULL;
  int protein = 0, gotoh = 0, device = -1, transcript = 0, best = 0, both = 0, xlate = 0, opt;
  int ndev = 0, devs[SW_MAX_DEVICES], fshift = 0, glocal = 0;
  long nalign = 0, fs = 0, nrounds = 0, nmin = 1;
  int have_stats = 0; /* 1: -S (given), 2: -E (estimated) */
  unsigned long stat_rounds = 0;
  unsigned long long stat_seed = 0;
  sw_statistics stats;
  memset(&stats, 0, sizeof(stats));
  while ((opt = getopt(argc, argv, "q:l:p:Pgd:o:TR:bA:E:S:BXF:G:N:h")) != -1) {
    switch (opt) {
      case 'q': qpath = optarg; break;
      case 'l': lpath = optarg; break;
      case 'p': pen = optarg; break;
      case 'P': protein = 1; break;
      case 'g': gotoh = 1; break;
      case 'd': {
        char *p = optarg, *end;
        ndev = 0;
        while (*p && ndev < SW_MAX_DEVICES) {
          devs[ndev++] = (int)strtol(p, &end, 10);
          if (end == p || (*end && *end != ',')) return usage(argv[0]), 1;
          p = *end ? end + 1 : end;
        }
        /* an empty list, or more devices than a bank holds */
        if (ndev == 0 || *p) return usage(argv[0]), 1;
        device = devs[0];
        break;
      }
      case 'b': best = 1; break;
      case 'B': both = 1; break;
      case 'X': xlate = protein = 1; break;
      case 'F': {
        char *end;
        fs = strtol(optarg, &end, 10);
        if (end == optarg || *end || fs > 0 || fs < -32767) {
          fprintf(stderr, "-F takes a frameshift penalty of 0 to -32767\n");
          return usage(argv[0]), 1;
        }
        fshift = gotoh = 1;
        break;
      }
      case 'G':
        glocal = !strcmp(optarg, "q")   ? SW_ENDS_QUERY
                 : !strcmp(optarg, "t") ? SW_ENDS_TARGET
                 : !strcmp(optarg, "b") ? SW_ENDS_BOTH
                                        : 0;
        if (!glocal) {
          fprintf(stderr, "-G takes q (query end to end), t (record end to end) or b (both)\n");
          return usage(argv[0]), 1;
        }
        gotoh = 1;
        break;
      case 'N': {
        char *end;
        nrounds = strtol(optarg, &end, 10);
        if (end != optarg && *end == ',') {
          char *p = end + 1;
          nmin = strtol(p, &end, 10);
          if (end == p) nmin = 0;
        }
        if (end == optarg || *end || nrounds < 1 || nrounds > SW_DISJOINT_MAX_ROUNDS || nmin < 1 ||
            nmin > INT32_MAX) {
          fprintf(stderr, "-N takes rounds[,min]: 1 to %d alignments per hit, min at least 1\n",
                  SW_DISJOINT_MAX_ROUNDS);
          return usage(argv[0]), 1;
        }
        gotoh = 1;
        break;
      }
      case 'A': {
        char *end;
        nalign = strtol(optarg, &end, 10);
        if (end == optarg || *end || nalign < 0) return usage(argv[0]), 1;
        break;
      }
      case 'E': {
        char *end;
        stat_rounds = strtoul(optarg, &end, 10);
        if (end == optarg || stat_rounds == 0 || stat_rounds > 0xFFFFFFFFul) return usage(argv[0]), 1;
        if (*end == ',') {
          char *p = end + 1;
          stat_seed = strtoull(p, &end, 10);
          if (end == p) return usage(argv[0]), 1;
        }
        if (*end) return usage(argv[0]), 1;
        have_stats = 2;
        break;
      }
      case 'S':
        if (sscanf(optarg, "%lf,%lf", &stats.lambda, &stats.K) != 2 || !(stats.lambda > 0) ||
            !(stats.K > 0))
          return usage(argv[0]), 1;
        have_stats = 1;
        break;
      case 'o': opath = optarg; break;
      case 'T': transcript = 1; break;
      case 'R': rpath = optarg; break;
      default: usage(argv[0]); return opt == 'h' ? 0 : 1;
    }
  }
  if (!qpath || !lpath) {
    fprintf(stderr, "Input files missing\n");
    usage(argv[0]);
    return 1;
  }
  if (fshift) {
    const char *why =
        !xlate       ? "-F is the frameshift penalty of the translated search: it needs -X"
        : nalign > 0 ? "-F: alignments of shifted hits do not exist yet: not with -A"
        : have_stats ? "-F: statistics of shifted scores do not exist yet: not with -E or -S"
        : both       ? "-F searches both strands already: not with -B"
                     : NULL;
    if (why) {
      fprintf(stderr, "%s\n", why);
      usage(argv[0]);
      return 1;
    }
  }
  if (glocal) {
    const char *why =
        xlate || fshift ? "-G: the translated searches are local: not with -X or -F"
        : nalign > 0    ? "-G: alignments of global-local hits do not exist yet: not with -A"
        : have_stats    ? "-G: statistics of global-local scores do not exist yet: not with -E or -S"
                        : NULL;
    if (why) {
      fprintf(stderr, "%s\n", why);
      usage(argv[0]);
      return 1;
    }
  }
  if (nrounds) {
    const char *why =
        nalign <= 0 ? "-N lists further alignments of the hits of -A: it needs -A"
        : both || xlate || fshift || glocal
            ? "-N aligns one strand locally, untranslated: not with -B, -X, -F or -G"
            : NULL;
    if (why) {
      fprintf(stderr, "%s\n", why);
      usage(argv[0]);
      return 1;
    }
  }
  if (xlate && both) {
    fprintf(stderr, "-X searches the reverse frames already: not with -B\n");
    usage(argv[0]);
    return 1;
  }
  if (both && protein) {
    fprintf(stderr, "-B searches DNA strands: not with -P\n");
    usage(argv[0]);
    return 1;
  }
  int ma = 5, mm = -4, go = -12, ge = -4;
  if (protein) {
    go = -11;
    ge = -1;
    if (pen && sscanf(pen, "%d,%d", &go, &ge) != 2) return usage(argv[0]), 1;
  } else if (pen && sscanf(pen, "%d,%d,%d,%d", &ma, &mm, &go, &ge) != 4) {
    return usage(argv[0]), 1;
  }

  fasta_t q = {0}, lib = {0};
  if (read_fasta(qpath, &q) || q.n == 0) {
    fprintf(stderr, "Query file error!\n");
    return 2;
  }
  if (read_fasta(lpath, &lib)) {
    fprintf(stderr, "Database file error!\n");
    return 2;
  }
  const int alphabet = protein ? SW_ALPHABET_PROTEIN : SW_ALPHABET_DNA;

  sw_config cfg;
  sw_config_default(&cfg);
  cfg.device = device;
  if (ndev > 1) { /* multi-device bank */
    cfg.n_devices = ndev;
    memcpy(cfg.devices, devs, sizeof(int) * (size_t)ndev);
  }
  cfg.alphabet = alphabet;
  cfg.gap_model = gotoh ? SW_GAP_GOTOH : SW_GAP_MERGED;
  sw_bank *bank = NULL;
  sw_status st = sw_bank_create(&bank, &cfg);
  if (st != SW_OK) {
    fprintf(stderr, "swbank: bank create failed: %s\n", sw_status_string(st));
    return 3;
  }
  if (protein) {
    int8_t m[SW_PROTEIN_ALPHA * SW_PROTEIN_ALPHA];
    sw_fill_matrix(SW_ALPHABET_PROTEIN, 0, 0, m);
    st = sw_set_matrix(bank, m, SW_PROTEIN_ALPHA, go, ge);
  } else {
    st = sw_set_penalties(bank, ma, mm, go, ge);
  }
  size_t qlen = strlen(q.seqs[0]);
  uint8_t *qc = malloc(qlen + 1);
  if (st == SW_OK && qc) {
    sw_encode_ascii(alphabet, q.seqs[0], qlen, qc);
    st = sw_load_query(bank, 0, qc, (uint32_t)qlen);
  }
  size_t total = 0;
  for (size_t k = 0; k < lib.n; ++k) total += strlen(lib.seqs[k]);
  uint8_t *res = malloc(total + 1);
  uint64_t *offs = malloc((lib.n + 1) * sizeof(uint64_t));
  uint32_t *lens = malloc((lib.n + 1) * sizeof(uint32_t));
  int32_t *scores = malloc((lib.n + 1) * sizeof(int32_t));
  uint8_t *strands = both || fshift ? calloc(lib.n + 1, 1) : NULL;
  uint8_t *frames = xlate && !fshift ? calloc(lib.n + 1, 1) : NULL;
  if (!res || !offs || !lens || !scores || ((both || fshift) && !strands) ||
      (xlate && !fshift && !frames))
    st = SW_ERR_NOMEM;
  size_t pos = 0;
  for (size_t k = 0; st == SW_OK && k < lib.n; ++k) {
    size_t l = strlen(lib.seqs[k]);
    sw_encode_ascii(xlate ? SW_ALPHABET_DNA : alphabet, lib.seqs[k], l, res + pos);
    offs[k] = pos;
    lens[k] = (uint32_t)l;
    pos += l;
  }
  if (st == SW_OK)
    st = fshift ? sw_score_fshift(bank, res, total, offs, lens, lib.n, NULL, (int32_t)fs, scores,
                                  strands)
         : xlate ? sw_score_frames(bank, res, total, offs, lens, lib.n, NULL, scores, frames)
         : glocal ? sw_score_glocal(bank, res, total, offs, lens, lib.n, glocal, both, scores,
                                    NULL, strands)
         : both ? sw_score_strands(bank, res, total, offs, lens, lib.n, scores, strands)
                : sw_score_batch(bank, res, total, offs, lens, NULL, lib.n, scores);
  if (st == SW_OK && have_stats == 2 && lib.n && xlate) {
    /* the estimate shuffles the batch it is given: give it the six translations, frame-major */
    const size_t tn = SW_FRAME_COUNT * lib.n;
    uint8_t *tres = malloc(2 * total + 1);
    uint64_t *toffs = malloc(tn * sizeof(uint64_t));
    uint32_t *tlens = malloc(tn * sizeof(uint32_t));
    size_t tpos = 0;
    if (!tres || !toffs || !tlens) st = SW_ERR_NOMEM;
    for (size_t s = 0; st == SW_OK && s < tn; ++s) {
      const size_t k = s % lib.n;
      toffs[s] = tpos;
      tlens[s] = (uint32_t)sw_translate_codes(res + offs[k], lens[k], (uint32_t)(s / lib.n), NULL,
                                              tres + tpos);
      tpos += tlens[s];
    }
    if (st == SW_OK)
      st = sw_estimate_statistics(bank, tres, tpos, toffs, tlens, tn, stat_seed,
                                  (uint32_t)stat_rounds, &stats);
    free(tres);
    free(toffs);
    free(tlens);
  } else if (st == SW_OK && have_stats == 2 && lib.n) {
    st = sw_estimate_statistics(bank, res, total, offs, lens, lib.n, stat_seed,
                                (uint32_t)stat_rounds, &stats);
  }
  if (have_stats == 1) stats.query_len = (uint32_t)qlen;
  if (st != SW_OK) {
    fprintf(stderr, "swbank: %s: %s\n", sw_status_string(st), sw_last_error(bank));
    sw_bank_destroy(bank);
    return 3;
  }
  FILE *out = opath ? fopen(opath, "w") : stdout;
  if (!out) {
    sw_bank_destroy(bank);
    return 2;
  }
  for (size_t k = 0; k < lib.n; ++k) {
    char nm[256];
    snprintf(nm, sizeof(nm), ">%s", lib.names[k]);
    const char *sd = strands ? (strands[k] ? " [r]" : " [f]") /* -B, -X -F */
                     : xlate ? kFrameTag[frames[k] < SW_FRAME_COUNT ? frames[k] : 0]
                             : "";
    if (transcript)
      fprintf(out, "@%6dns: %10s score: \t%10d%s\n", 0, nm, scores[k], sd);
    else
      fprintf(out, "%s score: %d%s\n", nm, scores[k], sd);
  }
  if (have_stats)
    fprintf(out, "Statistics: Lambda= %.4f;  K=%.4f (%llu samples)\n", stats.lambda, stats.K,
            (unsigned long long)stats.n_samples);
  if (nalign > 0 && lib.n) {
    int rc = print_alignments(out, bank, res, total, offs, lens, scores, &lib, (size_t)nalign,
                              protein ? "aa" : "nt", have_stats ? &stats : NULL, strands, frames,
                              (uint32_t)nrounds, (int32_t)nmin);
    if (rc) {
      if (opath) fclose(out);
      sw_bank_destroy(bank);
      return rc;
    }
  }
  if (opath) fclose(out);
  uint64_t bid = 0;
  int32_t bsc = 0;
  /* (-B, -X and -G track no best hit on the device: the lowest index with the best merged score) */
  if (best && lib.n &&
      (both || xlate || glocal ? sw_best_hit(bank, scores, NULL, lib.n, &bid, &bsc)
                     : sw_batch_best(bank, &bid, &bsc, NULL)) == SW_OK)
    fprintf(stderr, "best: >%s score: %d%s\n", lib.names[bid], bsc,
            strands ? (strands[bid] ? " [r]" : " [f]")
            : xlate ? kFrameTag[frames[bid] < SW_FRAME_COUNT ? frames[bid] : 0]
                    : "");
  if (rpath) { /* ssearch36 -R layout (data/score500.txt:1-3,502-503) */
    FILE *rf = fopen(rpath, "w");
    if (!rf) {
      sw_bank_destroy(bank);
      return 2;
    }
    fprintf(rf, "# swbank -R %s -q %s -l %s\n", rpath, qpath, lpath);
    fprintf(rf, ">>>0 %zu\t%s - %zu %s\n", qlen, q.names[0], qlen, protein ? "aa" : "nt");
    for (size_t k = 0; k < lib.n; ++k)
      fprintf(rf,
              "%-15s %3zu 0 -1.00000 -1.00000 %4d    0    0  1  0    0    0    0  1  0 %5zu "
              "%8ld\n",
              lib.names[k], strlen(lib.seqs[k]), scores[k], k, lib.offs[k]);
    fprintf(rf, "#Algorithm : Smith-Waterman (libswbank, %s gaps, MI355X)\n",
            gotoh ? "Gotoh" : "merged");
    if (protein)
      fprintf(rf, "#Parameters : BLOSUM62 matrix, open/ext: %d/%d\n", go, ge);
    else
      fprintf(rf, "#Parameters : +%d/%d matrix (%d:%d), open/ext: %d/%d\n", ma, mm, ma, mm, go, ge);
    fprintf(rf, "#Query: %3d>>>%s - %zu %s\n", 0, q.names[0], qlen, protein ? "aa" : "nt");
    fclose(rf);
  }
  sw_bank_destroy(bank);
  free(qc);
  free(res);
  free(offs);
  free(lens);
  free(scores);
  free(strands);
  free(frames);
  return 0;
}
