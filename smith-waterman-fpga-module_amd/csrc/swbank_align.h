/* swbank_align.h — the launch interface of the alignment kernels (swbank_kalign.hip), shared
 * with the host unit that drives them (swbank_align.hip).  Internal. */
#ifndef SWBANK_ALIGN_H
#define SWBANK_ALIGN_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

/* One call's arguments: the batch, the hit list (hits == NULL: hit h is target h), the query's
 * codes and the alpha x alpha matrix on the device, the records and the CIGAR buffer (cigar_stride
 * 0: coordinates only), per-wave scratch rows (waves x 2 x scols x 8 B; scols >= every length).
 * set != 0 (sw_align_set_hits*): hit h aligns query hit_queries[h], or h / hits_per_query, of
 * the nq queries whose codes lie at query + qtab[i].x, qtab[i].y of them; a hit whose query is
 * >= nq or whose target is >= n names no pair (SW_ALIGN_NO_HIT).  qlen is the longest query. */
typedef struct SwkAlign {
  int gotoh;
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint64_t* ids;
  const uint64_t* hits;
  size_t n_hits;
  const uint8_t* query;
  uint32_t qlen;
  const int8_t* mat;
  uint32_t alpha, pad;
  int32_t padscore;
  uint32_t O, E;
  void* out; /* sw_alignment[n_hits] */
  uint32_t* cigar;
  uint32_t cigar_stride;
  void* scratch;
  uint32_t scols;
  size_t waves; /* a multiple of 4 */
  int set;
  size_t n;                    /* targets in the batch (set) */
  const uint2* qtab;           /* {offset, length} per query (set) */
  uint32_t nq;
  const uint32_t* hit_queries; /* or NULL: hits_per_query >= 1 */
  uint32_t hits_per_query;
  /* the strand call (set != 0): hit h (query i, target t) is aligned against the reverse
   * complement of its target when strands[i * n + t], or strands[h] with strand_by_hit, is not 0;
   * NULL: every hit is on the forward strand and the set kernels run */
  const uint8_t* strands;
  int strand_by_hit;
} SwkAlign;

/* Where one hit's window sits in the direction store (dwords) and its ops in the CIGAR buffer. */
typedef struct SwkAlignPlan {
  uint64_t dir_off, dir_cap, cig_off;
  uint32_t cig_cap, reserved;
} SwkAlignPlan;

#ifdef __cplusplus
extern "C" {
#endif
/* Dwords of direction store a window of rows x cols cells takes:
 * ceil(rows / 256) strips x (cols + 63) steps x 64 lanes. */
uint64_t swk_align_dir_dwords(uint32_t rows, uint32_t cols);
hipError_t swk_launch_align_ends(const SwkAlign* p, hipStream_t st);
hipError_t swk_launch_align_paths(const SwkAlign* p, const uint32_t* list, size_t h0, size_t count,
                                  const SwkAlignPlan* plan, uint64_t slot, uint32_t* dirs,
                                  hipStream_t st);
/* After the paths of a strand call: SW_ALIGN_REVERSE and forward target coordinates. */
hipError_t swk_launch_align_flip(const SwkAlign* p, hipStream_t st);

/* Alignments of frameshift hits (swbank_kfsalign.hip): one call's arguments.  The
 * batch holds DNA; hit h is query hit_queries[h], or h / hits_per_query, of the nq queries of
 * qtab (at most qlen <= 1024 rows each) against target hits[h], or h, of n; a hit whose query is
 * >= nq or whose target is >= n names no pair.  table: 64 protein codes; o = open + extend, e,
 * fs <= 0. */
typedef struct SwkFsAlign {
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint64_t* ids;
  const uint64_t* hits;
  size_t n_hits, n;
  uint32_t max_len; /* codes of a target past it are not read */
  const uint2* qtab;
  const int8_t* mat;
  const uint8_t* query;
  uint32_t nq, qlen, alpha;
  const uint32_t* hit_queries;
  uint32_t hits_per_query;
  uint8_t table[64];
  int32_t o, e, fs;
  void* out; /* sw_alignment[n_hits] */
  uint32_t* cigar;
  uint32_t cigar_stride;
} SwkFsAlign;

/* Dwords of direction store a window of rows x cols cells (cols codon starts) takes under the
 * rows per lane K of queries of at most qlen rows: (ceil(cols / 3) + ceil(rows / K) - 1) steps x
 * 3K bytes x 64 lanes. */
uint64_t swk_fsalign_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t cols);
/* Passes A and B for hits [0, n_hits): every record written, paths left out. */
hipError_t swk_launch_fsalign_ends(const SwkFsAlign* p, hipStream_t st);
/* Passes C and D for `count` positions, placed as swk_launch_align_paths places them. */
hipError_t swk_launch_fsalign_paths(const SwkFsAlign* p, const uint32_t* list, size_t h0,
                                    size_t count, const SwkAlignPlan* plan, uint64_t slot,
                                    uint32_t* dirs, hipStream_t st);

/* Alignments of global-local hits (swbank_kglalign.hip): one call's arguments.  The
 * batch and the pair list as for SwkFsAlign (any alphabet of at most 24 codes; both != 0: DNA
 * codes); ends: SW_ENDS_*; o = open + extend, e <= 0, inside the range rule of sw_score_glocal
 * for max_len. */
typedef struct SwkGlAlign {
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint64_t* ids;
  const uint64_t* hits;
  size_t n_hits, n;
  uint32_t max_len; /* codes of a target past it are not read */
  const uint2* qtab;
  const int8_t* mat;
  const uint8_t* query;
  uint32_t nq, qlen, alpha;
  const uint32_t* hit_queries;
  uint32_t hits_per_query;
  int32_t o, e, ends, both;
  void* out; /* sw_alignment[n_hits] */
  uint32_t* cigar;
  uint32_t cigar_stride;
} SwkGlAlign;

/* Dwords of direction store a window of rows x cols cells takes under the rows per lane K of
 * queries of at most qlen rows: (cols + ceil(rows / K) - 1) steps x K bytes x 64 lanes. */
uint64_t swk_glalign_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t cols);
/* Passes A and B for hits [0, n_hits): every record written, paths left out. */
hipError_t swk_launch_glalign_ends(const SwkGlAlign* p, hipStream_t st);
/* Passes C and D for `count` positions, placed as swk_launch_align_paths places them. */
hipError_t swk_launch_glalign_paths(const SwkGlAlign* p, const uint32_t* list, size_t h0,
                                    size_t count, const SwkAlignPlan* plan, uint64_t slot,
                                    uint32_t* dirs, hipStream_t st);

/* Non-intersecting local alignments (swbank_klalign.hip): one call's arguments.  The
 * batch and the pair list as for SwkFsAlign (any alphabet of at most 24 codes); o = open + extend,
 * e <= 0.  The record of (hit h, round r) is out[h * rounds + r].  plan == NULL: its ops go to
 * cigar + (h * rounds + r) * cigar_stride (cigar NULL or stride 0: no ops), and position k of a
 * launch keeps its direction bytes in slot k of `slot` dwords.  plan != NULL, one entry per hit:
 * the store at dirs + plan[h].dir_off (dir_cap dwords), the ops of round r at
 * cigar + plan[h].cig_off + r * plan[h].cig_cap, at most cig_cap of them. */
typedef struct SwkLaAlign {
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint64_t* ids;
  const uint64_t* hits;
  size_t n_hits, n;
  uint32_t max_len; /* codes of a target past it are not read */
  const uint2* qtab;
  const int8_t* mat;
  const uint8_t* query;
  uint32_t nq, qlen, alpha;
  const uint32_t* hit_queries;
  uint32_t hits_per_query;
  int32_t o, e, min_score;
  uint32_t rounds;
  void* out; /* sw_alignment[n_hits * rounds] */
  uint32_t* cigar;
  uint32_t cigar_stride;
  const SwkAlignPlan* plan;
  uint64_t slot;
  uint32_t* dirs;
} SwkLaAlign;

/* Dwords of direction store the whole matrix of rows x cols cells takes under the rows per lane K
 * of queries of at most qlen rows: (cols + ceil(rows / K) - 1) steps x K bytes x 64 lanes. */
uint64_t swk_lalign_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t cols);
/* Round `round` < rounds of hits [h0, h0 + count): walk, best cell, path, used cells, record.
 * Round r > 0 follows round r - 1 of the same hits on the same stream. */
hipError_t swk_launch_lalign_round(const SwkLaAlign* p, size_t h0, size_t count, uint32_t round,
                                   hipStream_t st);

/* Non-intersecting alignments over the six reading frames of a hit (swbank_klaframes.hip, DESIGN
 * 3.20): one call's arguments.  `a` as for swk_launch_lalign_round, but the batch holds DNA codes
 * and alpha is the protein matrix's; a hit's direction store (a slot, or plan[h].dir_cap dwords)
 * holds the stores of its six frames back to back, frame f's of
 * swk_lalign_dir_dwords(qlen, m, codons of frame f) dwords.  table: 64 protein codes.  state:
 * SWK_LAFRAMES_STATE dwords per position of a launch, written by round 0 and carried through the
 * rounds of those positions: {score, column, row} of each frame's best remaining cell, then the
 * frame of the last record. */
#define SWK_LAFRAMES_STATE 20
typedef struct SwkLaFrames {
  SwkLaAlign a;
  uint8_t table[64];
  int32_t* state;
} SwkLaFrames;

/* Dwords of direction store the six frames of a target of `len` codes take against `rows` rows. */
uint64_t swk_laframes_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t len);
/* Round `round` < rounds of hits [h0, h0 + count), as swk_launch_lalign_round. */
hipError_t swk_launch_laframes_round(const SwkLaFrames* p, size_t h0, size_t count, uint32_t round,
                                     hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif /* SWBANK_ALIGN_H */
