/*
 * swbank.h — C ABI of the MI355X Smith-Waterman score bank (libswbank.so).
 *
 * This is the drop-in boundary for the reference's scoring path.  Each entry point
 * replaces one port group of the ScoreBank hardware (paths relative to the reference repo,
 * ilirlikalla/Smith-Waterman-FPGA-module) or one call of its C host over libcxl:
 *
 *   sw_bank_create / sw_bank_destroy
 *       ≙ instantiating ScoreBank_v2 (ScoreBank/ScoreBank_v2.v:11-44) + reset; on the CAPI
 *         host, cxl_afu_open_dev / cxl_afu_attach / cxl_afu_free
 *         (capi_sample_aligner/software-C,C++/src/main_test.c:342,370,530)
 *   sw_set_penalties
 *       ≙ ld_penalties with penalties = {match, mismatch, gap_open, gap_extend}
 *         (ScoreBank_v2.v:33-34,161; propagated to every PE, ScoringModule_v1.1.v:128-148)
 *   sw_set_matrix
 *       ≙ the PE's substitution LUT (SW_ProcessingElement_v1.0.v:119) widened to a full
 *         alphabet x alphabet matrix (protein mode; not in the reference)
 *   sw_load_query
 *       ≙ ld_sequence with the query flag, data_in = {01, ID, LEN, SEQ}
 *         (ScoreBank_v2.v:101-102,162; ScoreBank_v1_tb.sv:193-197)
 *   sw_score_batch / sw_score_batch_device
 *       ≙ streaming target records {10, ID, LEN, SEQ} (ScoreBank_v2.v:164-165,
 *         ScoreBank_v1_tb.sv:236-266) and collecting results/IDs/vld (ScoreBank_v2.v:39-41).
 *         Scores come back UNBIASED (the RTL's biased - 2048, ScoreBank_v1_tb.sv:280) and in
 *         INPUT order (the RTL reports completion order; callers re-keyed by ID).
 *   sw_best_hit
 *       ≙ the bank's max / vld_max outputs (ScoreBank_v2.v:42-43, declared but never driven).
 *   sw_top_hits / sw_top_hits_device
 *       ≙ the "The best scores are:" list ssearch36 prints over the bank's scores (the
 *         reference's data/alignments500.txt): the k best, highest score first.
 *   sw_align_hits / sw_align_set_hits (and their _device forms)
 *       ≙ the per-hit report ssearch36 prints below that list (data/alignments500.txt:
 *         score, identity, overlap coordinates and the alignment), for one query and, applied
 *         once per query, for a query set.
 *   sw_best_queries / sw_best_queries_device
 *       ≙ the same "best scores" question asked per target of a query set: which query hits
 *         this target best (the read-mapping shape, where the reads are the batch).
 *   sw_estimate_statistics / sw_hit_significance (and their _device forms)
 *       ≙ the "Statistics: (shuffled [500]) MLE statistics: Lambda= ...;  K=..." line and the
 *         "bits" and "E(499)" columns of that report (data/alignments500.txt:13,19-21,24).
 *   sw_score_strands / sw_align_strand_hits (and their _device forms)
 *       ≙ the "[f]" column of that report: the reference ran ssearch36 -3 (forward strand only,
 *         data/alignments500.txt:1); without -3 a DNA search scores both strands and prints
 *         [f] or [r] per hit.
 *   sw_encode_ascii
 *       ≙ ConvertToBase (ScoreBank_v1_tb.sv:44-52): A=2 G=3 T=0 C=1 (lower case too);
 *         any other byte -> SW_DNA_N (4), which mismatches every code.
 *   sw_pack_2bit
 *       ≙ charTo2bit (capi_sample_aligner/software-C,C++/include/aligner_Header.c:14-47):
 *         2 bits per base, base i at bits 2*(i%4) of byte i/4 (LSB first), N -> 00.
 *
 * Conventions (mirroring the reference host, main_test.c):
 *   - every call returns sw_status: 0 = SW_OK, negative = error; sw_last_error() gives text.
 *     The library never prints and never exits.
 *   - the caller owns every host buffer; the bank owns its device buffers and stream.
 *   - a bank is not thread-safe; use one bank per host thread (like one AFU context).
 *   - there is NO CPU fallback: without a usable gfx950 device sw_bank_create fails with
 *     SW_ERR_NO_DEVICE.
 */
#ifndef SWBANK_H
#define SWBANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 2: ids on the batch calls and the batch best hit (ScoreBank_v2.v:39-43), multi-device
 * banks (sw_config.n_devices / devices[]), scores past the 16-bit lanes (int32 re-score).
 * ABI 3: sw_score_batch_device_range (caller length range) and sw_bank_counters.
 * ABI 4: sw_bank_counters took the caller's struct size; multi-device banks take device
 *        batches and query sets.
 * ABI 5: SW_ERR_TIMEOUT and sw_bank_sync (device-side hand-off waits that run out fail the call,
 *        ≙ the CAPI host failing on the AFU's error bits, main_test.c:64-100); sw_bank_counters
 *        is the two-argument ABI-3 form again, sw_bank_counters_ex takes the struct size;
 *        multi-device device calls copy each device's share into its own HBM.
 * ABI 6: sw_counters.wave_balanced_timeouts; sw_score_batch_device_multi (each device scores
 *        a batch already resident in its own HBM, only the int32 scores cross xGMI); every entry
 *        point leaves the caller's current HIP device as it found it.
 * ABI 6 additions (purely additive, the version stays 6; test SWBANK_HAS_ALIGN): alignments of
 *        chosen hits -- sw_alignment, sw_align_hits, sw_align_hits_device, sw_cigar_string;
 *        (test SWBANK_HAS_TOPK) the k best hits of a score matrix -- sw_top_hits,
 *        sw_top_hits_device; (test SWBANK_HAS_ALIGN_SET) alignments against a query set --
 *        sw_align_set_hits, sw_align_set_hits_device, SW_QUERY_NONE, SW_ALIGN_NO_HIT -- and the
 *        best query of every target -- sw_best_queries, sw_best_queries_device; (test
 *        SWBANK_HAS_STATS) hit significance -- sw_shuffle_batch_device,
 *        sw_score_histogram_device, sw_fit_statistics, sw_estimate_statistics[_device],
 *        sw_hit_significance[_device], sw_statistics; (test SWBANK_HAS_STRANDS) both DNA
 *        strands -- sw_revcomp_codes, sw_revcomp_batch_device, sw_score_strands[_device],
 *        sw_align_strand_hits[_device], SW_ALIGN_REVERSE; (test SWBANK_HAS_FRAMES) the
 *        translated search -- sw_translate_codes, sw_translate_batch_device,
 *        sw_score_frames[_device], sw_align_frame_hits[_device], SW_ALIGN_FRAME_SHIFT / _MASK;
 *        (test SWBANK_HAS_FSHIFT) the frameshift-tolerant translated search --
 *        sw_score_fshift[_device], SW_FSHIFT_MAX_QUERY; (test SWBANK_HAS_FSHIFT_ALIGN) alignments
 *        of frameshift hits -- sw_align_fshift_hits[_device], SW_CIGAR_FS_SKIP / _BACK; (test
 *        SWBANK_HAS_FSHIFT_STATS) their statistics -- sw_estimate_fshift_statistics[_device];
 *        (test SWBANK_HAS_GLOCAL) the global-local search -- sw_score_glocal[_device],
 *        SW_ENDS_QUERY / _TARGET / _BOTH, SW_END_NONE, SW_GLOCAL_MAX_QUERY; (test
 *        SWBANK_HAS_GLOCAL_ALIGN) alignments of global-local hits --
 *        sw_align_glocal_hits[_device]; (test SWBANK_HAS_DISJOINT_ALIGN) the next best
 *        alignments of a pair -- sw_align_disjoint_hits[_device], SW_DISJOINT_MAX_QUERY /
 *        _MAX_ROUNDS; (test SWBANK_HAS_DISJOINT_FRAMES) the same over the six reading frames of
 *        a translated hit -- sw_align_disjoint_frame_hits[_device]. */
#define SWBANK_ABI_VERSION 6
#define SWBANK_HAS_ALIGN 1
#define SWBANK_HAS_TOPK 1
#define SWBANK_HAS_ALIGN_SET 1

typedef int32_t sw_status;
enum {
  SW_OK = 0,
  SW_ERR_ARG = -1,         /* bad argument (NULL pointer, code out of alphabet, ...)      */
  SW_ERR_NO_DEVICE = -2,   /* no HIP device / not gfx950                                 */
  SW_ERR_HIP = -3,         /* HIP runtime error (text in sw_last_error)                  */
  SW_ERR_RANGE = -4,       /* substitution span > 254 or gap penalties past the kernels  */
  SW_ERR_STATE = -5,       /* penalties or query not loaded yet                          */
  SW_ERR_NOMEM = -6,       /* host or device allocation failed                           */
  SW_ERR_IO = -7,          /* file I/O or parse error (FASTA helpers)                    */
  SW_ERR_UNSUPPORTED = -8, /* configuration not implemented (e.g. query too long)       */
  SW_ERR_TIMEOUT = -9      /* a device-side hand-off wait ran out: the scores of the call
                              (device calls: of the device calls since the last
                              synchronising call) are invalid; see sw_bank_sync            */
};

enum { SW_ALPHABET_DNA = 0, SW_ALPHABET_PROTEIN = 1 };
enum {
  SW_GAP_MERGED = 0, /* ScoreBank PE: one gap matrix I shared by both directions (default) */
  SW_GAP_GOTOH = 1   /* separate E/F matrices (ssearch36); equal to MERGED when
                        2*gap_extend <= min substitution score                           */
};
/* DNA codes (ConvertToBase). */
enum { SW_DNA_T = 0, SW_DNA_C = 1, SW_DNA_A = 2, SW_DNA_G = 3, SW_DNA_N = 4 };
#define SW_DNA_ALPHA 5
#define SW_PROTEIN_ALPHA 24 /* ARNDCQEGHILKMFPSTWYVBZX* */

#define SW_MAX_DEVICES 16

typedef struct sw_config {
  int32_t device;        /* HIP device ordinal; -1 = current device                       */
  int32_t alphabet;      /* SW_ALPHABET_*                                                 */
  int32_t gap_model;     /* SW_GAP_*                                                      */
  uint32_t max_query_len;/* 0 = library maximum (sw_max_query_len())                      */
  uint32_t flags;        /* reserved, 0                                                   */
  /* Multi-device bank (≙ MODULES scoring modules behind one PrioEncoder,
   * ScoreBank_v2.v:76-148): n_devices > 1 spreads every host batch over devices[0..n)
   * (length-balanced deal, one host thread per device) and gathers the scores on devices[0]
   * with one RCCL gather (rccl.h ncclCommInitAll + ncclGather) when the devices are distinct,
   * else with device copies.  0 or 1 = the single device `device`. */
  int32_t n_devices;
  int32_t devices[SW_MAX_DEVICES];
} sw_config;

typedef struct sw_bank sw_bank;

/* ---- library / device ---------------------------------------------------------------- */
int32_t sw_abi_version(void);
const char *sw_status_string(sw_status s);
int32_t sw_device_count(void);           /* HIP devices visible; 0 when none               */
uint32_t sw_max_query_len(void);
sw_status sw_config_default(sw_config *cfg);

/* ---- bank lifecycle (≙ ScoreBank_v2 instance) ------------------------------------------ */
sw_status sw_bank_create(sw_bank **out, const sw_config *cfg);
void sw_bank_destroy(sw_bank *bank);
const char *sw_last_error(const sw_bank *bank);

/* ---- ld_penalties / LUT ---------------------------------------------------------------- */
/* matrix[q * alpha + t] scores query code q against target code t; it need not be symmetric.
 * Accepted: 0 >= gap_open, gap_extend >= -32767 (else SW_ERR_ARG) and any int8 entries.  Two
 * combinations are refused with SW_ERR_RANGE by the first scoring or alignment call (with
 * S = max(0, largest entry), smin = smallest entry, o = -gap_open, e = -gap_extend):
 *   S - smin > 254          (the 8-bit biased tables)
 *   Gotoh and o + e + S > 65535   (the 16-bit columns; the merged model has no such limit)
 * Everything else is scored exactly (tests/test_gpu_params.py). */
sw_status sw_set_penalties(sw_bank *bank, int32_t match, int32_t mismatch, int32_t gap_open,
                           int32_t gap_extend);
sw_status sw_set_matrix(sw_bank *bank, const int8_t *matrix, int32_t alpha, int32_t gap_open,
                        int32_t gap_extend);

/* ---- ld_sequence (query) --------------------------------------------------------------- */
sw_status sw_load_query(sw_bank *bank, uint64_t id, const uint8_t *codes, uint32_t len);

/* A query set (ld_sequence for several queries; not in the reference, whose bank holds one):
 * query i = codes[offsets[i] .. + lens[i]) with id ids[i] (ids may be NULL).  Until the next
 * sw_load_query / sw_load_queries, sw_score_batch_device scores its batch against every query
 * of the set into d_scores[i * n + k] (query-major), in one launch per query segment (the
 * tile kernel streams (query, tile) units, so a workgroup scores many tiles per launch); the
 * other scoring calls return SW_ERR_STATE while a set of more than one query is loaded.
 * nq == 1 is sw_load_query.  A multi-device bank loads the set on every device (the
 * reference broadcasts its query to every module, ScoreBank_v2.v:101-102). */
sw_status sw_load_queries(sw_bank *bank, size_t nq, const uint64_t *ids, const uint8_t *codes,
                          const uint64_t *offsets, const uint32_t *lens);

/* Queries loaded (0 before any, 1 after sw_load_query). */
size_t sw_query_count(const sw_bank *bank);

/* ---- target stream -> scores ----------------------------------------------------------- */
/* Host buffers, blocking.  Target k = residues[offsets[k] .. offsets[k]+lens[k]) (codes) of
 * the residues_len-byte buffer (a target outside it is SW_ERR_ARG, nothing past it is read),
 * tagged ids[k] (the RTL's 48-bit record ID, ScoreBank_v2.v:26-28,39-41; NULL = the index k).
 * scores_out[k] = max local-alignment score of (query, target k).  The bank feeds the batch in
 * chunks through pinned staging on its own worker threads and a copy stream (gather, PCIe and
 * scoring overlap), so host buffers need no pinning or layout; n < 2^32.  The call also records
 * the batch's best hit for sw_batch_best.  A multi-device bank deals the batch over its
 * devices and gathers the scores back in input order. */
sw_status sw_score_batch(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                         const uint64_t *offsets, const uint32_t *lens, const uint64_t *ids,
                         size_t n, int32_t *scores_out);

/* Device buffers, asynchronous on `stream` (a hipStream_t; NULL = the bank's stream).
 * max_len must be >= every lens[k]; targets are visited in the caller's order unless their
 * lengths differ, then longest first (an on-device length sort).  d_scores receives int32
 * scores in input order.  With d_ids (device, may be NULL) the call also records the batch's
 * best hit on the device (sw_batch_best); without, it records nothing.  Nothing is copied to
 * or from the host.  On a multi-device bank (ABI 5) the buffers and the stream belong to the
 * root device (devices[0]): the batch is ordered longest first on the root (when its lengths
 * differ) and dealt round robin over the devices (length-balanced); each device copies its
 * share into its own HBM (DNA as 4-bit codes, ceil(max_len / 8) * 4 + 12 bytes per target over
 * xGMI, a share of more than one round of the kernel's slots in chunks that copy while the
 * previous chunk is scored; other alphabets max_len + 12 bytes), scores it there and copies
 * its int32 scores back, and the root writes them to d_scores in input order; the devices'
 * work is ordered after the caller's stream and the caller's stream after it (n < 2^32).
 * Device memory is not validated: the caller keeps every target inside d_residues
 * (d_offsets[k] + d_lens[k] <= its size) and every d_lens[k] <= max_len. */
sw_status sw_score_batch_device(sw_bank *bank, const uint8_t *d_residues,
                                const uint64_t *d_offsets, const uint32_t *d_lens,
                                const uint64_t *d_ids, size_t n, uint32_t max_len,
                                int32_t *d_scores, void *stream);

/* The same with the caller's length range: every d_lens[k] lies in [min_len, max_len].  The
 * RTL's feeder takes each target's LEN as given (SM_Feeder3.v:135-140) and feeds in arrival
 * order (ScoreBank_v2.v:142-148); when the range holds one length (a fixed-length read batch,
 * min_len == max_len) no visiting order is built on the device at all, as there.
 * sw_score_batch_device is this call with min_len = 0. */
sw_status sw_score_batch_device_range(sw_bank *bank, const uint8_t *d_residues,
                                      const uint64_t *d_offsets, const uint32_t *d_lens,
                                      const uint64_t *d_ids, size_t n, uint32_t min_len,
                                      uint32_t max_len, int32_t *d_scores, void *stream);

/* ABI 6: one batch per device, each ALREADY RESIDENT in that device's HBM (≙ every
 * ScoringModule's feeder latching its own targets before scoring them, ScoreBank_v2.v:117-137,
 * SM_Feeder3.v:104-182; BASELINE north_star: "RCCL over xGMI only to gather the final score
 * vector").  batches[d] belongs to the bank's d-th device (sw_bank_devices order; a single-device
 * bank takes one): its buffers and stream (NULL = that device's bank stream) are on that device,
 * and it is scored there against the loaded query (or query set) like
 * sw_score_batch_device_range -- no target byte crosses xGMI.  Its int32 scores go to
 * batches[d].d_scores (on device d, may be NULL; nq x n query-major for a query set) and/or are
 * gathered to the root device (devices[0]) into d_gathered (may be NULL if every d_scores is
 * given): query-major over the concatenated batch, N = sum of the n, query i, device d, target k at
 * d_gathered[i * N + (n_0 + ... + n_{d-1}) + k], written on `stream` (a root-device stream,
 * NULL = the bank's).  Distinct devices gather with one ncclGather (RCCL over xGMI: nq x max n
 * int32 per device), a device listed twice with peer copies.  Asynchronous: each device's work
 * follows its stream, `stream` follows every device's work.  No best hit is tracked (d_ids are
 * not taken); sw_bank_sync waits for it and returns a latched hand-off fault. */
typedef struct sw_device_batch {
  const uint8_t *d_residues;  /* codes on this device                                      */
  const uint64_t *d_offsets;
  const uint32_t *d_lens;
  size_t n;                   /* targets (0: the device scores nothing, still joins the gather) */
  uint32_t min_len, max_len;  /* every d_lens[k] in [min_len, max_len]                     */
  int32_t *d_scores;          /* this device's scores, or NULL                             */
  void *stream;               /* a hipStream_t of this device, or NULL                     */
} sw_device_batch;
sw_status sw_score_batch_device_multi(sw_bank *bank, const sw_device_batch *batches,
                                      size_t n_batches, int32_t *d_gathered, void *stream);

/* Best hit of the last batch call (≙ the bank's max / vld_max outputs, ScoreBank_v2.v:42-43):
 * the lowest input index with the maximum score, its id (ids[index], the record's ID for
 * sw_score_records, else the index) and score.  Waits for a device call's stream.
 * SW_ERR_STATE when the last call tracked no best hit (a device call without d_ids). */
sw_status sw_batch_best(sw_bank *bank, uint64_t *best_id, int32_t *best_score,
                        uint64_t *best_index);

/* Devices of the bank (1 for a single-device bank); writes min(count, cap) ordinals. */
int32_t sw_bank_devices(const sw_bank *bank, int32_t *devices, int32_t cap);

/* ---- CAPI record path: the reference host's packed wire format ---------
 * A record is the 64-byte `sequence_t` of capi_sample_aligner/.../aligner_Header.h:19-24:
 * { u32 ID; u16 length; u8 data[58]; } with 2-bit codes LSB-first (charTo2bit,
 * aligner_Header.c:14-47: T=0 C=1 A=2 G=3), at most 232 bases.  main_test.c:297-314 builds
 * such an array (query in record 0, targets after it) and hands it to the AFU through the
 * WED; here the query comes from sw_load_query_record and every record passed to
 * sw_score_records is a target.  DNA banks only (2 bits cannot carry N). */
#define SW_RECORD_BYTES 64
#define SW_RECORD_MAX_BASES 232
sw_status sw_load_query_record(sw_bank *bank, const void *record);
/* Host records in, unbiased scores out in input order (the kernel reads the 2-bit codes); the
 * best hit (sw_batch_best) carries the record's ID.  Multi-device banks deal the records. */
sw_status sw_score_records(sw_bank *bank, const void *records, size_t n, int32_t *scores_out);
/* Device-resident records (n x 64 B) -> device scores, asynchronous on `stream` (a
 * multi-device bank: device d copies the contiguous range [n*d/D, n*(d+1)/D) of records into
 * its own HBM and writes its scores into d_scores). */
sw_status sw_score_records_device(sw_bank *bank, const void *d_records, size_t n,
                                  int32_t *d_scores, void *stream);

/* Best hit of a host score vector (≙ max / vld_max): the lowest index with the maximum
 * score; *best_id = ids ? ids[index] : index. */
sw_status sw_best_hit(sw_bank *bank, const int32_t *scores, const uint64_t *ids, size_t n,
                      uint64_t *best_id, int32_t *best_score);
/* The same on device buffers, asynchronous on `stream`: d_out[0] = best id
 * (d_ids ? d_ids[index] : index), d_out[1] = best score (int32 sign-extended to 64 bits).
 * n <= 2^32. */
sw_status sw_best_hit_device(sw_bank *bank, const int32_t *d_scores, const uint64_t *d_ids,
                             size_t n, uint64_t *d_out, void *stream);

/* ---- the k best hits of a score matrix (ABI 6 addition) -------------------------------------
 * What connects the score calls to the alignment calls on the device: the list ssearch36 prints
 * as "The best scores are:" (the reference's data/alignments500.txt), the best hits of a query,
 * highest score first.  sw_score_batch_device, sw_top_hits_device and sw_align_hits_device run
 * back to back on one stream with no host round trip: d_hits is the align call's hit list.
 *
 * Semantics, the same for both entry points and every device layout:
 *   order     row i selects from scores[i*n .. i*n+n) the targets with score >= min_score
 *             (INT32_MIN: no threshold), ordered by score descending, then batch position
 *             ascending -- sw_batch_best's "lowest index with the maximum score", continued.
 *             The first c_i = min(k, n, number of qualifying targets) of them go to
 *             hits[i*k + j], j < c_i, as batch positions in [0, n).  This is exactly the first
 *             c_i entries of a stable descending sort of the row; the result is bitwise identical
 *             from run to run, however many targets share the k-th score.
 *   optional  hit_scores, hit_ids and counts may each be NULL.  hit_scores[i*k + j] is the hit's
 *             score, hit_ids[i*k + j] is ids ? ids[position] : position (ids holds n entries, shared
 *             by the rows), counts[i] is c_i.
 *   the rest  slots j >= c_i of every array given are written with SW_HIT_NONE / INT32_MIN /
 *             SW_HIT_NONE, so the caller's buffers are fully defined after the call.  A caller
 *             who passes no threshold and k <= n knows c_i = k without reading anything back and
 *             may pass d_hits and k straight to sw_align_hits_device.
 *   input     any int32 is a legal score, negative values, INT32_MIN and INT32_MAX included.
 * SW_ERR_ARG (nothing is written): a NULL bank, scores or hits; n, nq or k == 0;
 * k > SW_TOP_MAX_K; n > 2^32 (as sw_best_hit_device); nq * n or nq * k overflowing size_t. */
#define SW_TOP_MAX_K 4096              /* one query's selection is ordered in one workgroup's LDS:
                                          4096 64-bit keys = 32 KiB */
#define SW_HIT_NONE UINT64_MAX         /* a slot past the row's count */

/* Device buffers, asynchronous on `stream` (NULL = the bank's).
 * d_scores holds nq rows of n int32 scores, query-major, as sw_score_batch_device
 * writes them for a query set.  nq is given by the caller; the bank's loaded
 * query or query set is not consulted, so penalties and query need not be loaded.
 * A latched hand-off fault of an earlier device call is returned as by the other device calls.
 * On a multi-device bank the buffers and the stream belong to the root device (devices[0]) and
 * the work runs there, as for sw_best_hit_device.  The bank owns the scratch and orders a call
 * after the previous call's use of it, so calls on different streams need no synchronisation
 * between them; sw_bank_sync waits for the last one.  sw_last_kernel reports
 * "top k=<k> nq=<nq> n=<n>"; with sw_bank_set_timing the whole selection is bracketed as one
 * launch. */
sw_status sw_top_hits_device(sw_bank *bank, const int32_t *d_scores, const uint64_t *d_ids,
                             size_t n, size_t nq, size_t k, int32_t min_score,
                             uint64_t *d_hits, int32_t *d_hit_scores, uint64_t *d_hit_ids,
                             uint32_t *d_counts, void *stream);

/* Host buffers, blocking: uploads the scores, runs the same kernels, copies the result back.
 * hit_ids are looked up on the host, so ids are not uploaded.  Not counted in
 * sw_counters.h2d_bytes. */
sw_status sw_top_hits(sw_bank *bank, const int32_t *scores, const uint64_t *ids,
                      size_t n, size_t nq, size_t k, int32_t min_score,
                      uint64_t *hits, int32_t *hit_scores, uint64_t *hit_ids, uint32_t *counts);

/* ---- the best query per target (ABI 6 addition) ---------------------------------------------
 * The column maximum of the nq x n score matrix of a query set: for every target, which query
 * hits it best.  It is what "The best scores are:" of ssearch36 (the reference's
 * data/alignments500.txt) answers when the roles are swapped: in read mapping the references are
 * the query set and the reads are the batch, and the caller asks where each read belongs.
 * sw_score_batch_device (a set), sw_best_queries_device and sw_align_set_hits_device
 * (d_hit_queries = d_best_query, d_hits = NULL) run back to back on one stream with no host
 * round trip.
 *
 * For every target k < n: best_query[k] is the lowest i < nq whose scores[i*n + k] is the
 * column's maximum, best_score[k] that maximum; if the maximum is < min_score (INT32_MIN: no
 * threshold) they are SW_QUERY_NONE and INT32_MIN.  Either output may be NULL, not both.  Any
 * int32 is a legal score; the result is bitwise identical from run to run.
 * SW_ERR_ARG (nothing is written): a NULL bank or scores, or both outputs NULL; n or nq == 0;
 * nq > 65536 (the limit of sw_load_queries); n > 2^32; nq * n overflowing size_t. */
#define SW_QUERY_NONE UINT32_MAX       /* "no query" in a hit-query list */

/* Device buffers, asynchronous on `stream` (NULL = the bank's).  Like sw_top_hits_device it
 * consults neither the penalties nor the loaded queries, returns a latched hand-off fault of an
 * earlier device call, runs on the root device of a multi-device bank, and orders its use of
 * the bank's scratch after the previous call's, so calls on different streams need no
 * synchronisation between them.  sw_last_kernel reports "best-query nq=<nq> n=<n>"; with
 * sw_bank_set_timing the call is bracketed as one launch. */
sw_status sw_best_queries_device(sw_bank *bank, const int32_t *d_scores, size_t n, size_t nq,
                                 int32_t min_score, uint32_t *d_best_query,
                                 int32_t *d_best_score, void *stream);

/* Host buffers, blocking: uploads the scores, runs the same kernel, copies the result back.
 * Not counted in sw_counters.h2d_bytes. */
sw_status sw_best_queries(sw_bank *bank, const int32_t *scores, size_t n, size_t nq,
                          int32_t min_score, uint32_t *best_query, int32_t *best_score);

/* ---- alignments of chosen hits (ABI 6 addition) -------------------------------------------
 * The score calls return a number per pair; these return, for a caller-chosen list of hits
 * (typically the best few dozen to few thousand of a batch), where the alignment lies and the
 * alignment itself -- what ssearch36 prints per hit in the reference's data/alignments500.txt
 * ("Smith-Waterman score: 78; 66.7% identity ... in 51 nt overlap (9-55:62-110)").
 *
 * Semantics, the same for both gap models, every entry point and every device layout:
 *   score   what sw_score_batch returns for the pair (int32 arithmetic: no 16-bit bound).
 *   end     among the cells whose value is `score`: the smallest t_end, then the smallest q_end
 *           (so no other maximal cell lies in [0..q_end] x [0..t_end], which makes a reverse
 *           local pass over the reversed prefixes find the start).
 *   start   among the starts of optimal alignments ending there: the largest t_start, then the
 *           largest q_start (the same rule on the reversed problem).
 *   CIGAR   an optimal path from (q_start, t_start) to (q_end, t_end); an op is len << 4 | code,
 *           adjacent equal codes merged, the first and the last op are M; it consumes
 *           q_end - q_start + 1 query codes and t_end - t_start + 1 target codes, and re-scoring
 *           it under the bank's model gives `score`: a gap run of k columns costs
 *           open + k * extend, a run being a maximal stretch of one code under SW_GAP_GOTOH and a
 *           maximal stretch of I and D ops together under SW_GAP_MERGED (the merged gap matrix
 *           lets a gap turn the corner without re-opening).  Among co-optimal paths, walking
 *           back from the end cell: the diagonal (M) first, then a gap from the left (D), then a
 *           gap from above (I); a gap run opens rather than extends when both are optimal.
 *   empty   a pair scoring 0 (a zero-length target included): SW_ALIGN_EMPTY, every coordinate
 *           0, no ops.
 * A record with SW_ALIGN_NO_PATH has exact coordinates, no ops, and n_columns = n_identities = 0.
 *
 * Status: SW_ERR_STATE without penalties or a query, or while a query set of more than one
 * query is loaded (sw_align_set_hits below takes the set); SW_ERR_UNSUPPORTED for SW_GAP_MERGED penalties whose largest substitution
 * score exceeds open + extend (the only case in which the HDL's first-column rule,
 * SW_ProcessingElement_v1.0.v:131-141, changes a score: the reversed pass cannot apply it); a
 * latched hand-off fault of an earlier device call is returned as by the other device calls.
 * Inputs are byte codes only (no records, no packed codes). */
enum { SW_CIGAR_M = 0, SW_CIGAR_I = 1, SW_CIGAR_D = 2 };  /* BAM codes: I consumes query only,
                                                             D consumes target only          */
enum { SW_ALIGN_EMPTY = 1,    /* score 0: no alignment, all coordinates 0, no CIGAR (for
                                 sw_align_glocal_hits*: the boundary won; the score is the
                                 boundary's value and may be negative)                        */
       SW_ALIGN_NO_PATH = 2 };/* coordinates valid, CIGAR not produced (window over budget
                                 or the caller's CIGAR space too small)                      */
typedef struct sw_alignment {
  uint64_t index;             /* position of the target in the batch (the hit list's entry)  */
  uint64_t id;                /* ids[index], or index                                        */
  int32_t  score;
  uint32_t flags;
  uint32_t q_start, q_end, t_start, t_end;   /* 0-based, inclusive                           */
  uint32_t n_columns, n_identities;          /* alignment columns; columns with equal codes  */
  uint32_t cigar_offset, cigar_len;          /* ops at cigar[cigar_offset .. +cigar_len)     */
} sw_alignment;

/* Device buffers, asynchronous on `stream` (NULL = the bank's stream): aligns targets
 * d_hits[0..n_hits) (uint64 batch positions < n, any order, repeats allowed) of the batch
 * (d_residues, d_offsets, d_lens, d_ids as for sw_score_batch_device; max_len >= every
 * d_lens[k]) against the loaded query and writes d_out[h] for hit h.  Hit h's ops go to
 * d_cigar + h * cigar_stride (cigar_offset = h * cigar_stride); a path of more than cigar_stride
 * ops gets SW_ALIGN_NO_PATH.  d_cigar == NULL or cigar_stride == 0: coordinates only, every
 * non-empty hit gets SW_ALIGN_NO_PATH.  The path needs one direction byte per cell of the
 * window [q_start..q_end] x [t_start..t_end]; that memory is bounded by
 * SWBANK_ALIGN_MB (MiB, default 256) and the hits run in chunks that fit, sized here from
 * max_len x the query length so that nothing is read back; if one such window does not fit,
 * every non-empty hit gets SW_ALIGN_NO_PATH.  On a multi-device bank the buffers and the stream
 * belong to the root device (devices[0]) and the work runs there: hit lists are small.
 * sw_last_kernel reports e.g. "align i32 hits=2 chunks=1"; with sw_bank_set_timing the end /
 * start passes and the path passes are bracketed as one launch each. */
sw_status sw_align_hits_device(sw_bank *bank, const uint8_t *d_residues,
                               const uint64_t *d_offsets, const uint32_t *d_lens,
                               const uint64_t *d_ids, size_t n, uint32_t max_len,
                               const uint64_t *d_hits, size_t n_hits, sw_alignment *d_out,
                               uint32_t *d_cigar, uint32_t cigar_stride, void *stream);

/* Host buffers, blocking; the batch as for sw_score_batch (a target outside the residues, a
 * code outside the alphabet in a listed target, or a hit >= n is SW_ERR_ARG).  Only the listed
 * targets are gathered and uploaded.  The chunks are sized from the hits' actual windows (one
 * small copy of the coordinates back), so only a single window over SWBANK_ALIGN_MB gets
 * SW_ALIGN_NO_PATH.  The CIGARs are packed back to back in hit order into cigar[0..cigar_cap),
 * *cigar_used (may be NULL) = ops written; a hit whose ops no longer fit gets SW_ALIGN_NO_PATH
 * (later, shorter ones may still fit) and the call still returns SW_OK.  cigar == NULL or
 * cigar_cap == 0: coordinates only. */
sw_status sw_align_hits(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                        const uint64_t *offsets, const uint32_t *lens, const uint64_t *ids,
                        size_t n, const uint64_t *hits, size_t n_hits, sw_alignment *out,
                        uint32_t *cigar, size_t cigar_cap, size_t *cigar_used);

/* ---- alignments of chosen hits against a query set (ABI 6 addition) -------------------------
 * sw_align_hits[_device] for the pairs of a query set (sw_load_queries): ssearch36's per-hit
 * report (data/alignments500.txt) applied once per query of the set.  Apart from the pair list
 * a call behaves exactly as its single-query counterpart above: the score, the end / start /
 * CIGAR rules, the empty pair, SW_ALIGN_NO_PATH, the SWBANK_ALIGN_MB budget and its chunks, the
 * cigar_offset = h * cigar_stride layout of the device call and the packed layout of the host
 * call, SW_ERR_UNSUPPORTED for merged penalties with max(s) > open + extend, the latched
 * hand-off fault, the multi-device bank running on its root.  nq = sw_query_count(bank); a bank
 * with one loaded query is a set of one, and the call then equals sw_align_hits[_device] record
 * for record and op for op.  SW_ERR_STATE without penalties or a query.
 *
 * The pair list:
 *   query   of hit h: hit_queries[h] if hit_queries is given (hits_per_query must then be 0);
 *           else h / hits_per_query -- the nq x k layout sw_top_hits_device writes, with
 *           hits_per_query = that call's k; then hits_per_query >= 1 and
 *           n_hits <= nq * hits_per_query.  Both given, or neither: SW_ERR_ARG.
 *   target  of hit h: hits[h] if hits is given; else h itself (n_hits <= n) -- the form that
 *           follows sw_best_queries_device, whose output holds one entry per target.
 *   no pair a hit whose query is SW_QUERY_NONE or whose target is SW_HIT_NONE (the sentinel tails
 *           of sw_top_hits_device, the thresholded output of sw_best_queries_device): its record
 *           is index = id = SW_HIT_NONE, score 0, flags SW_ALIGN_EMPTY | SW_ALIGN_NO_HIT, every
 *           coordinate and count 0, cigar_len 0 (cigar_offset as for every record of the call);
 *           nothing of the batch is read for it.  Every record of the call is fully defined.
 *   record  out[h] belongs to hit h; it has no query field (the caller knows hit h's query);
 *           index and id speak of the target.
 * The device call validates nothing it would have to read back; a query index >= nq or a target
 * >= n in its lists is treated as naming no pair.  It sizes the direction-store slots from
 * max_len x the longest query of the set.  The host call returns SW_ERR_ARG for a query index
 * >= nq or a target >= n other than the sentinels, checks the batch as sw_align_hits does, and
 * sizes its chunks from the hits' actual windows.  sw_last_kernel reports
 * "align-set i32 nq=<nq> hits=<n_hits> chunks=<c>"; with sw_bank_set_timing the end / start
 * passes and the path passes are bracketed as one launch each. */
enum { SW_ALIGN_NO_HIT = 4 };  /* flag: the slot named no pair (always with SW_ALIGN_EMPTY) */

sw_status sw_align_set_hits_device(sw_bank *bank, const uint8_t *d_residues,
                                   const uint64_t *d_offsets, const uint32_t *d_lens,
                                   const uint64_t *d_ids, size_t n, uint32_t max_len,
                                   const uint32_t *d_hit_queries, size_t hits_per_query,
                                   const uint64_t *d_hits, size_t n_hits, sw_alignment *d_out,
                                   uint32_t *d_cigar, uint32_t cigar_stride, void *stream);

sw_status sw_align_set_hits(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                            const uint64_t *offsets, const uint32_t *lens, const uint64_t *ids,
                            size_t n, const uint32_t *hit_queries, size_t hits_per_query,
                            const uint64_t *hits, size_t n_hits, sw_alignment *out,
                            uint32_t *cigar, size_t cigar_cap, size_t *cigar_used);

/* ---- hit significance: shuffled-library statistics, bit scores, E-values (ABI 6 addition) ----
 * The column of ssearch36's report that says how significant a hit is (the reference's
 * data/alignments500.txt:13,19-21,24):
 *     Statistics: (shuffled [500]) MLE statistics: Lambda= 0.1840;  K=0.1293
 *     db211   ( 128) [f]   78 23.7    0.62
 *      s-w opt:  78  Z-score: 97.7  bits: 23.7 E(499): 0.62
 * ssearch36 scores the query against SHUFFLED library sequences and fits an extreme-value
 * distribution to those scores; here the shuffle, the scoring pass and the score histogram run
 * on the device over a batch that is already resident, only the histogram comes back, and the
 * fit is a few thousand exp() on the host.  The chain of a search becomes
 * score -> top hits -> significance -> align on one stream with no host step.
 *
 * The model: P(S < x) = exp(-K m n_t e^(-lambda x)) for a target of n_t codes against a query
 * of m codes (the Gumbel law with the search space as the length correction), and for a hit
 *     bits = (lambda S - ln K) / ln 2        E = db_size K m n_t e^(-lambda S)
 * (db_size: the number of library sequences searched; with the reference's Lambda, K,
 * 128 x 128 and db_size 499 these give the 23.7 / 0.62 and 22.1 / 1.9 the file prints).
 *
 * The shuffle of target k (position in the batch) under `seed`, in uint64 wrap-around
 * arithmetic -- Fisher-Yates with a counter-based draw, so the result depends on (seed, k, the
 * target's codes) alone, never on the grid, the slicing or the stream:
 *     mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *             z ^= z >> 31                      (the finaliser of splitmix64)
 *     G = 0x9E3779B97F4A7C15;  key = mix(seed + G (k + 1));  out = in;
 *     for j = L - 1 down to 1:  h = mix(key + G (j + 1));  r = ((h >> 32) (j + 1)) >> 32;
 *                               swap out[j], out[r]
 */
#define SWBANK_HAS_STATS 1
#define SW_STAT_BINS 4096              /* score bins of a histogram row: scores 0 .. 4095 */

/* Device buffers, asynchronous on `stream` (NULL = the bank's): d_out[d_offsets[k] .. +d_lens[k])
 * receives the shuffle of target k for every k < n (the batch as for sw_score_batch_device:
 * targets at any byte offset, d_lens[k] may be 0, every d_lens[k] <= max_len); no other byte of
 * d_out is written.  d_out must not overlap d_residues.  Neither penalties nor a query are
 * needed; a multi-device bank runs it on its root.  SW_ERR_ARG: a NULL bank or buffer, n == 0,
 * n >= 2^32.  sw_last_kernel reports "shuffle n=<n>". */
sw_status sw_shuffle_batch_device(sw_bank *bank, const uint8_t *d_residues,
                                  const uint64_t *d_offsets, const uint32_t *d_lens, size_t n,
                                  uint32_t max_len, uint64_t seed, uint8_t *d_out, void *stream);

/* Device buffers, asynchronous on `stream`: the score / length histogram of every row i of the
 * nq x n score matrix (query-major, rows at any multiple of 4 bytes, as for sw_top_hits_device).
 * With b = the score clamped into [0, SW_STAT_BINS - 1], every target adds 1 to
 * d_counts[i * SW_STAT_BINS + b], d_lens[k] to d_len_sums[i * SW_STAT_BINS + b], and, when the
 * clamp changed its score, 1 to d_clamped[i].  With d_lens, targets of length 0 are skipped
 * everywhere.  d_lens and d_len_sums may both be NULL (a NULL d_lens skips nothing and sums
 * nothing), d_clamped may be NULL.  The call ACCUMULATES into the caller's arrays, which the
 * caller zeroes: several shuffle rounds and slices pool their counts.  All integers are exact,
 * so the result does not depend on the order of arrival.  SW_ERR_ARG: a NULL bank, scores or
 * counts; n or nq == 0; n > 2^32; nq * n or nq * SW_STAT_BINS overflowing size_t.
 * sw_last_kernel reports "stat-hist nq=<nq> n=<n>". */
sw_status sw_score_histogram_device(sw_bank *bank, const int32_t *d_scores, const uint32_t *d_lens,
                                    size_t n, size_t nq, uint64_t *d_counts, uint64_t *d_len_sums,
                                    uint64_t *d_clamped, void *stream);

typedef struct sw_statistics {
  double lambda, K;
  uint64_t n_samples;         /* scores fitted (the non-empty targets over all rounds)      */
  uint64_t n_clamped;         /* scores outside [0, SW_STAT_BINS - 1] (sw_estimate_* only)  */
  uint32_t query_len, flags;
  int32_t min_score, max_score; /* lowest and highest occupied bin (0 when there is none)   */
} sw_statistics;
enum { SW_STAT_DEGENERATE = 1, /* fewer than two distinct scores: lambda = K = 0            */
       SW_STAT_CLAMPED = 2 };  /* a score was clamped into the histogram's range            */

/* Host, no device: the maximum-likelihood lambda and K of one histogram row (SW_STAT_BINS
 * counts and length sums, as sw_score_histogram_device writes them) for a query of query_len
 * codes.  With c_s = counts[s], A_s = query_len * len_sums[s], N = sum c_s: lambda is the root of
 *     1 / lambda - (sum s c_s) / N + (sum s A_s e^(-lambda s)) / (sum A_s e^(-lambda s))
 * (strictly decreasing, so the root is unique; bracketed, solved until the relative change of
 * lambda is <= 1e-13) and K = N / sum A_s e^(-lambda s).  Fewer than two occupied bins, N = 0 or
 * query_len = 0: lambda = K = 0 and SW_STAT_DEGENERATE, the status still SW_OK.
 * SW_ERR_ARG: a NULL argument. */
sw_status sw_fit_statistics(const uint64_t *counts, const uint64_t *len_sums, uint32_t query_len,
                            sw_statistics *out);

/* The estimate.  For every round r < rounds (rounds >= 1): the batch is shuffled with seed
 * seed + r into bank scratch, scored against the loaded query (every query of a loaded set)
 * through sw_score_batch_device_range, and the scores go into one histogram row per query;
 * after the last round the rows are copied back and fitted into out[0 .. sw_query_count()),
 * host memory.  n_samples counts the non-empty targets over all rounds, SW_STAT_CLAMPED is set
 * (and n_clamped counts) when a score left the histogram's range.  The work is enqueued on
 * `stream` (NULL = the bank's) and the call returns after synchronising it: it hands a host
 * struct back and runs once per query and library, not per batch.  The scratch (shuffled codes
 * at a stride of max_len and nq x n scores) is bounded by SWBANK_STAT_MB (MiB, default 256); a
 * batch past it runs in slices of targets, which cannot change a count, the shuffle being keyed
 * by the batch position.  A multi-device bank scores as its scoring call does, shuffle and
 * histogram on the root.  SW_ERR_STATE without penalties or a query; SW_ERR_ARG for a NULL
 * bank, buffer or out, n == 0, n >= 2^32, rounds == 0, min_len > max_len; a latched hand-off
 * fault is returned as by the other device calls.  sw_last_kernel reports
 * "stats rounds=<r> nq=<nq> n=<n> slices=<s>". */
sw_status sw_estimate_statistics_device(sw_bank *bank, const uint8_t *d_residues,
                                        const uint64_t *d_offsets, const uint32_t *d_lens,
                                        size_t n, uint32_t min_len, uint32_t max_len,
                                        uint64_t seed, uint32_t rounds, sw_statistics *out,
                                        void *stream);
/* Host buffers, blocking: the batch as for sw_score_batch (a target outside the residues is
 * SW_ERR_ARG); uploads it once and calls the device form. */
sw_status sw_estimate_statistics(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                                 const uint64_t *offsets, const uint32_t *lens, size_t n,
                                 uint64_t seed, uint32_t rounds, sw_statistics *out);

/* Host, no device: bits[h] and evalues[h] (either may be NULL, not both) of n_hits hits with
 * the given scores and target lengths.  SW_ERR_ARG: a NULL argument, both outputs NULL, or
 * degenerate statistics (SW_STAT_DEGENERATE, lambda <= 0 or K <= 0). */
sw_status sw_hit_significance(const sw_statistics *st, const int32_t *scores,
                              const uint32_t *target_lens, size_t n_hits, uint64_t db_size,
                              double *bits, double *evalues);
/* Device buffers, asynchronous on `stream`: the nq x hits_per_query layout sw_top_hits_device
 * writes -- d_hits[i * hits_per_query + j] a position into d_lens, d_hit_scores its score --
 * with row i under st[i] (host memory, nq entries, read before the call returns).  A sentinel
 * slot (SW_HIT_NONE) gets bits = -inf and E = +inf.  d_bits and d_evalues hold
 * nq x hits_per_query doubles; either may be NULL, not both.  Runs on the root of a
 * multi-device bank; calls on different streams are ordered by the bank.  SW_ERR_ARG as above,
 * for any degenerate st[i], hits_per_query or nq == 0, or an overflowing product.
 * sw_last_kernel reports "significance nq=<nq> k=<hits_per_query>". */
sw_status sw_hit_significance_device(sw_bank *bank, const sw_statistics *st,
                                     const int32_t *d_hit_scores, const uint64_t *d_hits,
                                     const uint32_t *d_lens, size_t hits_per_query, size_t nq,
                                     uint64_t db_size, double *d_bits, double *d_evalues,
                                     void *stream);

/* ---- both DNA strands (ABI 6 addition) --------------------------------------------------------
 * The "[f]" column of ssearch36's report (the reference's data/alignments500.txt:19-21,
 * "db211 ( 128) [f] 78 23.7 0.62").  The reference ran `ssearch36 -3`, which turns the reverse
 * strand off; every DNA search tool searches both strands by default, and these calls do.
 *
 * Definitions:
 *   rc        the reverse complement of a target: the codes in reverse order, each mapped
 *             T <-> A (0 <-> 2) and C <-> G (1 <-> 3), i.e. c < 4 ? c ^ 2 : c.  N stays N.
 *   reverse   the reverse-strand score of (query, target) is what the bank returns for
 *             (query, rc(target)).  That is exact by construction under every gap model and
 *             matrix the bank accepts; no reversal-symmetry argument is needed.
 *   ssearch36 searches the reverse strand as (rc(query), target).  Under SW_GAP_GOTOH, or
 *             SW_GAP_MERGED penalties without the first-column case (max(s) <= open + extend),
 *             and a complement-symmetric matrix (s(a, b) = s(comp a, comp b), as every
 *             match / mismatch matrix is), the two are the same number: an alignment of
 *             (q, rc(t)) read backwards and complemented is an alignment of (rc(q), t) with the
 *             same columns and the same gap runs (tests/test_strand_cases.py pins it on the
 *             reference's data500: 0 of 499 targets differ, both gap models).
 *   merged    score = max(forward, reverse); the strand is 1 only when the reverse score is
 *             strictly greater.  A tie is the forward strand -- "lowest index wins", as
 *             everywhere else.
 *   alphabet  DNA banks only: every call below returns SW_ERR_UNSUPPORTED on a protein bank.
 */
#define SWBANK_HAS_STRANDS 1

/* Host, no device: out[0..n) = rc(codes[0..n)); out may be codes itself (in place), any other
 * overlap is not allowed.  Returns n (0 for a NULL argument). */
size_t sw_revcomp_codes(const uint8_t *codes, size_t n, uint8_t *out);

/* Device buffers, asynchronous on `stream` (NULL = the bank's): d_out[d_offsets[k] .. +d_lens[k])
 * receives rc of target k for every k < n (the batch as for sw_score_batch_device: targets at any
 * byte offset, d_lens[k] may be 0); no other byte of d_out is written.  d_out must not overlap
 * d_residues.  Neither penalties nor a query are needed; a multi-device bank runs it on its root.
 * A library is complemented once and handed to sw_score_strands_device for every query.
 * SW_ERR_ARG: a NULL bank or buffer, n == 0, n >= 2^32.  sw_last_kernel reports
 * "revcomp n=<n>". */
sw_status sw_revcomp_batch_device(sw_bank *bank, const uint8_t *d_residues,
                                  const uint64_t *d_offsets, const uint32_t *d_lens, size_t n,
                                  uint8_t *d_out, void *stream);

/* Device buffers, asynchronous on `stream`: scores the batch on both strands against the loaded
 * query or query set.  With nq = sw_query_count(): d_scores receives the merged nq x n int32
 * scores, query-major; d_strands (may be NULL) the nq x n uint8 strands.  Each strand goes
 * through sw_score_batch_device_range exactly as a forward search does -- a single query stays
 * on the single-query kernels; kernel choice, the int32 re-score, balanced ranges and
 * multi-device dealing are unchanged -- and a merge kernel follows.
 *   d_rc given  the caller's resident reverse complement (sw_revcomp_batch_device), target k at
 *               d_rc + d_offsets[k].
 *   d_rc NULL   the bank makes it in its own scratch.  The scratch (rc codes at a stride of
 *               max_len, plus the reverse scores) is bounded by SWBANK_STRAND_MB (MiB, default
 *               256); a batch past the bound runs in slices of targets, which cannot change a
 *               result.
 * No best hit is tracked (sw_batch_best: SW_ERR_STATE).  A latched hand-off fault of an earlier
 * device call is returned as by the other device calls; sw_bank_sync waits for the merge.
 * SW_ERR_STATE without penalties or a query; SW_ERR_ARG for min_len > max_len, a NULL buffer
 * (n > 0) or n >= 2^32; n == 0 is SW_OK.  sw_last_kernel reports
 * "strands nq=<nq> n=<n> slices=<s>"; with sw_bank_set_timing the rc pass and the merge are
 * each bracketed as one launch (per slice), beside the scoring passes' own. */
sw_status sw_score_strands_device(sw_bank *bank, const uint8_t *d_residues, const uint8_t *d_rc,
                                  const uint64_t *d_offsets, const uint32_t *d_lens, size_t n,
                                  uint32_t min_len, uint32_t max_len, int32_t *d_scores,
                                  uint8_t *d_strands, void *stream);

/* Host buffers, blocking; the batch as for sw_score_batch (a target outside the residues or a
 * code outside the alphabet is SW_ERR_ARG): uploads it once and calls the device form with
 * d_rc = NULL.  scores_out: nq x n; strands_out: nq x n, may be NULL. */
sw_status sw_score_strands(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                           const uint64_t *offsets, const uint32_t *lens, size_t n,
                           int32_t *scores_out, uint8_t *strands_out);

/* sw_align_set_hits[_device] with one more argument, the nq x n strand matrix sw_score_strands
 * writes (a single loaded query is a set of one): hit h (query i, target k) is aligned against
 * rc(target k) when strands[i * n + k] != 0.  strands == NULL equals sw_align_set_hits[_device]
 * byte for byte.  No reverse complement is taken or needed: a reverse hit reads its target from
 * the far end under a column-complemented matrix.
 *
 * The record of a reverse hit: every rule above (end, start, CIGAR preference, empty pair,
 * SW_ALIGN_NO_PATH, budget, chunks) holds on the reverse-complemented target, so it is record
 * for record what sw_align_set_hits returns for a batch holding rc(target), except that
 *   flags |= SW_ALIGN_REVERSE (an empty pair too), and
 *   the target coordinates are given on the forward target, t_start = L - 1 - t_end',
 *   t_end = L - 1 - t_start' (L the target's length), so t_start <= t_end; an empty pair keeps 0.
 * Its CIGAR runs forward along the query and from t_end down to t_start along the complemented
 * target.  A slot that names no pair is never a reverse hit.  sw_last_kernel reports
 * "align-strand i32 nq=<nq> hits=<n_hits> chunks=<c>". */
enum { SW_ALIGN_REVERSE = 8 }; /* flag: aligned against the reverse complement of the target */

sw_status sw_align_strand_hits_device(sw_bank *bank, const uint8_t *d_residues,
                                      const uint64_t *d_offsets, const uint32_t *d_lens,
                                      const uint64_t *d_ids, size_t n, uint32_t max_len,
                                      const uint8_t *d_strands, const uint32_t *d_hit_queries,
                                      size_t hits_per_query, const uint64_t *d_hits,
                                      size_t n_hits, sw_alignment *d_out, uint32_t *d_cigar,
                                      uint32_t cigar_stride, void *stream);

sw_status sw_align_strand_hits(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                               const uint64_t *offsets, const uint32_t *lens, const uint64_t *ids,
                               size_t n, const uint8_t *strands, const uint32_t *hit_queries,
                               size_t hits_per_query, const uint64_t *hits, size_t n_hits,
                               sw_alignment *out, uint32_t *cigar, size_t cigar_cap,
                               size_t *cigar_used);

/* ---- translated search: a protein query against DNA in six reading frames (ABI 6 addition) ----
 * What the FASTA suite's tfastx does without frameshifts (for a search that follows a hit across
 * a frameshift see sw_score_fshift below): every DNA target is translated in its
 * three forward and three reverse reading frames, each frame is scored against the protein
 * query with the bank's matrix, and the best frame is kept.
 *
 * Definitions:
 *   codon     three adjacent DNA codes c0 c1 c2 (SW_DNA_T = 0, C = 1, A = 2, G = 3, N = 4).  All
 *             three below 4: the amino acid is table[c0 * 16 + c1 * 4 + c2] -- the T,C,A,G order
 *             of a genetic-code table, so the codes index it directly.  Any of the three at 4 or
 *             above: X (protein code 22).  The default table is the standard code,
 *             FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG, its letters as the
 *             protein codes of ARNDCQEGHILKMFPSTWYVBZX*.  A stop is * (code 23): it stays in the
 *             frame and is scored by the matrix like any residue; frames are not split at stops.
 *             codon_table: 64 protein codes in host memory, NULL for the standard code; an entry
 *             of 24 or more is SW_ERR_ARG.
 *   frame f   of a target of L codes, f in 0..5.  Frames 0..2 are the forward frames: frame f is
 *             codons j = 0 .. (L - f) / 3 - 1 over codes f + 3j .. f + 3j + 2, empty when
 *             L < f + 3.  Frames 3..5 are frames 0..2 of rc(target), rc as sw_revcomp_codes.
 *             The frame score of (query, target, f) is what the bank returns for (query, the
 *             translation of frame f): exact by construction for every matrix and gap model.
 *   merged    score = max over f; frame = the lowest f that reaches it.  A target with no codon
 *             scores 0 in frame 0.
 *   bank      protein banks only (SW_ALPHABET_PROTEIN): every call below returns
 *             SW_ERR_UNSUPPORTED on a DNA bank.  The batch holds DNA byte codes 0..4: the host
 *             forms return SW_ERR_ARG for a code of 5 or more, the device forms validate nothing
 *             and translate such a code as X.
 */
#define SWBANK_HAS_FRAMES 1
#define SW_FRAME_COUNT 6

/* Host, no device: out[0..) = the translation of frame `frame` (0..5) of codes[0..n); returns
 * the codons written (0 for a NULL codes or out, a frame above 5 or a table entry >= 24). */
size_t sw_translate_codes(const uint8_t *codes, size_t n, uint32_t frame,
                          const uint8_t *codon_table, uint8_t *out);

/* Device buffers, asynchronous on `stream` (NULL = the bank's): translates the batch (as for
 * sw_score_batch_device: targets at any byte offset, d_lens[k] may be 0, every d_lens[k] <=
 * max_len) into 6n protein targets, frame-major: translated target f * n + k is frame f of
 * target k, its codes at d_out + (f * n + k) * out_stride, that offset in
 * d_out_offsets[f * n + k] and its length in d_out_lens[f * n + k].  Nothing is written past a
 * translated target's length.  out_stride >= max(max_len / 3, 1), else SW_ERR_ARG.  The reverse
 * frames read the target from its far end; no reverse complement is made.  Neither penalties
 * nor a query are needed: a library is translated once and handed to sw_score_batch_device,
 * sw_estimate_statistics_device and the rest as an ordinary protein batch (whose padding the
 * caller zeroes, as for any batch).  A multi-device bank runs it on its root.  SW_ERR_ARG: a
 * NULL bank or buffer, n == 0, 6n >= 2^32.  sw_last_kernel reports "translate n=<n>". */
sw_status sw_translate_batch_device(sw_bank *bank, const uint8_t *d_residues,
                                    const uint64_t *d_offsets, const uint32_t *d_lens, size_t n,
                                    uint32_t max_len, const uint8_t *codon_table, uint8_t *d_out,
                                    size_t out_stride, uint64_t *d_out_offsets,
                                    uint32_t *d_out_lens, void *stream);

/* Device buffers, asynchronous on `stream`: scores the six frames of every target against the
 * loaded query or query set.  With nq = sw_query_count(): d_scores receives the merged nq x n
 * int32 scores, query-major; d_frames (may be NULL) the nq x n uint8 frames.  The batch runs in
 * slices of targets whose scratch (six translations at a stride of max_len / 3, their offsets
 * and lengths, 6 nq scores per target) is bounded by SWBANK_FRAME_MB (MiB, default 256);
 * slicing cannot change a result.  A slice is translated and its 6 nk translated targets are
 * scored in ONE sw_score_batch_device_range call over the lengths
 * [(max(min_len, 2) - 2) / 3, max_len / 3], so the length sort and the balanced ranges see all
 * frames together; a single query stays on the single-query kernels, multi-device dealing is
 * that of a forward search; a merge kernel follows.  No best hit is tracked.  A latched hand-off
 * fault of an earlier device call is returned as by the other device calls; sw_bank_sync waits
 * for the merge.  SW_ERR_STATE without penalties or a query; SW_ERR_ARG for min_len > max_len, a
 * NULL buffer (n > 0) or n >= 2^32; n == 0 is SW_OK.  sw_last_kernel reports
 * "frames nq=<nq> n=<n> slices=<s>"; with sw_bank_set_timing the translation and the merge are
 * each bracketed as one launch per slice, beside the scoring pass's own. */
sw_status sw_score_frames_device(sw_bank *bank, const uint8_t *d_residues,
                                 const uint64_t *d_offsets, const uint32_t *d_lens, size_t n,
                                 uint32_t min_len, uint32_t max_len, const uint8_t *codon_table,
                                 int32_t *d_scores, uint8_t *d_frames, void *stream);

/* Host buffers, blocking; the batch as for sw_score_batch (a target outside the residues or a
 * code of 5 or more is SW_ERR_ARG): uploads it once and calls the device form.  scores_out:
 * nq x n; frames_out: nq x n, may be NULL. */
sw_status sw_score_frames(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                          const uint64_t *offsets, const uint32_t *lens, size_t n,
                          const uint8_t *codon_table, int32_t *scores_out, uint8_t *frames_out);

/* sw_align_set_hits[_device] on the translation of each hit's frame.  The pair list is that
 * call's (hit_queries or hits_per_query, hits or h itself, the SW_QUERY_NONE / SW_HIT_NONE
 * sentinels); frames is the nq x n matrix sw_score_frames writes and is required (NULL:
 * SW_ERR_ARG).  Hit h (query i, target k) is aligned against frame f = frames[i * n + k] of
 * target k; only the listed hits are translated.  Every rule of sw_align_set_hits (end, start,
 * CIGAR preference, empty pair, SW_ALIGN_NO_PATH, the SWBANK_ALIGN_MB budget and its chunks)
 * holds on the translated target: the record is what that call returns for a batch holding the
 * translation, except that
 *   index and id name the DNA target: k, and ids[k] or k;
 *   flags |= (f % 3) << SW_ALIGN_FRAME_SHIFT, and |= SW_ALIGN_REVERSE for f >= 3 (an empty pair
 *   too, never a slot that names no pair);
 *   t_start and t_end are nucleotide positions on the forward target, 0-based, inclusive,
 *   t_start <= t_end: with the alignment over amino positions a_start..a_end of the frame,
 *   o = f % 3 and L the target's length,
 *     forward   t_start = o + 3 a_start,                t_end = o + 3 a_end + 2
 *     reverse   t_start = L - 1 - (o + 3 a_end + 2),    t_end = L - 1 - (o + 3 a_start)
 *   (an empty pair keeps 0).
 * q_*, n_columns, n_identities and the CIGAR stay in amino-acid columns: an identity is a pair
 * of equal protein codes, a D op consumes one codon.  The device form treats a frame above 5 as
 * a target without codons (an empty pair, no frame flags); the host form returns SW_ERR_ARG for
 * a listed pair whose frame is above 5 and for a code of 5 or more in a listed target.
 * max_len >= every d_lens[k].  sw_last_kernel reports
 * "align-frame i32 nq=<nq> hits=<n_hits> chunks=<c>". */
enum { SW_ALIGN_FRAME_SHIFT = 4, SW_ALIGN_FRAME_MASK = 0x30 }; /* flags: f % 3 of the hit's frame */

sw_status sw_align_frame_hits_device(sw_bank *bank, const uint8_t *d_residues,
                                     const uint64_t *d_offsets, const uint32_t *d_lens,
                                     const uint64_t *d_ids, size_t n, uint32_t max_len,
                                     const uint8_t *codon_table, const uint8_t *d_frames,
                                     const uint32_t *d_hit_queries, size_t hits_per_query,
                                     const uint64_t *d_hits, size_t n_hits, sw_alignment *d_out,
                                     uint32_t *d_cigar, uint32_t cigar_stride, void *stream);

sw_status sw_align_frame_hits(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                              const uint64_t *offsets, const uint32_t *lens, const uint64_t *ids,
                              size_t n, const uint8_t *codon_table, const uint8_t *frames,
                              const uint32_t *hit_queries, size_t hits_per_query,
                              const uint64_t *hits, size_t n_hits, sw_alignment *out,
                              uint32_t *cigar, size_t cigar_cap, size_t *cigar_used);

/* ---- frameshift-tolerant translated search: one score over the three frames of a strand (ABI 6
 *      addition) -----------------------------------------------------------------------------
 * The six-frame search above scores the frames as six unrelated proteins, so a single-base
 * insertion or deletion inside a coding region (raw reads, ESTs, draft assemblies) cuts the hit
 * in two and only the longer half is reported.  The calls below score a strand's three frames in
 * ONE matrix whose cells may step from one frame to another at a price.  This is this library's
 * own definition: the FASTA suite's tfasty and tfastx penalise shifts differently, and nothing
 * in the project this one was modelled on pins it.
 *
 * Definition:
 *   strand    L DNA codes c[0..L) (T, C, A, G = 0..3, N = 4).  The forward strand is the target,
 *             the reverse strand rc(target), rc as sw_revcomp_codes.
 *   columns   codon starts p = 0 .. L - 3.  The amino acid a(p) is the translation of c[p],
 *             c[p + 1], c[p + 2] by the rules of the translated search above: the same
 *             codon_table argument, any code of 4 or more gives X, * is scored like any residue.
 *   rows      i = 0 .. m - 1 over the protein query q.
 *   scores    with o = gap_open + gap_extend and e = gap_extend, the bank's Gotoh penalties, and
 *             the frameshift penalty fs <= 0:
 *               M(i,p) = s(q_i, a(p)) + max(0, H(i-1,p-3), H(i-1,p-2) + fs, H(i-1,p-4) + fs)
 *               E(i,p) = max(H(i,p-3) + o, E(i,p-3) + e)      a codon of the target against a gap
 *               F(i,p) = max(H(i-1,p) + o, F(i-1,p) + e)      a query residue against a gap
 *               H(i,p) = max(0, M(i,p), E(i,p), F(i,p))
 *             H is 0 and E, F are -infinity outside 0 <= i < m, 0 <= p <= L - 3.  The frame of a
 *             column is p mod 3: p - 3 stays in the frame, p - 2 re-reads one base, p - 4 skips
 *             one base.
 *   result    the strand score is the maximum of H, 0 when L < 3; the search score is the larger
 *             of the two strand scores; the strand output is 0 (forward) unless the reverse
 *             strand is strictly better.
 * While every score stays below 32,767, fs = -32767 can never win: the search then equals the
 * merged six-frame score of sw_score_frames, and the strand is (frame >= 3).
 *
 * Limits: protein banks only (a DNA bank: SW_ERR_UNSUPPORTED); the Gotoh gap model only
 * (SW_GAP_MERGED: SW_ERR_UNSUPPORTED); 0 >= frameshift >= -32767 (else SW_ERR_ARG); every query
 * of the loaded set has at most SW_FSHIFT_MAX_QUERY rows (else SW_ERR_UNSUPPORTED).  Scores are
 * exact int32 with no width limit.  The bank's two scoring limits hold all the same, although
 * the int32 kernel has neither: a matrix with max(0, largest entry) - smallest entry > 254, or
 * Gotoh penalties with |gap_open| + |gap_extend| + max(0, largest entry) > 65535, is refused with
 * SW_ERR_RANGE by sw_score_fshift[_device], sw_align_fshift_hits[_device] and
 * sw_estimate_fshift_statistics[_device] alike (each prepares the bank's query tables, which are
 * built for the 16-bit kernels), after the checks above and each call's argument checks and
 * before any output is written; the bank stays usable.  Everything else of 0 >= gap_open,
 * gap_extend >= -32767 and of int8 matrices is accepted: zero penalties, matrices without a
 * positive entry (every score 0), entries of -128.  Alignments of shifted hits:
 * sw_align_fshift_hits[_device] below; their statistics: sw_estimate_fshift_statistics[_device]
 * after those. */
#define SWBANK_HAS_FSHIFT 1
#define SW_FSHIFT_MAX_QUERY 1024

/* Device buffers, asynchronous on `stream` (NULL = the bank's): the batch as for
 * sw_score_frames_device (every d_lens[k] <= max_len: codes of a target past max_len are not
 * read; a code of 5 or more reads as N).  With nq = sw_query_count(): d_scores receives the
 * nq x n int32 search scores, query-major -- the layout sw_top_hits_device takes, so the top-k
 * list chains on the same stream -- and d_strands (may be NULL) the nq x n uint8 strands.  One
 * kernel reads the targets as they lie: no translation and no reverse complement is made, the
 * call owns no scratch.  No best hit is tracked.  SW_ERR_STATE without penalties or a query;
 * n == 0 is SW_OK; a NULL buffer (n > 0), n >= 2^32 or a table entry >= 24 is SW_ERR_ARG.  A
 * latched hand-off fault of an earlier device call is returned as by the other device calls; a
 * multi-device bank runs the call on its root; sw_bank_sync covers it.  sw_last_kernel reports
 * "fshift nq=<nq> n=<n>"; with sw_bank_set_timing the call is bracketed as one launch. */
sw_status sw_score_fshift_device(sw_bank *bank, const uint8_t *d_residues,
                                 const uint64_t *d_offsets, const uint32_t *d_lens, size_t n,
                                 uint32_t max_len, const uint8_t *codon_table, int32_t frameshift,
                                 int32_t *d_scores, uint8_t *d_strands, void *stream);

/* Host buffers, blocking; the batch as for sw_score_frames (a target outside the residues or a
 * code of 5 or more is SW_ERR_ARG): uploads it once and calls the device form.  scores_out:
 * nq x n; strands_out: nq x n, may be NULL. */
sw_status sw_score_fshift(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                          const uint64_t *offsets, const uint32_t *lens, size_t n,
                          const uint8_t *codon_table, int32_t frameshift, int32_t *scores_out,
                          uint8_t *strands_out);

/* ---- alignments of frameshift hits (ABI 6 addition) ---------------------------------------------
 * Where a hit of the frameshift-tolerant search lies and where it changes frame: the step that
 * follows sw_score_fshift_device -> sw_top_hits_device on the same stream.  The pair list is that
 * of sw_align_set_hits (hit_queries or hits_per_query, hits or h itself, the SW_QUERY_NONE /
 * SW_HIT_NONE sentinels).  The call takes no strand matrix: it scores both strands itself.
 *
 * Everything is defined on the hit's strand c[0..L), the target or rc(target), over the matrices
 * M, E, F, H of the definition above; a cell is (i, p), query row i and codon start p.
 *   score   what sw_score_fshift returns for the pair; the forward strand unless the reverse
 *           strand is strictly better (then flags |= SW_ALIGN_REVERSE).
 *   end     among the cells with H = score: the smallest p, then the smallest i.  The end cell is
 *           walked as an M cell.
 *   start   among the first cells of optimal alignments that end there: the largest p, then the
 *           largest i -- the same rule on the reversed problem (rows q[q_end..0], columns
 *           p_end..0, each column keeping its forward codon): between two consecutive match
 *           cells the forward and the reversed recurrence consume the same bases and pay the same
 *           penalties, only the gap cells move by a base.
 *   CIGAR   an op is len << 4 | code, adjacent equal codes merged, the first and the last op M.
 *           SW_CIGAR_M, _I, _D as in the translated search: amino-acid columns, a D consumes one
 *           codon.  Two more codes, always of length 1, each directly before the M run it leads
 *           into: SW_CIGAR_FS_SKIP, text '/': the next codon starts one base later than the frame
 *           says (the p - 4 link); SW_CIGAR_FS_BACK, text '\': it starts one base earlier,
 *           re-reading a base (the p - 2 link).  The ops consume (M + I) = q_end - q_start + 1
 *           query rows and 3 (M + D) + (count of '/') - (count of '\') = p_end + 2 - p_start + 1
 *           bases; re-scoring them gives `score`: an M scores s(q_i, a(p)), a gap run of k
 *           columns costs open + k * extend, a shift costs `frameshift`.  n_columns = M + I + D
 *           columns, n_identities = M columns with q_i == a(p).  The path is optimal among the
 *           paths from the start cell to the end cell, values taken in that anchored matrix (a 0
 *           diagonal at the start cell only, no floor).  Walking back from the end cell: in state
 *           H, M first, then E (D), then F (I); in an M cell the in-frame link p - 3, then p - 2
 *           ('\'), then p - 4 ('/'); a gap run opens rather than extends when both are optimal.
 *   record  index and id name the DNA target; flags |= (p_start mod 3) << SW_ALIGN_FRAME_SHIFT,
 *           the frame of the first codon on its strand; t_start and t_end are nucleotide positions
 *           on the forward target, 0-based, inclusive:
 *             forward   t_start = p_start,                 t_end = p_end + 2
 *             reverse   t_start = L - 1 - (p_end + 2),     t_end = L - 1 - p_start
 *           q_* are query rows.  The empty pair (score 0, L < 3 included) is SW_ALIGN_EMPTY: every
 *           coordinate 0, no ops, no strand or frame bits.
 * SW_ALIGN_NO_PATH (exact coordinates, no ops, n_columns = n_identities = 0), the SW_ALIGN_NO_HIT
 * sentinel slots, the cigar_offset = h * cigar_stride device layout, the packed host layout and
 * the SWBANK_ALIGN_MB budget with its chunks are those of sw_align_set_hits.  While scores stay
 * below 32,767 and one frame of the six is strictly best, the record at frameshift = -32767 equals
 * the record of sw_align_frame_hits for that frame, field for field and op for op.
 *
 * Limits and refusals are sw_score_fshift's, in its order: protein banks, the Gotoh model, the
 * frameshift range, the codon table, the state, queries of at most SW_FSHIFT_MAX_QUERY rows; then
 * max_len (the host form: the longest listed target) of less than 2^29, else SW_ERR_UNSUPPORTED.  A
 * latched hand-off fault is returned as elsewhere; a multi-device bank runs the call on its root.
 * sw_last_kernel reports "align-fshift i32 nq=<nq> hits=<n_hits> chunks=<c>"; with
 * sw_bank_set_timing the end / start passes and the path passes are bracketed as one launch each.
 * One workgroup aligns one hit, with K = 4, 8 or 16 rows per lane by the longest loaded query; a
 * window of r rows and c codon starts takes (ceil(c / 3) + ceil(r / K) - 1) x 192 K bytes of the
 * direction store. */
#define SWBANK_HAS_FSHIFT_ALIGN 1
enum { SW_CIGAR_FS_SKIP = 3, SW_CIGAR_FS_BACK = 4 };

/* Device buffers, asynchronous on `stream`: as sw_align_frame_hits_device without the frames.  The
 * slots of the direction store are sized from max_len x the longest query; if one does not fit
 * SWBANK_ALIGN_MB, every non-empty hit gets SW_ALIGN_NO_PATH. */
sw_status sw_align_fshift_hits_device(sw_bank *bank, const uint8_t *d_residues,
                                      const uint64_t *d_offsets, const uint32_t *d_lens,
                                      const uint64_t *d_ids, size_t n, uint32_t max_len,
                                      const uint8_t *codon_table, int32_t frameshift,
                                      const uint32_t *d_hit_queries, size_t hits_per_query,
                                      const uint64_t *d_hits, size_t n_hits, sw_alignment *d_out,
                                      uint32_t *d_cigar, uint32_t cigar_stride, void *stream);

/* Host buffers, blocking: gathers and uploads only the listed targets (a code of 5 or more in one
 * is SW_ERR_ARG) and plans its chunks from the actual windows after one small copy of the
 * coordinates back, so only a single window over the budget loses its path. */
sw_status sw_align_fshift_hits(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                               const uint64_t *offsets, const uint32_t *lens, const uint64_t *ids,
                               size_t n, const uint8_t *codon_table, int32_t frameshift,
                               const uint32_t *hit_queries, size_t hits_per_query,
                               const uint64_t *hits, size_t n_hits, sw_alignment *out,
                               uint32_t *cigar, size_t cigar_cap, size_t *cigar_used);

/* ---- statistics of frameshift hits (ABI 6 addition) ----------------------------------------------
 * Lambda and K of the frameshift-tolerant search, estimated like those of the plain search ("hit
 * significance" above) but with this search's own score: three frames in one matrix and two
 * strands give chance more places to score, so a fit made on a forward protein search would
 * understate E.
 *
 * Definition.  For every round r < rounds (rounds >= 1):
 *   - target k of the DNA batch is shuffled under seed + r exactly as sw_shuffle_batch_device
 *     defines it: the bases are shuffled, N included, keyed by the batch position k;
 *   - every loaded query is scored against every shuffled target with the search score of
 *     sw_score_fshift (the larger of the two strand scores) under `codon_table` and `frameshift`;
 *   - the scores go into one histogram row per query exactly as sw_score_histogram_device counts
 *     them, the lengths being the targets' lengths in NUCLEOTIDES; targets of length 0 are skipped.
 * After the last round row i is fitted by sw_fit_statistics with query_len = the residues of query
 * i, into out[0 .. sw_query_count()), host memory.  n_samples, n_clamped, SW_STAT_CLAMPED and
 * SW_STAT_DEGENERATE are as for sw_estimate_statistics.
 *
 * Significance of a hit: sw_hit_significance[_device] unchanged, with d_lens / target_lens in
 * nucleotides (the batch's own lengths, as sw_top_hits_device indexes them) and db_size the number
 * of library sequences.  Both strands are already inside the score, as they are inside the
 * shuffled scores the fit was made on: db_size is not doubled.
 *
 * The work is enqueued on `stream` (NULL = the bank's) and the call returns after synchronising
 * it.  The scratch (shuffled bases at a stride of max_len and nq x n scores) is bounded by
 * SWBANK_STAT_MB as for sw_estimate_statistics_device, and slices cannot change a count.  Limits
 * and refusals are sw_score_fshift's, in its order: protein banks, the Gotoh model, the frameshift
 * range, the codon table, the state, queries of at most SW_FSHIFT_MAX_QUERY rows; then
 * SW_ERR_ARG for a NULL buffer or out, n == 0, n >= 2^32, rounds == 0.  A latched hand-off fault
 * is returned as elsewhere; a multi-device bank runs the call on its root.  No best hit is
 * tracked.  sw_last_kernel reports "fshift-stats rounds=<r> nq=<nq> n=<n> slices=<s>"; with
 * sw_bank_set_timing every shuffle, scoring and histogram pass of a slice is bracketed as one
 * launch each (3 x rounds x slices in all). */
#define SWBANK_HAS_FSHIFT_STATS 1

/* Device buffers: the batch as for sw_score_fshift_device (every d_lens[k] <= max_len). */
sw_status sw_estimate_fshift_statistics_device(sw_bank *bank, const uint8_t *d_residues,
                                               const uint64_t *d_offsets, const uint32_t *d_lens,
                                               size_t n, uint32_t max_len,
                                               const uint8_t *codon_table, int32_t frameshift,
                                               uint64_t seed, uint32_t rounds, sw_statistics *out,
                                               void *stream);

/* Host buffers, blocking; the batch as for sw_score_fshift (a target outside the residues or a
 * code of 5 or more is SW_ERR_ARG): uploads it once and calls the device form. */
sw_status sw_estimate_fshift_statistics(sw_bank *bank, const uint8_t *residues,
                                        size_t residues_len, const uint64_t *offsets,
                                        const uint32_t *lens, size_t n, const uint8_t *codon_table,
                                        int32_t frameshift, uint64_t seed, uint32_t rounds,
                                        sw_statistics *out);

/* ---- global-local search: a query or a target scored end to end (ABI 6 addition) ---------------
 * Every other score of this library is local: the best piece of the query against the best piece
 * of the target, floored at 0.  The calls below score the whole query (what the FASTA suite's
 * glsearch36 does), the whole target (reads as the batch against a set of references) or both
 * (ggsearch36) with penalised boundaries, no floor and negative scores.  The definition is this
 * library's own; nothing in the project this one was modelled on pins it.
 *
 * Definition: rows i = 0 .. m - 1 over the query q, columns j = 0 .. L - 1 over the strand t
 * walked, o = gap_open + gap_extend and e = gap_extend (the bank's Gotoh penalties), no floor:
 *     M(i,j) = s(q_i, t_j) + H(i-1, j-1)
 *     E(i,j) = max(H(i, j-1) + o, E(i, j-1) + e)      a target residue against a gap
 *     F(i,j) = max(H(i-1, j) + o, F(i-1, j) + e)      a query residue against a gap
 *     H(i,j) = max(M, E, F)
 * H(-1,-1) = 0; E and F are -infinity outside the matrix.  `ends` selects the boundaries and the
 * result:
 *     ends                 H(i,-1), i >= 0   H(-1,j), j >= 0   score                        end position
 *     SW_ENDS_QUERY  (1)   o + i e           0                 max over j = -1 .. L-1 of    that j, the smallest
 *                                                              H(m-1, j)                    on a tie
 *     SW_ENDS_TARGET (2)   0                 o + j e           max over i = -1 .. m-1 of    that i, the smallest
 *                                                              H(i, L-1)                    on a tie
 *     SW_ENDS_BOTH   (3)   o + i e           o + j e           H(m-1, L-1)                  SW_END_NONE
 * QUERY: the query end to end, the target local.  TARGET: the target end to end, the query local.
 * The boundary index -1 is reported as SW_END_NONE: it is what L = 0 gives, or a query (a target)
 * that is all gap.  With both_strands the reverse strand is rc(target), rc as sw_revcomp_codes;
 * the search score is the larger strand score, the strand is 0 unless the reverse strand is
 * strictly better, and a QUERY end position on the reverse strand is reported on the forward
 * target, as L - 1 - j (a TARGET end position is a query row on either strand).
 *
 * Limits and refusals, checked in this order before anything else: both_strands on a protein bank
 * is SW_ERR_UNSUPPORTED (DNA and protein banks are both accepted otherwise); SW_GAP_MERGED is
 * SW_ERR_UNSUPPORTED; ends outside 1 .. 3 is SW_ERR_ARG; SW_ERR_STATE without penalties or a
 * query; every query of the loaded set has at most SW_GLOCAL_MAX_QUERY rows, else
 * SW_ERR_UNSUPPORTED.  Then each call's argument checks (n == 0 is SW_OK; a NULL buffer (n > 0) or
 * n >= 2^32 is SW_ERR_ARG).  Then SW_ERR_RANGE, before any output is written and with the bank
 * left usable: the bank's two scoring limits (see sw_score_fshift: the call prepares the bank's
 * query tables), and one rule of its own,
 *     |o| + (1024 + 64 + max_len) x max(|e|, 128) < 2^30
 * with the caller's max_len (the host form: the longest listed target).  Every real cell lies at
 * or above -(|o| + (m + L) x max(|e|, |smallest entry|)); the rule leaves room for the kernel's pad
 * rows.  Scores are exact int32 and may be negative: sw_top_hits_device and
 * sw_best_queries_device take them unchanged (mind min_score). */
#define SWBANK_HAS_GLOCAL 1
#define SW_GLOCAL_MAX_QUERY 1024
#define SW_END_NONE UINT32_MAX
enum { SW_ENDS_QUERY = 1, SW_ENDS_TARGET = 2, SW_ENDS_BOTH = 3 };

/* Device buffers, asynchronous on `stream` (NULL = the bank's): the batch as for
 * sw_score_batch_device (targets at any byte offset, d_lens[k] may be 0, every d_lens[k] <=
 * max_len: codes of a target past max_len are not read).  Nothing is validated: a code past the
 * bank's alphabet reads as the alphabet's last code -- N on a DNA bank, * (code 23) on a protein
 * bank, the one code every protein matrix scores like an unknown residue.  With nq =
 * sw_query_count(): d_scores receives the nq x n int32 scores, query-major; d_end_pos (may be
 * NULL) the nq x n uint32 end positions; d_strands (may be NULL) the nq x n uint8 strands, all 0
 * without both_strands.  One kernel reads the targets as they lie; the call owns no scratch.  No
 * best hit is tracked.  A latched hand-off fault of an earlier device call is returned as by the
 * other device calls; a multi-device bank runs the call on its root; sw_bank_sync covers it.
 * sw_last_kernel reports "glocal ends=<e> nq=<nq> n=<n>"; with sw_bank_set_timing the call is
 * bracketed as one launch. */
sw_status sw_score_glocal_device(sw_bank *bank, const uint8_t *d_residues,
                                 const uint64_t *d_offsets, const uint32_t *d_lens, size_t n,
                                 uint32_t max_len, int32_t ends, int32_t both_strands,
                                 int32_t *d_scores, uint32_t *d_end_pos, uint8_t *d_strands,
                                 void *stream);

/* Host buffers, blocking; the batch as for sw_score_batch (a target outside the residues or a
 * code outside the bank's alphabet is SW_ERR_ARG): uploads it once and calls the device form.
 * scores_out: nq x n; end_pos_out and strands_out: nq x n, each may be NULL. */
sw_status sw_score_glocal(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                          const uint64_t *offsets, const uint32_t *lens, size_t n, int32_t ends,
                          int32_t both_strands, int32_t *scores_out, uint32_t *end_pos_out,
                          uint8_t *strands_out);

/* ---- alignments of global-local hits (ABI 6 addition) ------------------------------------------
 * Where a pair of sw_score_glocal aligns: the start, a CIGAR and the identities.  The pair list,
 * SW_ALIGN_NO_PATH, the SW_ALIGN_NO_HIT sentinel slots, the cigar_offset layouts, the packed host
 * layout, the SWBANK_ALIGN_MB budget and its chunks are sw_align_set_hits[_device]'s.
 * sw_align_set_hits itself cannot stand in: it aligns the best local piece, floored at 0, which
 * is another alignment with another score.
 *
 * Everything is stated on the strand walked, c[0..L): the target or rc(target).  H, E, F and the
 * boundaries are those of "global-local search" above for the call's `ends`; a path runs from a
 * boundary cell to the end cell.
 *   score   what sw_score_glocal returns for the pair; the forward strand unless the reverse
 *           strand is strictly better (then flags |= SW_ALIGN_REVERSE).
 *   end     the score call's end position: QUERY the cell (m-1, j_end), the smallest such j;
 *           TARGET (i_end, L-1), the smallest such i; BOTH (m-1, L-1).  The end cell is walked in
 *           state H, not forced to M: a query tail may lie against a gap.
 *   start   the boundary cell the path leaves from.  QUERY: a cell (-1, c), -1 <= c < j_end;
 *           among the c for which a path from (-1, c) to the end cell scores `score` -- which is
 *           to say that the BOTH score of q against c[c+1 .. j_end] equals `score`; no c gives
 *           more -- the largest is taken, and t_start = c + 1.  TARGET: the transpose, the largest
 *           r gives q_start = r + 1.  BOTH: (-1, -1).
 *   CIGAR   an optimal path of the anchored matrix over the window [q_start..q_end] x
 *           [t_start..t_end]: both boundaries penalised, no floor; its value at the last cell is
 *           `score`.  An op is len << 4 | code with the codes M, I, D above, adjacent equal codes
 *           merged.  The first and the last op need NOT be M ("3I40M", "40M2I").  The ops consume
 *           exactly the window's rows and columns, and re-scoring them gives `score`: a gap run of
 *           k columns costs open + k * extend, a run being a maximal stretch of one code.  Walking
 *           back from the end cell: the diagonal (M) first, then a gap from the left (D), then a
 *           gap from above (I); a gap run opens rather than extends when both are optimal; on
 *           reaching row -1 the rest of the path is D ops, on column -1 I ops.  n_columns = M + I
 *           + D columns; n_identities = M columns with equal codes, the complemented code on the
 *           reverse strand.
 *   record  ends     q_start  q_end  t_start  t_end
 *           QUERY    0        m-1    c+1      j_end
 *           TARGET   r+1      i_end  0        L-1
 *           BOTH     0        m-1    0        L-1
 *           A reverse hit reports t_start = L-1 - t_end' and t_end = L-1 - t_start' of the strand
 *           walked, as sw_align_strand_hits does; its CIGAR runs along the strand walked.
 *   empty   the boundary won: SW_END_NONE under QUERY or TARGET, L = 0 under BOTH.  The record is
 *           SW_ALIGN_EMPTY with `score` the boundary's value, which may be negative; every
 *           coordinate and count is 0 and there are no ops.  An empty pair is never reverse (both
 *           strands tie).  For these calls SW_ALIGN_EMPTY therefore means "no cell aligned", not
 *           "score 0", and a record with a path may score 0 or less.
 *
 * Limits and refusals are sw_score_glocal's, in its order (both_strands on a protein bank, the
 * gap model, ends, the state, the query length); then a latched hand-off fault (the device form),
 * the multi-device bank running on its root, n_hits == 0 (SW_OK), a NULL buffer or n == 0
 * (SW_ERR_ARG), the pair list's checks, n_hits x cigar_stride >= 2^32 (SW_ERR_ARG), and the
 * SW_ERR_RANGE rules of sw_score_glocal with the caller's max_len (the host form: the longest
 * listed target, after its SW_ERR_ARG checks of the listed targets).  Nothing is written by a
 * refused call.  The device form sizes its direction-store slots from max_len x the longest
 * query and validates nothing it would have to read back; the host form gathers only the listed
 * targets, checks their codes against the bank's alphabet and plans its chunks from the actual
 * windows.  sw_last_kernel reports "align-glocal i32 ends=<e> nq=<nq> hits=<n_hits> chunks=<c>";
 * with sw_bank_set_timing the end / start passes and the path passes are bracketed as one launch
 * each. */
#define SWBANK_HAS_GLOCAL_ALIGN 1

sw_status sw_align_glocal_hits_device(sw_bank *bank, const uint8_t *d_residues,
                                      const uint64_t *d_offsets, const uint32_t *d_lens,
                                      const uint64_t *d_ids, size_t n, uint32_t max_len,
                                      int32_t ends, int32_t both_strands,
                                      const uint32_t *d_hit_queries, size_t hits_per_query,
                                      const uint64_t *d_hits, size_t n_hits, sw_alignment *d_out,
                                      uint32_t *d_cigar, uint32_t cigar_stride, void *stream);

sw_status sw_align_glocal_hits(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                               const uint64_t *offsets, const uint32_t *lens,
                               const uint64_t *ids, size_t n, int32_t ends, int32_t both_strands,
                               const uint32_t *hit_queries, size_t hits_per_query,
                               const uint64_t *hits, size_t n_hits, sw_alignment *out,
                               uint32_t *cigar, size_t cigar_cap, size_t *cigar_used);

/* ---- non-intersecting local alignments: the next best hits of a pair (ABI 6 addition) -----------
 * sw_align_set_hits reports the best local alignment of a pair.  These calls report up to `rounds`
 * of them in order: the best one, then the best one that shares no matrix cell with it, and so on
 * (Waterman and Eggert; what lalign36 prints) -- the second copy of a repeated domain, the second
 * occurrence of a read's motif.  The pair list (hit_queries / hits_per_query / hits), the
 * SW_ALIGN_NO_HIT sentinel slots and the sw_alignment record are sw_align_set_hits[_device]'s; a
 * bank with one query is a set of one.  One strand, DNA and protein banks, SW_GAP_GOTOH only.
 *
 * The definition, for a pair with m rows and L columns, o = open + extend, e = extend.  Round r
 * has a set U_r of used cells; U_0 is empty.
 *     (i,j) in U_r :  H = 0, E = F = -inf            nothing passes through a used cell
 *     otherwise    :  M = s(q_i,t_j) + H(i-1,j-1)
 *                     E = max(H(i,j-1) + o, E(i,j-1) + e)
 *                     F = max(H(i-1,j) + o, F(i-1,j) + e)
 *                     H = max(0, M, E, F)
 * with the boundaries H = 0 and E = F = -inf.
 *   score   score_r is the largest H of round r.  score_0 is the pair's local Gotoh score, what
 *           sw_score_batch returns; scores never increase with r.  If score_r < min_score, this
 *           slot and every later slot of the hit is SW_ALIGN_EMPTY with score 0, every coordinate
 *           and count 0 and no ops.
 *   end     among the cells with H = score_r: the smallest t_end, then the smallest q_end
 *           (sw_align_hits's rule).
 *   path    walked back from the end cell in state H.  A cell with H = 0 ends the walk and is not
 *           part of the path; otherwise the source M is taken first, then E (op D), then F (op
 *           I); a gap run opens rather than extends on a tie.  The cell where the walk stops gives
 *           q_start / t_start.  The first and the last op are M.  n_columns and n_identities are
 *           as for sw_align_hits, and re-scoring the ops gives score_r.
 *   used    U_{r+1} = U_r and every cell the path of round r visits in any state: the cell of
 *           each M, D and I column.  The paths of one hit are therefore pairwise cell-disjoint.
 *   ops     a path with more ops than its CIGAR slot gets SW_ALIGN_NO_PATH with exact coordinates;
 *           its cells are marked all the same, so later rounds do not depend on the caller's
 *           cigar_stride.
 *   layout  the record of (hit h, round r) is out[h * rounds + r].  The device form puts its ops
 *           at d_cigar + (h * rounds + r) * cigar_stride (cigar_offset says so); d_cigar == NULL
 *           or cigar_stride == 0: coordinates only, every non-empty record gets SW_ALIGN_NO_PATH.
 *           The host form packs the CIGARs back to back in that order into cigar[0..cigar_cap),
 *           *cigar_used (may be NULL) = ops written; a record whose ops no longer fit gets
 *           SW_ALIGN_NO_PATH.  A slot that names no pair has SW_ALIGN_NO_HIT in all its `rounds`
 *           records.
 *
 * Limits: queries of at most SW_DISJOINT_MAX_QUERY rows, 1 <= rounds <= SW_DISJOINT_MAX_ROUNDS,
 * min_score >= 1.  Every round walks the whole m x L matrix and keeps one direction byte per cell
 * (bit 7 of it is the used flag), so the direction store of ONE hit, about (L + m / K) x 64K bytes
 * with K = 4, 8 or 16 rows per lane for a longest query of at most 256, 512 or 1,024 rows, must fit
 * SWBANK_ALIGN_MB (MiB, default 256); the hits run in chunks that fit it together, `rounds`
 * launches per chunk.
 *
 * Refusals, in this order: the gap model (SW_ERR_UNSUPPORTED); the state, penalties or query not
 * loaded (SW_ERR_STATE); a longest query over SW_DISJOINT_MAX_QUERY rows (SW_ERR_UNSUPPORTED);
 * rounds or min_score out of range (SW_ERR_ARG); a latched hand-off fault (the device form); the
 * multi-device bank running on its root; n_hits == 0 (SW_OK); a NULL buffer or n == 0
 * (SW_ERR_ARG); the pair list's checks (the host form: then those of the listed targets, all
 * SW_ERR_ARG); n_hits x rounds or n_hits x rounds x cigar_stride >= 2^32 (SW_ERR_ARG); a direction
 * slot that alone exceeds SWBANK_ALIGN_MB (SW_ERR_UNSUPPORTED, the text names the knob): without
 * the store there is no used set, so there is nothing exact to return.  A refused call writes
 * nothing.  The device form sizes every slot from max_len x the longest query and reads nothing
 * back; the host form gathers only the listed targets, checks their codes against the bank's
 * alphabet and sizes each slot from the lengths it knows.  sw_last_kernel reports
 * "align-disjoint i32 rounds=<r> nq=<nq> hits=<n_hits> chunks=<c>"; with sw_bank_set_timing the
 * rounds of a chunk are bracketed as one launch. */
#define SWBANK_HAS_DISJOINT_ALIGN 1
#define SW_DISJOINT_MAX_QUERY 1024
#define SW_DISJOINT_MAX_ROUNDS 64

sw_status sw_align_disjoint_hits_device(sw_bank *bank, const uint8_t *d_residues,
                                        const uint64_t *d_offsets, const uint32_t *d_lens,
                                        const uint64_t *d_ids, size_t n, uint32_t max_len,
                                        uint32_t rounds, int32_t min_score,
                                        const uint32_t *d_hit_queries, size_t hits_per_query,
                                        const uint64_t *d_hits, size_t n_hits,
                                        sw_alignment *d_out, uint32_t *d_cigar,
                                        uint32_t cigar_stride, void *stream);

sw_status sw_align_disjoint_hits(sw_bank *bank, const uint8_t *residues, size_t residues_len,
                                 const uint64_t *offsets, const uint32_t *lens,
                                 const uint64_t *ids, size_t n, uint32_t rounds,
                                 int32_t min_score, const uint32_t *hit_queries,
                                 size_t hits_per_query, const uint64_t *hits, size_t n_hits,
                                 sw_alignment *out, uint32_t *cigar, size_t cigar_cap,
                                 size_t *cigar_used);

/* ---- non-intersecting alignments over reading frames: every exon of a hit (ABI 6 addition) ------
 * sw_align_frame_hits aligns a hit of the translated search on its one best frame, and
 * sw_align_disjoint_hits walks one matrix on one strand.  A protein's exons in a contig lie in
 * different reading frames and on either strand; these calls report up to `rounds` alignments of
 * a hit over all six frames, best first, in one call that chains behind sw_score_frames_device
 * and sw_top_hits_device on one stream.  Protein banks, SW_GAP_GOTOH only.  The batch holds DNA
 * codes as for sw_score_frames; codon_table is as there (NULL: the standard code).
 *
 * The definition.  For a hit (query i, target k of L codes) let S_f, f = 0..5, be the records
 * sw_align_disjoint_hits returns for the pair (query i, sw_translate_codes(target k, frame f)) at
 * the same `rounds` and min_score: non-increasing in score, ending at its first empty record.  The
 * call returns the first `rounds` records of the merge of S_0 .. S_5: at each step the head with
 * the largest score, a tie to the lowest frame; within a frame S_f's order.  When every head is
 * empty, that slot and every later slot of the hit is SW_ALIGN_EMPTY: score 0, all coordinates
 * and counts 0, no ops, no frame bits.  A record taken from frame f is S_f's record with, as
 * sw_align_frame_hits reports them,
 *   index and id naming the DNA target,
 *   flags |= (f % 3) << SW_ALIGN_FRAME_SHIFT, and |= SW_ALIGN_REVERSE for f >= 3,
 *   t_start / t_end in nucleotides on the forward target,
 * while q_*, the counts and the CIGAR stay in amino-acid columns.  A record with SW_ALIGN_NO_PATH
 * had more ops than its slot; its cells are used all the same.  It follows that record 0 has the
 * score and the frame of sw_score_frames (both break ties to the lowest frame), that scores never
 * increase along the records of a hit, and that two records of a hit in the same frame share no
 * cell.
 *
 * The layout (record (h, r) at out[h * rounds + r]), the pair list, the SW_ALIGN_NO_HIT sentinel
 * slots and the CIGAR placement of both forms are sw_align_disjoint_hits[_device]'s, and so are
 * SW_DISJOINT_MAX_QUERY, SW_DISJOINT_MAX_ROUNDS and min_score >= 1.  Round 0 walks the six
 * matrices at once and every later round only the matrix the previous record came from: 6 +
 * (rounds - 1) walks per hit.  The direction store of ONE hit, the sum over the frames of the
 * disjoint call's store for that frame's codons, must fit SWBANK_ALIGN_MB; the hits run in chunks
 * that fit it together, `rounds` launches per chunk.  The device form sizes every hit at six
 * stores of the longest query against max_len / 3 codons and reads nothing back; the host form
 * gathers only the listed targets, checks that their codes are DNA codes (< SW_DNA_ALPHA) and
 * sizes each hit from the lengths it knows, a CIGAR slot per round from the longest frame's
 * codons.
 *
 * Refusals, in this order: a DNA bank (SW_ERR_UNSUPPORTED); the gap model (SW_ERR_UNSUPPORTED);
 * the state, penalties or query not loaded (SW_ERR_STATE); a longest query over
 * SW_DISJOINT_MAX_QUERY rows (SW_ERR_UNSUPPORTED); rounds or min_score out of range, then a codon
 * table entry >= SW_PROTEIN_ALPHA (SW_ERR_ARG); a latched hand-off fault (the device form); the
 * multi-device bank running on its root; n_hits == 0 (SW_OK); a NULL buffer or n == 0
 * (SW_ERR_ARG); the pair list's checks (the host form: then those of the listed targets, all
 * SW_ERR_ARG); n_hits x rounds or n_hits x rounds x cigar_stride >= 2^32 (SW_ERR_ARG); a hit
 * whose store alone exceeds SWBANK_ALIGN_MB (SW_ERR_UNSUPPORTED, the text names the knob).  A
 * refused call writes nothing.  sw_last_kernel reports
 * "align-disjoint-frames i32 rounds=<r> nq=<nq> hits=<n_hits> chunks=<c>"; with
 * sw_bank_set_timing the rounds of a chunk are bracketed as one launch. */
#define SWBANK_HAS_DISJOINT_FRAMES 1

sw_status sw_align_disjoint_frame_hits_device(sw_bank *bank, const uint8_t *d_residues,
                                              const uint64_t *d_offsets, const uint32_t *d_lens,
                                              const uint64_t *d_ids, size_t n, uint32_t max_len,
                                              const uint8_t *codon_table, uint32_t rounds,
                                              int32_t min_score, const uint32_t *d_hit_queries,
                                              size_t hits_per_query, const uint64_t *d_hits,
                                              size_t n_hits, sw_alignment *d_out,
                                              uint32_t *d_cigar, uint32_t cigar_stride,
                                              void *stream);

sw_status sw_align_disjoint_frame_hits(sw_bank *bank, const uint8_t *residues,
                                       size_t residues_len, const uint64_t *offsets,
                                       const uint32_t *lens, const uint64_t *ids, size_t n,
                                       const uint8_t *codon_table, uint32_t rounds,
                                       int32_t min_score, const uint32_t *hit_queries,
                                       size_t hits_per_query, const uint64_t *hits, size_t n_hits,
                                       sw_alignment *out, uint32_t *cigar, size_t cigar_cap,
                                       size_t *cigar_used);

/* ---- profiling(≙ the CAPI AFU's cycle counters, capi_sample_aligner/hdl-verliog/afu.v
 *      _DEBUGGING_ "calculation #N completed, runtime: C cycles") ------------------------- */
/* When enabled, every launch is bracketed by hipEvents on the stream it runs on. */
sw_status sw_bank_set_timing(sw_bank *bank, int32_t enable);
/* Synchronises on the recorded events and returns the launches and the summed milliseconds of
 * the feeder (pack: host gather / packing time of the host-buffer calls) and of the score
 * kernels (device time) since the previous call. */
sw_status sw_bank_timing(sw_bank *bank, uint64_t *launches, double *pack_ms, double *score_ms);
/* Feeder / fallback counters since the bank was created (a multi-device bank sums its
 * devices'), so silent slow paths show: host calls that ran as one streamed kernel, streamed
 * calls re-run through the chunked feeder because a chunk's wait ran out, streamed calls
 * declined for the memory cap (SWBANK_STREAM_MB) or a failed allocation, chunked host calls,
 * device-side length sorts, multi-device gathers abandoned after their time limit, chunks
 * of chunked calls sent as mixed 2-bit / 4-bit codes (ragged DNA), and the pool parts of those
 * chunks packed as one run (targets back to back in the caller's residues), device calls
 * with balanced chunk ranges. */
typedef struct sw_counters {
  uint64_t stream_calls;
  uint64_t stream_reruns;
  uint64_t stream_declined;
  uint64_t chunked_calls;
  uint64_t device_sorts;
  uint64_t gather_timeouts;
  uint64_t mixed_chunks;
  uint64_t mixed_runs;
  /* ABI 4: device calls run with balanced chunk ranges (tiles handed between workgroups),
   * and hand-off waits that ran out (0 unless a workgroup never started) */
  uint64_t balanced_calls;
  uint64_t balanced_timeouts;
  /* ABI 5: protein-tail hand-off waits that ran out, and host-buffer calls re-run without
   * hand-offs because one did (counted when a synchronising call observed them) */
  uint64_t tail_timeouts;
  uint64_t handoff_reruns;
  /* ABI 6: hand-off waits of the protein wave kernel's balanced ranges that ran out (the
   * tile kernel's are balanced_timeouts); each kind of time-out in a call is counted once */
  uint64_t wave_balanced_timeouts;
  /* ABI 6: bytes the host-buffer calls copied host -> device (packed codes and metadata): the
   * PCIe traffic of the drop-in path */
  uint64_t h2d_bytes;
} sw_counters;
/* The first 8 counters (the ABI-3 struct, 64 bytes): safe for a caller of any ABI. */
sw_status sw_bank_counters(const sw_bank *bank, sw_counters *out);
/* out_size = sizeof(sw_counters) as the caller compiled it: 64 (ABI 3), 80 (ABI 4), 96 (ABI 5)
 * or 112 (ABI 6); any other size is SW_ERR_ARG.  No HIP call: the counts are host-side. */
sw_status sw_bank_counters_ex(const sw_bank *bank, sw_counters *out, size_t out_size);

/* Device-side failure reporting (≙ the CAPI host decoding the AFU's error bits and failing the
 * call, capi_sample_aligner/software-C,C++/src/main_test.c:64-100).  Two launch shapes hand
 * work between workgroups of one launch (balanced chunk ranges of device batches, the segmented
 * protein tail); each wait is bounded, and one that runs out marks the launch as failed instead
 * of hanging.  A host-buffer call that sees the mark re-runs itself without hand-offs
 * (handoff_reruns) and returns SW_ERR_TIMEOUT only if that fails too.  A device call is
 * asynchronous, so its mark is latched on the bank and returned (once, as SW_ERR_TIMEOUT) by
 * the next call that synchronises with it -- sw_bank_sync, sw_batch_best, sw_bank_timing -- or
 * by the next device scoring call on the bank, which then scores nothing.
 * sw_bank_sync waits for the bank's last scoring call (any stream) and returns that status. */
sw_status sw_bank_sync(sw_bank *bank);

/* Which kernel the last score call ran, e.g. "tile f16 R=32 W=4 segs=1 grid=998" or
 * "wave u16 K=4" (empty before the first call).  No reference counterpart: the RTL has one
 * datapath; this lets tests and profiles confirm the path taken. */
const char *sw_last_kernel(const sw_bank *bank);

/* ---- host-side helpers (no device needed) ---------------------------------------------- */
/* ASCII -> codes for the alphabet; returns n. */
size_t sw_encode_ascii(int32_t alphabet, const char *ascii, size_t n, uint8_t *codes);
/* ASCII DNA -> 2-bit LSB-first packing (charTo2bit); out must hold (n+3)/4 bytes, which are
 * OR-ed into (caller zeroes them, as the reference host's posix_memalign'd buffer).  */
size_t sw_pack_2bit(const char *ascii, size_t n, uint8_t *out);
/* 2-bit packed -> DNA codes (inverse of sw_pack_2bit for A/C/G/T). */
size_t sw_unpack_2bit(const uint8_t *packed, size_t n, uint8_t *codes);
/* Fill a substitution matrix: DNA (alpha 5) from match/mismatch, or BLOSUM62 (alpha 24). */
sw_status sw_fill_matrix(int32_t alphabet, int32_t match, int32_t mismatch, int8_t *matrix);
/* CIGAR ops -> text, e.g. "15M2I17M4D13M" or "20M1/20M" (SW_CIGAR_FS_SKIP prints as '/',
 * SW_CIGAR_FS_BACK as '\', any other op code past D as '?'): writes at most
 * cap - 1 characters and a NUL into buf (nothing when cap == 0; buf may then be NULL) and
 * returns the length the whole string needs, excluding the NUL. */
size_t sw_cigar_string(const uint32_t *ops, size_t n_ops, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SWBANK_H */
