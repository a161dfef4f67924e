// swbank_glocal.hip — the global-local search (include/swbank.h "global-local search", DESIGN.md
// §3.17): the ABI entries.  The kernel is in swbank_kglocal.hip; like the frameshift search's it
// reads the batch as it lies (no reverse complement is made) and builds its query profiles from
// the alignment unit's table of the queries' codes and the matrix (prepare_align), so the call
// owns no device scratch: it waits for the table upload (ev_ready) and is followed by ev_used
// like every launch that reads query tables.  The host form stages its batch and results in the
// frame search's host buffers and its end positions in gl_hend (both calls synchronise).
#include "swbank_bank.h"

// What both entries (and the aligner's, swbank_align.hip) check before anything else, in the
// order of the header's list.
sw_status glocal_opening(sw_bank* b, const char* what, int32_t ends, int32_t both_strands) {
  if (both_strands && b->cfg.alphabet != SW_ALPHABET_DNA)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: both_strands on DNA banks only", what);
  if (!b->gotoh())
    return fail(b, SW_ERR_UNSUPPORTED, "%s: the Gotoh gap model only", what);
  if (ends < SW_ENDS_QUERY || ends > SW_ENDS_BOTH)
    return fail(b, SW_ERR_ARG, "%s: ends is SW_ENDS_QUERY, _TARGET or _BOTH (got %d)", what, ends);
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  if (b->query.size() > SW_GLOCAL_MAX_QUERY)  // (a set: its longest query)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: a query of %zu rows (at most %d)", what,
                b->query.size(), SW_GLOCAL_MAX_QUERY);
  return SW_OK;
}

// The range rule of the header: no cell, pad rows and lanes past the target included, leaves int32.
bool glocal_in_range(const sw_bank* b, uint32_t max_len) {
  const int64_t o = std::llabs((int64_t)b->gap_open + b->gap_extend);
  const int64_t e = std::max<int64_t>(std::llabs((int64_t)b->gap_extend), 128);
  return o + (SW_GLOCAL_MAX_QUERY + 64 + (int64_t)max_len) * e < ((int64_t)1 << 30);
}

extern "C" sw_status sw_score_glocal_device(sw_bank* b, const uint8_t* d_res,
                                            const uint64_t* d_offs, const uint32_t* d_lens,
                                            size_t n, uint32_t max_len, int32_t ends,
                                            int32_t both_strands, int32_t* d_scores,
                                            uint32_t* d_end_pos, uint8_t* d_strands,
                                            void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = glocal_opening(b, "sw_score_glocal_device", ends, both_strands);
      st != SW_OK)
    return st;
  // a hand-off fault latched by an earlier device call is returned before anything is scored
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (n == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_scores)
    return fail(b, SW_ERR_ARG, "sw_score_glocal_device: null device buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_glocal_device: n < 2^32");
  if (n > SIZE_MAX / sizeof(int32_t) / sw_query_count(b))
    return fail(b, SW_ERR_ARG, "sw_score_glocal_device: nq x n overflows size_t");
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_score_glocal_device(r, d_res, d_offs, d_lens, n, max_len, ends, both_strands,
                                      d_scores, d_end_pos, d_strands, s);
      }))
    return st;
  sw_status st = prepare(b);
  if (st != SW_OK) return st;
  if (!glocal_in_range(b, max_len))
    return fail(b, SW_ERR_RANGE,
                "sw_score_glocal_device: |open + extend| + (%d + 64 + max_len %u) x "
                "max(|extend|, 128) reaches 2^30",
                SW_GLOCAL_MAX_QUERY, max_len);
  if ((size_t)b->alpha * b->alpha != b->matrix.size() || b->alpha > SW_PROTEIN_ALPHA)
    return fail(b, SW_ERR_UNSUPPORTED, "sw_score_glocal_device: alphabet %d too large", b->alpha);
  if ((st = prepare_align(b)) != SW_OK) return st;
  const size_t nq = sw_query_count(b);
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  st = timed_on(b, hs, [&] {
    return swk_glocal_score(
        d_res, d_offs, d_lens, n, max_len, reinterpret_cast<const uint2*>(b->al_tab.p),
        reinterpret_cast<const int8_t*>(b->al_tab.p + nq * sizeof(uint2)),
        b->al_tab.p + nq * sizeof(uint2) + b->matrix.size(), nq, (uint32_t)b->query.size(),
        (uint32_t)b->alpha, b->gap_open + b->gap_extend, b->gap_extend, ends, both_strands,
        d_scores, d_end_pos, d_strands, hs);
  });
  // whatever was launched reads the table: the next upload is ordered after it in any case
  const hipError_t er = hipEventRecord(b->ev_used, hs);
  if (st != SW_OK) return st;
  HIPOK(b, er);
  b->best_kind = 0;  // no best hit is tracked
  snprintf(b->last_kernel, sizeof(b->last_kernel), "glocal ends=%d nq=%zu n=%zu", ends, nq, n);
  return SW_OK;
}

extern "C" sw_status sw_score_glocal(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                     const uint64_t* offsets, const uint32_t* lens, size_t n,
                                     int32_t ends, int32_t both_strands, int32_t* scores_out,
                                     uint32_t* end_pos_out, uint8_t* strands_out) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = glocal_opening(b, "sw_score_glocal", ends, both_strands); st != SW_OK)
    return st;
  if (n == 0) return SW_OK;
  if (!offsets || !lens || !scores_out) return fail(b, SW_ERR_ARG, "sw_score_glocal: null buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_glocal: n < 2^32");
  const size_t nq = sw_query_count(b);
  if (n > SIZE_MAX / sizeof(int32_t) / nq)
    return fail(b, SW_ERR_ARG, "sw_score_glocal: nq x n overflows size_t");
  // the previous call (on any stream) is done with the buffers before they are refilled; the
  // staging checks every code against the bank's alphabet, which is the batch's
  sw_bank* r = root_of(b);
  uint32_t lo, hi;
  StagedBatch& sb = r->fr_host;
  sw_status st = stage_host_batch(b, sb, residues, residues_len, offsets, lens, n,
                                  "sw_score_glocal", false, r->ev_frame, lo, hi);
  if (st != SW_OK) return st;  // (refused before any upload)
  hipStream_t hs = r->stream;
  hipError_t e = r->fr_hsc.reserve(nq * n);
  if (e == hipSuccess && end_pos_out) e = r->gl_hend.reserve(nq * n);
  if (e == hipSuccess && strands_out) e = r->fr_hfr.reserve(nq * n);
  if (e == hipSuccess)
    st = sw_score_glocal_device(b, sb.res.p, sb.offs.p, sb.lens.p, n, hi, ends, both_strands,
                                r->fr_hsc.p, end_pos_out ? r->gl_hend.p : nullptr,
                                strands_out ? r->fr_hfr.p : nullptr, hs);
  if (st != SW_OK || e != hipSuccess) {
    (void)hipStreamSynchronize(hs);  // (the uploads have left the caller's buffers)
    HIPOK(b, e);
    return st;
  }
  HIPOK(b, hipSetDevice(r->device));
  HIPOK(b, hipMemcpyAsync(scores_out, r->fr_hsc.p, nq * n * sizeof(int32_t), hipMemcpyDeviceToHost,
                          hs));
  if (end_pos_out)
    HIPOK(b, hipMemcpyAsync(end_pos_out, r->gl_hend.p, nq * n * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, hs));
  if (strands_out)
    HIPOK(b, hipMemcpyAsync(strands_out, r->fr_hfr.p, nq * n, hipMemcpyDeviceToHost, hs));
  if (!r->ev_frame) HIPOK(b, hipEventCreateWithFlags(&r->ev_frame, hipEventDisableTiming));
  HIPOK(b, hipEventRecord(r->ev_frame, hs));  // (the copies read the result buffers)
  HIPOK(b, hipStreamSynchronize(hs));
  return take_fault(b, 0);
}
