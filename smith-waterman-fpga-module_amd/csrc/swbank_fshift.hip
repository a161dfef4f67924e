// swbank_fshift.hip — the frameshift-tolerant translated search (include/swbank.h
// "frameshift-tolerant translated search"): the ABI entries.  The kernel is in
// swbank_kfshift.hip; it reads the DNA batch as it lies (no translation, no reverse complement is
// made) and builds its query profiles from the alignment unit's table of the queries' codes and
// the matrix (prepare_align), so the call owns no device scratch: it waits for the table upload
// (ev_ready) and is followed by ev_used like every launch that reads query tables.  The host form
// stages its batch and results in the frame search's host buffers (both calls synchronise).
#include "swbank_bank.h"

// What every frameshift entry (the alignments of swbank_align.hip too) checks before anything
// else, in the order of the header's list.
sw_status fshift_opening(sw_bank* b, const char* what, const uint8_t* codon_table,
                         int32_t frameshift, uint8_t tab[64]) {
  if (b->cfg.alphabet != SW_ALPHABET_PROTEIN)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: protein banks only (the targets are translated)", what);
  if (!b->gotoh())
    return fail(b, SW_ERR_UNSUPPORTED, "%s: the Gotoh gap model only", what);
  if (frameshift > 0 || frameshift < -32767)
    return fail(b, SW_ERR_ARG, "%s: 0 >= frameshift >= -32767 (got %d)", what, frameshift);
  if (!swbank_codon_table(codon_table, tab))
    return fail(b, SW_ERR_ARG, "%s: a codon table entry is no protein code (>= %d)", what,
                SW_PROTEIN_ALPHA);
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  if (b->query.size() > SW_FSHIFT_MAX_QUERY)  // (a set: its longest query)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: a query of %zu rows (at most %d)", what,
                b->query.size(), SW_FSHIFT_MAX_QUERY);
  return SW_OK;
}

extern "C" sw_status sw_score_fshift_device(sw_bank* b, const uint8_t* d_res,
                                            const uint64_t* d_offs, const uint32_t* d_lens,
                                            size_t n, uint32_t max_len, const uint8_t* codon_table,
                                            int32_t frameshift, int32_t* d_scores,
                                            uint8_t* d_strands, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  uint8_t tab[64];
  if (const sw_status st = fshift_opening(b, "sw_score_fshift_device", codon_table, frameshift, tab);
      st != SW_OK)
    return st;
  // a hand-off fault latched by an earlier device call is returned before anything is scored
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (n == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_scores)
    return fail(b, SW_ERR_ARG, "sw_score_fshift_device: null device buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_fshift_device: n < 2^32");
  if (n > SIZE_MAX / sizeof(int32_t) / sw_query_count(b))
    return fail(b, SW_ERR_ARG, "sw_score_fshift_device: nq x n overflows size_t");
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_score_fshift_device(r, d_res, d_offs, d_lens, n, max_len, codon_table,
                                      frameshift, d_scores, d_strands, s);
      }))
    return st;
  sw_status st = prepare(b);
  if (st != SW_OK) return st;
  if ((size_t)b->alpha * b->alpha != b->matrix.size() || b->alpha > SW_PROTEIN_ALPHA)
    return fail(b, SW_ERR_UNSUPPORTED, "sw_score_fshift_device: alphabet %d too large", b->alpha);
  if ((st = prepare_align(b)) != SW_OK) return st;
  const size_t nq = sw_query_count(b);
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  st = timed_on(b, hs, [&] {
    return swk_fshift_score(
        d_res, d_offs, d_lens, n, max_len, reinterpret_cast<const uint2*>(b->al_tab.p),
        reinterpret_cast<const int8_t*>(b->al_tab.p + nq * sizeof(uint2)),
        b->al_tab.p + nq * sizeof(uint2) + b->matrix.size(), nq, (uint32_t)b->query.size(),
        (uint32_t)b->alpha, tab, b->gap_open + b->gap_extend, b->gap_extend, frameshift, d_scores,
        d_strands, hs);
  });
  // whatever was launched reads the table: the next upload is ordered after it in any case
  const hipError_t er = hipEventRecord(b->ev_used, hs);
  if (st != SW_OK) return st;
  HIPOK(b, er);
  b->best_kind = 0;  // no best hit is tracked
  snprintf(b->last_kernel, sizeof(b->last_kernel), "fshift nq=%zu n=%zu", nq, n);
  return SW_OK;
}

extern "C" sw_status sw_score_fshift(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                     const uint64_t* offsets, const uint32_t* lens, size_t n,
                                     const uint8_t* codon_table, int32_t frameshift,
                                     int32_t* scores_out, uint8_t* strands_out) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  uint8_t tab[64];
  if (const sw_status st = fshift_opening(b, "sw_score_fshift", codon_table, frameshift, tab);
      st != SW_OK)
    return st;
  if (n == 0) return SW_OK;
  if (!offsets || !lens || !scores_out) return fail(b, SW_ERR_ARG, "sw_score_fshift: null buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_fshift: n < 2^32");
  const size_t nq = sw_query_count(b);
  if (n > SIZE_MAX / sizeof(int32_t) / nq)
    return fail(b, SW_ERR_ARG, "sw_score_fshift: nq x n overflows size_t");
  // the previous call (on any stream) is done with the buffers before they are refilled.  The
  // batch holds DNA codes, which the staging (it knows the bank's protein alphabet) cannot
  // check: checked here, after the staging has placed every target inside the residues
  sw_bank* r = root_of(b);
  uint32_t lo, hi;
  StagedBatch& sb = r->fr_host;
  sw_status st = stage_host_batch(b, sb, residues, residues_len, offsets, lens, n, nullptr, false,
                                  r->ev_frame, lo, hi);
  hipStream_t hs = r->stream;
  for (size_t k = 0; k < n && st == SW_OK; ++k) {
    if (lens[k] && !residues) st = fail(b, SW_ERR_ARG, "sw_score_fshift: null residues");
    for (uint32_t i = 0; i < lens[k] && st == SW_OK; ++i)
      if (residues[offsets[k] + i] >= SW_DNA_ALPHA)
        st = fail(b, SW_ERR_ARG, "target %zu code %u at %u is no DNA code", k,
                  residues[offsets[k] + i], i);
  }
  hipError_t e = hipSuccess;
  if (st == SW_OK) e = r->fr_hsc.reserve(nq * n);
  if (st == SW_OK && e == hipSuccess && strands_out) e = r->fr_hfr.reserve(nq * n);
  if (st == SW_OK && e == hipSuccess)
    st = sw_score_fshift_device(b, sb.res.p, sb.offs.p, sb.lens.p, n, hi, codon_table, frameshift,
                                r->fr_hsc.p, strands_out ? r->fr_hfr.p : nullptr, hs);
  if (st != SW_OK || e != hipSuccess) {
    (void)hipStreamSynchronize(hs);  // (the uploads have left the caller's buffers)
    HIPOK(b, e);
    return st;
  }
  HIPOK(b, hipSetDevice(r->device));
  HIPOK(b, hipMemcpyAsync(scores_out, r->fr_hsc.p, nq * n * sizeof(int32_t), hipMemcpyDeviceToHost,
                          hs));
  if (strands_out)
    HIPOK(b, hipMemcpyAsync(strands_out, r->fr_hfr.p, nq * n, hipMemcpyDeviceToHost, hs));
  if (!r->ev_frame) HIPOK(b, hipEventCreateWithFlags(&r->ev_frame, hipEventDisableTiming));
  HIPOK(b, hipEventRecord(r->ev_frame, hs));  // (the copies read the result buffers)
  HIPOK(b, hipStreamSynchronize(hs));
  return take_fault(b, 0);
}
