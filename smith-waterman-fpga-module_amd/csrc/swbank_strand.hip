// swbank_strand.hip — both DNA strands (include/swbank.h "both DNA strands"):
// the ABI entries of the reverse complement of a batch and of the strand-merged scores.  The
// kernels are in swbank_kstrand.hip; each strand is scored by the bank's own
// sw_score_batch_device_range, so kernel choice, the int32 re-score, balanced ranges and
// multi-device dealing are what they are for a forward search.  The strand-aware alignment
// entries are in swbank_align.hip.
#include "swbank_bank.h"

namespace {

sw_status dna_only(sw_bank* b, const char* what) {
  if (b->cfg.alphabet != SW_ALPHABET_DNA)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: DNA banks only (a protein has no reverse strand)", what);
  return SW_OK;
}

}  // namespace

extern "C" sw_status sw_revcomp_batch_device(sw_bank* b, const uint8_t* d_res,
                                             const uint64_t* d_offs, const uint32_t* d_lens,
                                             size_t n, uint8_t* d_out, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = dna_only(b, "sw_revcomp_batch_device"); st != SW_OK) return st;
  if (!d_res || !d_offs || !d_lens || !d_out)
    return fail(b, SW_ERR_ARG, "sw_revcomp_batch_device: null device buffer");
  if (n == 0 || n >= 0x100000000ull)
    return fail(b, SW_ERR_ARG, "sw_revcomp_batch_device: 0 < n < 2^32");
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_revcomp_batch_device(r, d_res, d_offs, d_lens, n, d_out, s);
      }))
    return st;
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  const sw_status st = timed_on(b, hs, [&] {
    return swk_revcomp_batch(d_res, d_offs, d_lens, n, d_out, nullptr, 0, hs);
  });
  if (st != SW_OK) return st;
  snprintf(b->last_kernel, sizeof(b->last_kernel), "revcomp n=%zu", n);
  return SW_OK;
}

extern "C" sw_status sw_score_strands_device(sw_bank* b, const uint8_t* d_res, const uint8_t* d_rc,
                                             const uint64_t* d_offs, const uint32_t* d_lens,
                                             size_t n, uint32_t min_len, uint32_t max_len,
                                             int32_t* d_scores, uint8_t* d_strands, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = dna_only(b, "sw_score_strands_device"); st != SW_OK) return st;
  if (min_len > max_len) return fail(b, SW_ERR_ARG, "min_len %u > max_len %u", min_len, max_len);
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  // a hand-off fault latched by an earlier device call is returned before anything is scored
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (n == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_scores)
    return fail(b, SW_ERR_ARG, "sw_score_strands_device: null device buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_strands_device: n < 2^32");
  const size_t nq = sw_query_count(b);
  if (n > SIZE_MAX / sizeof(int32_t) / nq)
    return fail(b, SW_ERR_ARG, "sw_score_strands_device: nq x n overflows size_t");
  HIPOK(b, hipSetDevice(r->device));
  hipStream_t hs = stream_or(r, stream);
  // a slice of targets: its reverse-strand scores and, without the caller's d_rc, its reverse
  // complement at a fixed stride and the offsets of that
  SlicePlan pl;
  SliceScratch& sl = r->str_slice;
  sw_status st = slice_plan(b, "SWBANK_STRAND_MB", n, nq, max_len, !d_rc, pl);
  if (st != SW_OK) return st;
  const size_t span = pl.span;
  // the forward strand, the whole batch, straight into the caller's matrix
  st = sw_score_batch_device_range(b, d_res, d_offs, d_lens, nullptr, n, min_len, max_len, d_scores,
                                   hs);
  if (st != SW_OK) return st;
  HIPOK(b, hipSetDevice(r->device));
  // the previous call's use of the scratch, on whichever stream it ran
  if ((st = scratch_event(b, r->ev_strand, hs)) != SW_OK) return st;
  if ((st = slice_reserve(b, sl, pl, nq, hs)) != SW_OK) return st;
  for (size_t k0 = 0; k0 < n && st == SW_OK; k0 += span) {
    const size_t nk = std::min(span, n - k0);
    const uint8_t* res = d_rc;
    const uint64_t* offs = d_offs + k0;
    if (!d_rc) {
      st = timed_on(b, hs, [&] {
        return swk_revcomp_batch(d_res, d_offs + k0, d_lens + k0, nk, sl.codes.p, sl.offs.p,
                                 (uint32_t)pl.stride, hs);
      });
      if (st != SW_OK) break;
      res = sl.codes.p;
      offs = sl.offs.p;
    }
    st = sw_score_batch_device_range(b, res, offs, d_lens + k0, nullptr, nk, min_len, max_len,
                                     sl.scores.p, hs);
    if (st != SW_OK) break;
    HIPOK(b, hipSetDevice(r->device));
    st = timed_on(b, hs, [&] {
      return swk_strand_merge(d_scores, sl.scores.p, d_strands, n, k0, nk, nq, hs);
    });
  }
  // whatever was launched uses the scratch: the next call is ordered after it in any case, and
  // sw_bank_sync waits for the merge
  const hipError_t er = hipEventRecord(r->ev_strand, hs);
  if (st != SW_OK) return b == r ? st : root_failed(b, r, st);
  HIPOK(b, er);
  snprintf(b->last_kernel, sizeof(b->last_kernel), "strands nq=%zu n=%zu slices=%zu", nq, n,
           pl.slices);
  return SW_OK;
}

extern "C" sw_status sw_score_strands(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                      const uint64_t* offsets, const uint32_t* lens, size_t n,
                                      int32_t* scores_out, uint8_t* strands_out) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = dna_only(b, "sw_score_strands"); st != SW_OK) return st;
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  if (n == 0) return SW_OK;
  if (!offsets || !lens || !scores_out)
    return fail(b, SW_ERR_ARG, "sw_score_strands: null buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_strands: n < 2^32");
  const size_t nq = sw_query_count(b);
  if (n > SIZE_MAX / sizeof(int32_t) / nq)
    return fail(b, SW_ERR_ARG, "sw_score_strands: nq x n overflows size_t");
  // the previous call (on any stream) is done with the buffers before they are refilled; the
  // codes zeroed like a caller's padded batch: what a score kernel reads past the last target's
  // end is a code of the alphabet
  uint32_t lo, hi;
  StagedBatch& sb = r->str_host;
  sw_status st = stage_host_batch(b, sb, residues, residues_len, offsets, lens, n,
                                  "sw_score_strands", true, r->ev_strand, lo, hi);
  if (st != SW_OK) return st;
  hipStream_t hs = r->stream;
  hipError_t e = r->str_hsc.reserve(nq * n);
  if (e == hipSuccess && strands_out) e = r->str_hstr.reserve(nq * n);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(hs);  // (the uploads have left the caller's buffers)
    HIPOK(b, e);
  }
  st = sw_score_strands_device(b, sb.res.p, nullptr, sb.offs.p, sb.lens.p, n, lo, hi, r->str_hsc.p,
                               strands_out ? r->str_hstr.p : nullptr, hs);
  if (st != SW_OK) {
    (void)hipStreamSynchronize(hs);  // (the uploads have left the caller's buffers)
    return st;
  }
  HIPOK(b, hipSetDevice(r->device));
  HIPOK(b, hipMemcpyAsync(scores_out, r->str_hsc.p, nq * n * sizeof(int32_t), hipMemcpyDeviceToHost,
                          hs));
  if (strands_out)
    HIPOK(b, hipMemcpyAsync(strands_out, r->str_hstr.p, nq * n, hipMemcpyDeviceToHost, hs));
  HIPOK(b, hipEventRecord(r->ev_strand, hs));  // (the copies read the result buffers)
  HIPOK(b, hipStreamSynchronize(hs));
  // the scoring passes' hand-off faults: the scores are invalid
  return take_fault(b, 0);
}
