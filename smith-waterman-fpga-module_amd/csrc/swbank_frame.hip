// swbank_frame.hip — the translated search (include/swbank.h "translated search", DESIGN.md
// §3.15): the ABI entries of the six-frame translation of a batch and of the frame-merged
// scores.  The kernels are in swbank_kframe.hip; the six frames of a slice of targets are scored
// in one sw_score_batch_device_range call, so kernel choice, the int32 re-score, the length sort,
// balanced ranges and multi-device dealing are what they are for a forward protein search.  The
// frame-aware alignment entries are in swbank_align.hip.
#include "swbank_bank.h"

namespace {

sw_status protein_only(sw_bank* b, const char* what) {
  if (b->cfg.alphabet != SW_ALPHABET_PROTEIN)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: protein banks only (the targets are translated)", what);
  return SW_OK;
}

sw_status table_of(sw_bank* b, const char* what, const uint8_t* codon_table, uint8_t tab[64]) {
  if (!swbank_codon_table(codon_table, tab))
    return fail(b, SW_ERR_ARG, "%s: a codon table entry is no protein code (>= %d)", what,
                SW_PROTEIN_ALPHA);
  return SW_OK;
}

// The slices of a frame call over n targets of at most max_len codes against nq queries, as a
// plan over TRANSLATED targets (slice_plan's sibling): six per target, each with its codes at
// the stride, an offset, a length and nq scores; span is a multiple of 6 and below 2^32.
sw_status frame_plan(sw_bank* b, size_t n, size_t nq, uint32_t max_len, SlicePlan& plan) {
  plan.stride = ((size_t)max_len / 3 + 15) / 16 * 16 + 16;
  const size_t per = SW_FRAME_COUNT * (plan.stride + sizeof(uint64_t) + sizeof(uint32_t) +
                                       nq * sizeof(int32_t));
  const size_t budget = (size_t)std::max(1, env_int("SWBANK_FRAME_MB", 256)) << 20;
  const size_t targets = std::min({n, std::max<size_t>(1, budget / per),
                                   (size_t)0xFFFFFFFFull / SW_FRAME_COUNT});
  plan.span = targets * SW_FRAME_COUNT;
  plan.slices = (n + targets - 1) / targets;
  return SW_OK;
}

}  // namespace

extern "C" sw_status sw_translate_batch_device(sw_bank* b, const uint8_t* d_res,
                                               const uint64_t* d_offs, const uint32_t* d_lens,
                                               size_t n, uint32_t max_len,
                                               const uint8_t* codon_table, uint8_t* d_out,
                                               size_t out_stride, uint64_t* d_out_offs,
                                               uint32_t* d_out_lens, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = protein_only(b, "sw_translate_batch_device"); st != SW_OK) return st;
  if (!d_res || !d_offs || !d_lens || !d_out || !d_out_offs || !d_out_lens)
    return fail(b, SW_ERR_ARG, "sw_translate_batch_device: null device buffer");
  if (n == 0 || n >= 0x100000000ull / SW_FRAME_COUNT)
    return fail(b, SW_ERR_ARG, "sw_translate_batch_device: 0 < 6 n < 2^32");
  if (out_stride < std::max<size_t>(max_len / 3, 1))
    return fail(b, SW_ERR_ARG, "sw_translate_batch_device: out_stride %zu < max(max_len / 3, 1)",
                out_stride);
  uint8_t tab[64];
  if (const sw_status st = table_of(b, "sw_translate_batch_device", codon_table, tab); st != SW_OK)
    return st;
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_translate_batch_device(r, d_res, d_offs, d_lens, n, max_len, codon_table, d_out,
                                         out_stride, d_out_offs, d_out_lens, s);
      }))
    return st;
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  const sw_status st = timed_on(b, hs, [&] {
    return swk_translate_batch(d_res, d_offs, d_lens, n, tab, d_out, out_stride, max_len / 3,
                               d_out_offs, d_out_lens, hs);
  });
  if (st != SW_OK) return st;
  snprintf(b->last_kernel, sizeof(b->last_kernel), "translate n=%zu", n);
  return SW_OK;
}

extern "C" sw_status sw_score_frames_device(sw_bank* b, const uint8_t* d_res,
                                            const uint64_t* d_offs, const uint32_t* d_lens,
                                            size_t n, uint32_t min_len, uint32_t max_len,
                                            const uint8_t* codon_table, int32_t* d_scores,
                                            uint8_t* d_frames, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = protein_only(b, "sw_score_frames_device"); st != SW_OK) return st;
  if (min_len > max_len) return fail(b, SW_ERR_ARG, "min_len %u > max_len %u", min_len, max_len);
  uint8_t tab[64];
  if (const sw_status st = table_of(b, "sw_score_frames_device", codon_table, tab); st != SW_OK)
    return st;
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  // a hand-off fault latched by an earlier device call is returned before anything is scored
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (n == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_scores)
    return fail(b, SW_ERR_ARG, "sw_score_frames_device: null device buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_frames_device: n < 2^32");
  const size_t nq = sw_query_count(b);
  if (n > SIZE_MAX / sizeof(int32_t) / SW_FRAME_COUNT / nq)
    return fail(b, SW_ERR_ARG, "sw_score_frames_device: nq x 6 n overflows size_t");
  HIPOK(b, hipSetDevice(r->device));
  hipStream_t hs = stream_or(r, stream);
  // a slice of targets: its six translations at a fixed stride, their offsets and lengths, and
  // the nq rows of 6 nk scores
  SlicePlan pl;
  SliceScratch& sl = r->fr_slice;
  sw_status st = frame_plan(b, n, nq, max_len, pl);
  if (st != SW_OK) return st;
  const size_t span = pl.span / SW_FRAME_COUNT;
  // the lengths of the translations: the shortest frame of the shortest target, the longest frame
  // of the longest
  const uint32_t lo = (std::max(min_len, 2u) - 2) / 3, hi = max_len / 3;
  // the previous call's use of the scratch, on whichever stream it ran
  if ((st = scratch_event(b, r->ev_frame, hs)) != SW_OK) return st;
  if ((st = slice_reserve(b, sl, pl, nq, hs)) != SW_OK) return st;
  HIPOK(b, r->fr_lens.reserve(pl.span));
  for (size_t k0 = 0; k0 < n && st == SW_OK; k0 += span) {
    const size_t nk = std::min(span, n - k0);
    st = timed_on(b, hs, [&] {
      return swk_translate_batch(d_res, d_offs + k0, d_lens + k0, nk, tab, sl.codes.p, pl.stride, hi,
                                 sl.offs.p, r->fr_lens.p, hs);
    });
    if (st != SW_OK) break;
    // all six frames in one call: the length sort and the balanced ranges see them together
    st = sw_score_batch_device_range(b, sl.codes.p, sl.offs.p, r->fr_lens.p, nullptr,
                                     SW_FRAME_COUNT * nk, lo, hi, sl.scores.p, hs);
    if (st != SW_OK) break;
    HIPOK(b, hipSetDevice(r->device));
    st = timed_on(b, hs, [&] {
      return swk_frame_merge(d_scores, sl.scores.p, d_frames, n, k0, nk, nq, hs);
    });
  }
  // whatever was launched uses the scratch: the next call is ordered after it in any case, and
  // sw_bank_sync waits for the merge
  const hipError_t er = hipEventRecord(r->ev_frame, hs);
  if (st != SW_OK) return b == r ? st : root_failed(b, r, st);
  HIPOK(b, er);
  snprintf(b->last_kernel, sizeof(b->last_kernel), "frames nq=%zu n=%zu slices=%zu", nq, n,
           pl.slices);
  return SW_OK;
}

extern "C" sw_status sw_score_frames(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                     const uint64_t* offsets, const uint32_t* lens, size_t n,
                                     const uint8_t* codon_table, int32_t* scores_out,
                                     uint8_t* frames_out) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const sw_status st = protein_only(b, "sw_score_frames"); st != SW_OK) return st;
  uint8_t tab[64];
  if (const sw_status st = table_of(b, "sw_score_frames", codon_table, tab); st != SW_OK) return st;
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  if (n == 0) return SW_OK;
  if (!offsets || !lens || !scores_out) return fail(b, SW_ERR_ARG, "sw_score_frames: null buffer");
  if (n >= 0x100000000ull) return fail(b, SW_ERR_ARG, "sw_score_frames: n < 2^32");
  const size_t nq = sw_query_count(b);
  if (n > SIZE_MAX / sizeof(int32_t) / SW_FRAME_COUNT / nq)
    return fail(b, SW_ERR_ARG, "sw_score_frames: nq x 6 n overflows size_t");
  // the previous call (on any stream) is done with the buffers before they are refilled.  The
  // batch holds DNA codes, which the staging (it knows the bank's protein alphabet) cannot
  // check: checked here, after the staging has placed every target inside the residues
  uint32_t lo, hi;
  StagedBatch& sb = r->fr_host;
  sw_status st = stage_host_batch(b, sb, residues, residues_len, offsets, lens, n, nullptr, false,
                                  r->ev_frame, lo, hi);
  hipStream_t hs = r->stream;
  for (size_t k = 0; k < n && st == SW_OK; ++k) {
    if (lens[k] && !residues) st = fail(b, SW_ERR_ARG, "sw_score_frames: null residues");
    for (uint32_t i = 0; i < lens[k] && st == SW_OK; ++i)
      if (residues[offsets[k] + i] >= SW_DNA_ALPHA)
        st = fail(b, SW_ERR_ARG, "target %zu code %u at %u is no DNA code", k,
                  residues[offsets[k] + i], i);
  }
  hipError_t e = hipSuccess;
  if (st == SW_OK) e = r->fr_hsc.reserve(nq * n);
  if (st == SW_OK && e == hipSuccess && frames_out) e = r->fr_hfr.reserve(nq * n);
  if (st == SW_OK && e == hipSuccess)
    st = sw_score_frames_device(b, sb.res.p, sb.offs.p, sb.lens.p, n, lo, hi, codon_table,
                                r->fr_hsc.p, frames_out ? r->fr_hfr.p : nullptr, hs);
  if (st != SW_OK || e != hipSuccess) {
    (void)hipStreamSynchronize(hs);  // (the uploads have left the caller's buffers)
    HIPOK(b, e);
    return st;
  }
  HIPOK(b, hipSetDevice(r->device));
  HIPOK(b, hipMemcpyAsync(scores_out, r->fr_hsc.p, nq * n * sizeof(int32_t), hipMemcpyDeviceToHost,
                          hs));
  if (frames_out)
    HIPOK(b, hipMemcpyAsync(frames_out, r->fr_hfr.p, nq * n, hipMemcpyDeviceToHost, hs));
  HIPOK(b, hipEventRecord(r->ev_frame, hs));  // (the copies read the result buffers)
  HIPOK(b, hipStreamSynchronize(hs));
  // the scoring pass's hand-off faults: the scores are invalid
  return take_fault(b, 0);
}
