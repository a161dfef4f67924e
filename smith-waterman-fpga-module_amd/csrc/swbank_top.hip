// swbank_top.hip — the k best hits of every row of a score matrix (include/swbank.h "the k best
// hits") and the best query of every column ("the best query per target",
// §3.11): the ABI entries.  The kernels are in swbank_ktop.hip and swbank_kbestq.hip.
#include "swbank_bank.h"

namespace {

// The arguments both entries refuse; nullptr when they are fine.
const char* bad_args(const void* scores, const void* hits, size_t n, size_t nq, size_t k) {
  if (!scores || !hits) return "null scores or hits";
  if (n == 0 || nq == 0 || k == 0) return "n, nq and k must be positive";
  if (k > SW_TOP_MAX_K) return "k > SW_TOP_MAX_K";
  if (n > 0x100000000ull) return "a row holds <= 2^32 scores";
  if (n > SIZE_MAX / nq || k > SIZE_MAX / nq) return "nq x n or nq x k overflows size_t";
  if (nq > SIZE_MAX / (swk_top_state_words() * sizeof(unsigned long long)))
    return "nq overflows the select's state";
  return nullptr;
}

// The selection on `hs`, ordered after the previous call's use of the bank's scratch (ev_top).
sw_status select_on(sw_bank* b, const int32_t* d_scores, const uint64_t* d_ids, size_t n, size_t nq,
                    size_t k, int32_t min_score, uint64_t* d_hits, int32_t* d_hit_scores,
                    uint64_t* d_hit_ids, uint32_t* d_counts, hipStream_t hs) {
  HIPOK(b, b->top_state.reserve(nq * swk_top_state_words()));
  HIPOK(b, b->top_keys.reserve(nq * k));
  sw_status st = scratch_event(b, b->ev_top, hs);
  if (st != SW_OK) return st;
  st = timed_on(b, hs, [&] {
    const hipError_t e = swk_top_hits(d_scores, d_ids, n, nq, k, min_score, b->top_state.p,
                                      b->top_keys.p, d_hits, d_hit_scores, d_hit_ids, d_counts, hs);
    // whatever was launched uses the scratch: the next call is ordered after it in any case
    const hipError_t er = hipEventRecord(b->ev_top, hs);
    return e != hipSuccess ? e : er;
  });
  if (st != SW_OK) return st;
  snprintf(b->last_kernel, sizeof(b->last_kernel), "top k=%zu nq=%zu n=%zu", k, nq, n);
  return SW_OK;
}

// ---- the best query of every column ---------------------------------------------------------
const char* bad_best_args(const void* scores, const void* bq, const void* bs, size_t n, size_t nq) {
  if (!scores || (!bq && !bs)) return "null scores, or neither output given";
  if (n == 0 || nq == 0) return "n and nq must be positive";
  if (nq > 65536) return "nq > 65536 (the limit of sw_load_queries)";
  if (n > 0x100000000ull) return "a row holds <= 2^32 scores";
  if (n > SIZE_MAX / sizeof(int32_t) / nq) return "nq x n overflows size_t";
  return nullptr;
}

// The column best on `hs`, ordered after the previous use of the scratch it shares with the
// top-hits calls (ev_top).
sw_status best_queries_on(sw_bank* b, const int32_t* d_scores, size_t n, size_t nq,
                          int32_t min_score, uint32_t* d_best_query, int32_t* d_best_score,
                          hipStream_t hs) {
  const size_t nkeys = swk_best_queries_keys(n, nq);
  if (nkeys) HIPOK(b, b->top_keys.reserve(nkeys));
  sw_status st = scratch_event(b, b->ev_top, hs);
  if (st != SW_OK) return st;
  st = timed_on(b, hs, [&] {
    const hipError_t e = swk_best_queries(d_scores, n, nq, min_score,
                                          nkeys ? b->top_keys.p : nullptr, d_best_query,
                                          d_best_score, hs);
    const hipError_t er = hipEventRecord(b->ev_top, hs);  // (as in select_on)
    return e != hipSuccess ? e : er;
  });
  if (st != SW_OK) return st;
  snprintf(b->last_kernel, sizeof(b->last_kernel), "best-query nq=%zu n=%zu", nq, n);
  return SW_OK;
}

}  // namespace

extern "C" sw_status sw_best_queries_device(sw_bank* b, const int32_t* d_scores, size_t n,
                                            size_t nq, int32_t min_score, uint32_t* d_best_query,
                                            int32_t* d_best_score, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const char* why = bad_best_args(d_scores, d_best_query, d_best_score, n, nq))
    return fail(b, SW_ERR_ARG, "sw_best_queries_device: %s", why);
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_best_queries_device(r, d_scores, n, nq, min_score, d_best_query, d_best_score, s);
      }))
    return st;
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  return best_queries_on(b, d_scores, n, nq, min_score, d_best_query, d_best_score,
                         stream_or(b, stream));
}

extern "C" sw_status sw_best_queries(sw_bank* b, const int32_t* scores, size_t n, size_t nq,
                                     int32_t min_score, uint32_t* best_query,
                                     int32_t* best_score) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const char* why = bad_best_args(scores, best_query, best_score, n, nq))
    return fail(b, SW_ERR_ARG, "sw_best_queries: %s", why);
  if (sw_status st; on_root(b, nullptr, st, [&](sw_bank* r, void*) {
        return sw_best_queries(r, scores, n, nq, min_score, best_query, best_score);
      }))
    return st;
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = b->stream;
  // the previous call (on any stream) is done with the buffers before they are refilled
  if (b->ev_top) HIPOK(b, hipStreamWaitEvent(hs, b->ev_top, 0));
  HIPOK(b, b->top_scores.reserve(nq * n));
  if (best_query) HIPOK(b, b->top_cnt.reserve(n));
  if (best_score) HIPOK(b, b->top_hsc.reserve(n));
  HIPOK(b, hipMemcpyAsync(b->top_scores.p, scores, nq * n * sizeof(int32_t),
                          hipMemcpyHostToDevice, hs));
  const sw_status st = best_queries_on(b, b->top_scores.p, n, nq, min_score,
                                       best_query ? b->top_cnt.p : nullptr,
                                       best_score ? b->top_hsc.p : nullptr, hs);
  if (st != SW_OK) return st;
  if (best_query)
    HIPOK(b, hipMemcpyAsync(best_query, b->top_cnt.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            hs));
  if (best_score)
    HIPOK(b, hipMemcpyAsync(best_score, b->top_hsc.p, n * sizeof(int32_t), hipMemcpyDeviceToHost,
                            hs));
  HIPOK(b, hipEventRecord(b->ev_top, hs));  // (the copies read the result buffers)
  HIPOK(b, hipStreamSynchronize(hs));
  return SW_OK;
}

extern "C" sw_status sw_top_hits_device(sw_bank* b, const int32_t* d_scores, const uint64_t* d_ids,
                                        size_t n, size_t nq, size_t k, int32_t min_score,
                                        uint64_t* d_hits, int32_t* d_hit_scores,
                                        uint64_t* d_hit_ids, uint32_t* d_counts, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const char* why = bad_args(d_scores, d_hits, n, nq, k))
    return fail(b, SW_ERR_ARG, "sw_top_hits_device: %s", why);
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_top_hits_device(r, d_scores, d_ids, n, nq, k, min_score, d_hits, d_hit_scores,
                                  d_hit_ids, d_counts, s);
      }))
    return st;
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  return select_on(b, d_scores, d_ids, n, nq, k, min_score, d_hits, d_hit_scores, d_hit_ids,
                   d_counts, stream_or(b, stream));
}

extern "C" sw_status sw_top_hits(sw_bank* b, const int32_t* scores, const uint64_t* ids, size_t n,
                                 size_t nq, size_t k, int32_t min_score, uint64_t* hits,
                                 int32_t* hit_scores, uint64_t* hit_ids, uint32_t* counts) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const char* why = bad_args(scores, hits, n, nq, k))
    return fail(b, SW_ERR_ARG, "sw_top_hits: %s", why);
  if (nq > SIZE_MAX / sizeof(uint64_t) / std::max(n, k))
    return fail(b, SW_ERR_ARG, "sw_top_hits: nq x n or nq x k bytes overflow size_t");
  if (sw_status st; on_root(b, nullptr, st, [&](sw_bank* r, void*) {
        return sw_top_hits(r, scores, ids, n, nq, k, min_score, hits, hit_scores, hit_ids, counts);
      }))
    return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = b->stream;
  // the previous call (on any stream) is done with the buffers before they are refilled
  if (b->ev_top) HIPOK(b, hipStreamWaitEvent(hs, b->ev_top, 0));
  HIPOK(b, b->top_scores.reserve(nq * n));
  HIPOK(b, b->top_hits.reserve(nq * k));
  if (hit_scores) HIPOK(b, b->top_hsc.reserve(nq * k));
  if (counts) HIPOK(b, b->top_cnt.reserve(nq));
  HIPOK(b, hipMemcpyAsync(b->top_scores.p, scores, nq * n * sizeof(int32_t),
                          hipMemcpyHostToDevice, hs));
  const sw_status st =
      select_on(b, b->top_scores.p, nullptr, n, nq, k, min_score, b->top_hits.p,
                hit_scores ? b->top_hsc.p : nullptr, nullptr, counts ? b->top_cnt.p : nullptr, hs);
  if (st != SW_OK) return st;
  HIPOK(b, hipMemcpyAsync(hits, b->top_hits.p, nq * k * sizeof(uint64_t), hipMemcpyDeviceToHost,
                          hs));
  if (hit_scores)
    HIPOK(b, hipMemcpyAsync(hit_scores, b->top_hsc.p, nq * k * sizeof(int32_t),
                            hipMemcpyDeviceToHost, hs));
  if (counts)
    HIPOK(b, hipMemcpyAsync(counts, b->top_cnt.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            hs));
  HIPOK(b, hipEventRecord(b->ev_top, hs));  // (the copies read the result buffers)
  HIPOK(b, hipStreamSynchronize(hs));
  if (hit_ids)
    for (size_t i = 0; i < nq * k; ++i)
      hit_ids[i] = hits[i] == SW_HIT_NONE ? SW_HIT_NONE : ids ? ids[hits[i]] : hits[i];
  return SW_OK;
}
