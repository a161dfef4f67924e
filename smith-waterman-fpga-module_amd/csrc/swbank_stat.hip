// swbank_stat.hip — hit statistics (include/swbank.h "hit significance"): the
// ABI entries of the seeded shuffle, the score / length histogram, the estimate (shuffle ->
// score -> histogram per round, then the host fit of swbank_host.c) and the significance of a
// hit list.  The kernels are in swbank_kstat.hip; the scoring pass is the bank's own
// sw_score_batch_device_range, and swbank_kfshift.hip's kernel for the estimate of the
// frameshift-tolerant translated search.
#include "swbank_bank.h"

namespace {

const char* bad_hist_args(const void* scores, const void* counts, size_t n, size_t nq) {
  if (!scores || !counts) return "null scores or counts";
  if (n == 0 || nq == 0) return "n and nq must be positive";
  if (n > 0x100000000ull) return "a row holds <= 2^32 scores";
  if (n > SIZE_MAX / sizeof(int32_t) / nq) return "nq x n overflows size_t";
  if (nq > SIZE_MAX / (SW_STAT_BINS * sizeof(uint64_t))) return "nq x SW_STAT_BINS overflows size_t";
  return nullptr;
}

bool degenerate(const sw_statistics& s) {
  return (s.flags & SW_STAT_DEGENERATE) || !(s.lambda > 0.0) || !(s.K > 0.0);
}

// The estimates' last step: `host` holds nq rows of counts, nq rows of length sums and nq
// clamped counters; row i is fitted with the length of query i of `src` (the root of a
// multi-device bank holds the queries) into out[i].
sw_status fit_rows(sw_bank* b, const sw_bank* src, const std::vector<unsigned long long>& host,
                   size_t nq, sw_statistics* out) {
  const size_t row = (size_t)SW_STAT_BINS;
  for (size_t i = 0; i < nq; ++i) {
    const size_t qlen = src->qset.size() > 1 ? src->qset[i].size() : src->query.size();
    const sw_status st = sw_fit_statistics(reinterpret_cast<const uint64_t*>(host.data() + i * row),
                                           reinterpret_cast<const uint64_t*>(host.data() + (nq + i) * row),
                                           (uint32_t)qlen, &out[i]);
    if (st != SW_OK) return fail(b, st, "sw_fit_statistics failed for query %zu", i);
    out[i].n_clamped = host[2 * nq * row + i];
    if (out[i].n_clamped) out[i].flags |= SW_STAT_CLAMPED;
  }
  return SW_OK;
}

}  // namespace

extern "C" sw_status sw_shuffle_batch_device(sw_bank* b, const uint8_t* d_res,
                                             const uint64_t* d_offs, const uint32_t* d_lens,
                                             size_t n, uint32_t max_len, uint64_t seed,
                                             uint8_t* d_out, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (!d_res || !d_offs || !d_lens || !d_out)
    return fail(b, SW_ERR_ARG, "sw_shuffle_batch_device: null device buffer");
  if (n == 0 || n >= 0x100000000ull)
    return fail(b, SW_ERR_ARG, "sw_shuffle_batch_device: 0 < n < 2^32");
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_shuffle_batch_device(r, d_res, d_offs, d_lens, n, max_len, seed, d_out, s);
      }))
    return st;
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  const sw_status st = timed_on(b, hs, [&] {
    return swk_shuffle_batch(d_res, d_offs, d_lens, n, max_len, 0, seed, d_out, nullptr, 0, hs);
  });
  if (st != SW_OK) return st;
  snprintf(b->last_kernel, sizeof(b->last_kernel), "shuffle n=%zu", n);
  return SW_OK;
}

extern "C" sw_status sw_score_histogram_device(sw_bank* b, const int32_t* d_scores,
                                               const uint32_t* d_lens, size_t n, size_t nq,
                                               uint64_t* d_counts, uint64_t* d_len_sums,
                                               uint64_t* d_clamped, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (const char* why = bad_hist_args(d_scores, d_counts, n, nq))
    return fail(b, SW_ERR_ARG, "sw_score_histogram_device: %s", why);
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_score_histogram_device(r, d_scores, d_lens, n, nq, d_counts, d_len_sums,
                                         d_clamped, s);
      }))
    return st;
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  const sw_status st = timed_on(b, hs, [&] {
    return swk_stat_hist(d_scores, d_lens, n, nq, reinterpret_cast<unsigned long long*>(d_counts),
                         reinterpret_cast<unsigned long long*>(d_len_sums),
                         reinterpret_cast<unsigned long long*>(d_clamped), hs);
  });
  if (st != SW_OK) return st;
  snprintf(b->last_kernel, sizeof(b->last_kernel), "stat-hist nq=%zu n=%zu", nq, n);
  return SW_OK;
}

extern "C" sw_status sw_estimate_statistics_device(sw_bank* b, const uint8_t* d_res,
                                                   const uint64_t* d_offs, const uint32_t* d_lens,
                                                   size_t n, uint32_t min_len, uint32_t max_len,
                                                   uint64_t seed, uint32_t rounds,
                                                   sw_statistics* out, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (!d_res || !d_offs || !d_lens || !out)
    return fail(b, SW_ERR_ARG, "sw_estimate_statistics_device: null buffer");
  if (n == 0 || n >= 0x100000000ull || rounds == 0)
    return fail(b, SW_ERR_ARG, "sw_estimate_statistics_device: 0 < n < 2^32 and rounds >= 1");
  if (min_len > max_len) return fail(b, SW_ERR_ARG, "min_len %u > max_len %u", min_len, max_len);
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  const size_t nq = sw_query_count(b);
  HIPOK(b, hipSetDevice(r->device));
  hipStream_t hs = stream_or(r, stream);
  // a slice of targets: its shuffled codes at a fixed stride, its offsets, nq rows of scores
  SlicePlan pl;
  SliceScratch& sl = r->stat_slice;
  sw_status ps = slice_plan(b, "SWBANK_STAT_MB", n, nq, max_len, true, pl);
  if (ps == SW_OK) ps = slice_reserve(b, sl, pl, nq, hs);
  if (ps != SW_OK) return ps;
  const size_t span = pl.span;
  const size_t row = (size_t)SW_STAT_BINS, words = nq * (2 * row + 1);  // counts, sums, clamped
  HIPOK(b, r->stat_cnt.reserve(words));
  unsigned long long* counts = r->stat_cnt.p;
  unsigned long long* sums = counts + nq * row;
  unsigned long long* clamped = sums + nq * row;
  HIPOK(b, hipMemsetAsync(counts, 0, words * sizeof(*counts), hs));
  for (uint32_t rd = 0; rd < rounds; ++rd) {
    for (size_t k0 = 0; k0 < n; k0 += span) {
      const size_t nk = std::min(span, n - k0);
      HIPOK(b, swk_shuffle_batch(d_res, d_offs + k0, d_lens + k0, nk, max_len, k0, seed + rd,
                                 sl.codes.p, sl.offs.p, (uint32_t)pl.stride, hs));
      const sw_status st =
          sw_score_batch_device_range(b, sl.codes.p, sl.offs.p, d_lens + k0, nullptr, nk, min_len,
                                      max_len, sl.scores.p, hs);
      if (st != SW_OK) {
        (void)hipStreamSynchronize(hs);  // (nothing of the call is left in flight)
        return st;
      }
      HIPOK(b, hipSetDevice(r->device));
      HIPOK(b, swk_stat_hist(sl.scores.p, d_lens + k0, nk, nq, counts, sums, clamped, hs));
    }
  }
  std::vector<unsigned long long> host(words);
  HIPOK(b, hipMemcpyAsync(host.data(), counts, words * sizeof(*counts), hipMemcpyDeviceToHost,
                          hs));
  HIPOK(b, hipStreamSynchronize(hs));
  // the scoring passes' hand-off faults: their scores, and so the counts, are invalid
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (const sw_status st = fit_rows(b, r, host, nq, out); st != SW_OK) return st;
  snprintf(b->last_kernel, sizeof(b->last_kernel), "stats rounds=%u nq=%zu n=%zu slices=%zu",
           rounds, nq, n, pl.slices);
  return SW_OK;
}

extern "C" sw_status sw_estimate_statistics(sw_bank* b, const uint8_t* residues,
                                            size_t residues_len, const uint64_t* offsets,
                                            const uint32_t* lens, size_t n, uint64_t seed,
                                            uint32_t rounds, sw_statistics* out) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (!residues || !offsets || !lens || !out)
    return fail(b, SW_ERR_ARG, "sw_estimate_statistics: null buffer");
  if (n == 0 || n >= 0x100000000ull || rounds == 0)
    return fail(b, SW_ERR_ARG, "sw_estimate_statistics: 0 < n < 2^32 and rounds >= 1");
  sw_bank* r = root_of(b);
  if (!r->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  uint32_t lo, hi;
  StagedBatch& sb = r->stat_host;
  sw_status st = stage_host_batch(b, sb, residues, residues_len, offsets, lens, n, nullptr, false,
                                  nullptr, lo, hi);
  if (st != SW_OK) return st;
  hipStream_t hs = r->stream;
  st = sw_estimate_statistics_device(b, sb.res.p, sb.offs.p, sb.lens.p, n, lo, hi, seed, rounds,
                                     out, hs);
  if (st != SW_OK) (void)hipStreamSynchronize(hs);  // (the uploads have left the caller's buffers)
  return st;
}

// The estimate for the frameshift-tolerant translated search (include/swbank.h "statistics of
// frameshift hits"): the same slices, counters and fit, the scoring pass being
// swbank_kfshift.hip's kernel on the shuffled DNA, which needs the alignment unit's table
// (prepare_align, the ev_ready wait, the ev_used record) and no scratch beyond the slice.
extern "C" sw_status sw_estimate_fshift_statistics_device(
    sw_bank* b, const uint8_t* d_res, const uint64_t* d_offs, const uint32_t* d_lens, size_t n,
    uint32_t max_len, const uint8_t* codon_table, int32_t frameshift, uint64_t seed,
    uint32_t rounds, sw_statistics* out, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  const char* const me = "sw_estimate_fshift_statistics_device";
  uint8_t tab[64];
  if (const sw_status st = fshift_opening(b, me, codon_table, frameshift, tab); st != SW_OK)
    return st;
  if (!d_res || !d_offs || !d_lens || !out) return fail(b, SW_ERR_ARG, "%s: null buffer", me);
  if (n == 0 || n >= 0x100000000ull || rounds == 0)
    return fail(b, SW_ERR_ARG, "%s: 0 < n < 2^32 and rounds >= 1", me);
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (sw_status st; on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_estimate_fshift_statistics_device(r, d_res, d_offs, d_lens, n, max_len,
                                                    codon_table, frameshift, seed, rounds, out, s);
      }))
    return st;
  sw_status st = prepare(b);
  if (st != SW_OK) return st;
  if ((size_t)b->alpha * b->alpha != b->matrix.size() || b->alpha > SW_PROTEIN_ALPHA)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: alphabet %d too large", me, b->alpha);
  if ((st = prepare_align(b)) != SW_OK) return st;
  const size_t nq = sw_query_count(b);
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  // a slice of targets: its shuffled bases at a fixed stride, its offsets, nq rows of scores
  SlicePlan pl;
  SliceScratch& sl = b->stat_slice;
  if ((st = slice_plan(b, "SWBANK_STAT_MB", n, nq, max_len, true, pl)) != SW_OK) return st;
  if ((st = slice_reserve(b, sl, pl, nq, hs)) != SW_OK) return st;
  const size_t row = (size_t)SW_STAT_BINS, words = nq * (2 * row + 1);  // counts, sums, clamped
  HIPOK(b, b->stat_cnt.reserve(words));
  unsigned long long* counts = b->stat_cnt.p;
  unsigned long long* sums = counts + nq * row;
  unsigned long long* clamped = sums + nq * row;
  HIPOK(b, hipMemsetAsync(counts, 0, words * sizeof(*counts), hs));
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  const uint2* qtab = reinterpret_cast<const uint2*>(b->al_tab.p);
  const int8_t* mat = reinterpret_cast<const int8_t*>(b->al_tab.p + nq * sizeof(uint2));
  const uint8_t* qcodes = b->al_tab.p + nq * sizeof(uint2) + b->matrix.size();
  for (uint32_t rd = 0; rd < rounds && st == SW_OK; ++rd) {
    for (size_t k0 = 0; k0 < n && st == SW_OK; k0 += pl.span) {
      const size_t nk = std::min(pl.span, n - k0);
      st = timed_on(b, hs, [&] {
        return swk_shuffle_batch(d_res, d_offs + k0, d_lens + k0, nk, max_len, k0, seed + rd,
                                 sl.codes.p, sl.offs.p, (uint32_t)pl.stride, hs);
      });
      if (st == SW_OK)
        st = timed_on(b, hs, [&] {
          return swk_fshift_score(sl.codes.p, sl.offs.p, d_lens + k0, nk, max_len, qtab, mat,
                                  qcodes, nq, (uint32_t)b->query.size(), (uint32_t)b->alpha, tab,
                                  b->gap_open + b->gap_extend, b->gap_extend, frameshift,
                                  sl.scores.p, nullptr, hs);
        });
      if (st == SW_OK)
        st = timed_on(b, hs, [&] {
          return swk_stat_hist(sl.scores.p, d_lens + k0, nk, nq, counts, sums, clamped, hs);
        });
    }
  }
  // whatever was launched reads the table: the next upload is ordered after it in any case
  const hipError_t er = hipEventRecord(b->ev_used, hs);
  std::vector<unsigned long long> host(words);
  hipError_t ec = hipSuccess;
  if (st == SW_OK && er == hipSuccess)
    ec = hipMemcpyAsync(host.data(), counts, words * sizeof(*counts), hipMemcpyDeviceToHost, hs);
  const hipError_t es = hipStreamSynchronize(hs);  // (nothing of the call is left in flight)
  if (st != SW_OK) return st;
  HIPOK(b, er);
  HIPOK(b, ec);
  HIPOK(b, es);
  if ((st = take_fault(b, 0)) != SW_OK) return st;
  if ((st = fit_rows(b, b, host, nq, out)) != SW_OK) return st;
  b->best_kind = 0;  // no best hit is tracked
  snprintf(b->last_kernel, sizeof(b->last_kernel),
           "fshift-stats rounds=%u nq=%zu n=%zu slices=%zu", rounds, nq, n, pl.slices);
  return SW_OK;
}

extern "C" sw_status sw_estimate_fshift_statistics(sw_bank* b, const uint8_t* residues,
                                                   size_t residues_len, const uint64_t* offsets,
                                                   const uint32_t* lens, size_t n,
                                                   const uint8_t* codon_table, int32_t frameshift,
                                                   uint64_t seed, uint32_t rounds,
                                                   sw_statistics* out) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  const char* const me = "sw_estimate_fshift_statistics";
  uint8_t tab[64];
  if (const sw_status st = fshift_opening(b, me, codon_table, frameshift, tab); st != SW_OK)
    return st;
  if (!offsets || !lens || !out) return fail(b, SW_ERR_ARG, "%s: null buffer", me);
  if (n == 0 || n >= 0x100000000ull || rounds == 0)
    return fail(b, SW_ERR_ARG, "%s: 0 < n < 2^32 and rounds >= 1", me);
  // the batch holds DNA codes, which the staging (it knows the bank's protein alphabet) cannot
  // check: checked here, after the staging has placed every target inside the residues
  sw_bank* r = root_of(b);
  uint32_t lo, hi;
  StagedBatch& sb = r->stat_host;
  sw_status st = stage_host_batch(b, sb, residues, residues_len, offsets, lens, n, nullptr, false,
                                  nullptr, lo, hi);
  hipStream_t hs = r->stream;
  for (size_t k = 0; k < n && st == SW_OK; ++k) {
    if (lens[k] && !residues) st = fail(b, SW_ERR_ARG, "%s: null residues", me);
    for (uint32_t i = 0; i < lens[k] && st == SW_OK; ++i)
      if (residues[offsets[k] + i] >= SW_DNA_ALPHA)
        st = fail(b, SW_ERR_ARG, "target %zu code %u at %u is no DNA code", k,
                  residues[offsets[k] + i], i);
  }
  if (st == SW_OK)
    st = sw_estimate_fshift_statistics_device(b, sb.res.p, sb.offs.p, sb.lens.p, n, hi,
                                              codon_table, frameshift, seed, rounds, out, hs);
  if (st != SW_OK) (void)hipStreamSynchronize(hs);  // (the uploads have left the caller's buffers)
  return st;
}

extern "C" sw_status sw_hit_significance_device(sw_bank* b, const sw_statistics* st,
                                                const int32_t* d_hit_scores, const uint64_t* d_hits,
                                                const uint32_t* d_lens, size_t hits_per_query,
                                                size_t nq, uint64_t db_size, double* d_bits,
                                                double* d_evalues, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (!st || !d_hit_scores || !d_hits || !d_lens || (!d_bits && !d_evalues))
    return fail(b, SW_ERR_ARG, "sw_hit_significance_device: null argument, or neither output");
  if (hits_per_query == 0 || nq == 0)
    return fail(b, SW_ERR_ARG, "sw_hit_significance_device: hits_per_query and nq must be positive");
  const size_t pw = swk_stat_par_doubles();
  if (hits_per_query > SIZE_MAX / sizeof(uint64_t) / nq || nq > SIZE_MAX / (pw * sizeof(double)))
    return fail(b, SW_ERR_ARG, "sw_hit_significance_device: nq x hits_per_query overflows size_t");
  for (size_t i = 0; i < nq; ++i)
    if (degenerate(st[i]))
      return fail(b, SW_ERR_ARG, "sw_hit_significance_device: degenerate statistics (row %zu)", i);
  if (sw_status fs; on_root(b, stream, fs, [&](sw_bank* r, void* s) {
        return sw_hit_significance_device(r, st, d_hit_scores, d_hits, d_lens, hits_per_query, nq,
                                          db_size, d_bits, d_evalues, s);
      }))
    return fs;
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  // the previous call's upload and kernel (on any stream) are done with the parameters, on the
  // host and on the device, before they are replaced: a short host wait for a small kernel
  if (!b->ev_stat) HIPOK(b, hipEventCreateWithFlags(&b->ev_stat, hipEventDisableTiming));
  else HIPOK(b, hipEventSynchronize(b->ev_stat));
  std::vector<double>& par = b->stat_hpar;
  par.assign(nq * pw, 0.0);
  for (size_t i = 0; i < nq; ++i) {
    par[i * pw + 0] = st[i].lambda;
    par[i * pw + 1] = st[i].K;
    par[i * pw + 2] = (double)st[i].query_len;
    par[i * pw + 3] = std::log(st[i].K);
  }
  HIPOK(b, b->stat_par.reserve(par.size()));
  HIPOK(b, hipMemcpyAsync(b->stat_par.p, par.data(), par.size() * sizeof(double),
                          hipMemcpyHostToDevice, hs));
  const sw_status s = timed_on(b, hs, [&] {
    return swk_stat_signif(b->stat_par.p, d_hit_scores, d_hits, d_lens, hits_per_query, nq,
                           (double)db_size, d_bits, d_evalues, hs);
  });
  const hipError_t er = hipEventRecord(b->ev_stat, hs);
  if (s != SW_OK) return s;
  HIPOK(b, er);
  snprintf(b->last_kernel, sizeof(b->last_kernel), "significance nq=%zu k=%zu", nq, hits_per_query);
  return SW_OK;
}
