// swbank_bank.hip — the bank object: lifecycle, penalties, queries and the query tables.
// 
// Call surface mirrors ScoreBank_v2 (reference ScoreBank/ScoreBank_v2.v:30-44): penalties once,
// a query once, then any number of target batches; one max score per target.  See
// include/swbank.h for the per-function reference citations.
#include "swbank_bank.h"

sw_status fail(sw_bank* b, sw_status st, const char* fmt, ...) {
  if (b) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b->err, sizeof(b->err), fmt, ap);
    va_end(ap);
  }
  return st;
}

extern "C" int32_t sw_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// RCCL for the multi-device score gather (SURVEY §8 e: ncclCommInitAll, rccl.h:236, and
// ncclGather, rccl.h:745).  Loaded on first use so single-device users never map it; in a
// process where PyTorch already mapped its librccl.so.1 that copy is reused (same SONAME).
static sw_status check_device(int dev) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SW_ERR_NO_DEVICE;
  if (dev < 0 || dev >= ndev) return SW_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return SW_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SW_ERR_NO_DEVICE;
  return SW_OK;
}


extern "C" sw_status sw_bank_create(sw_bank** out, const sw_config* cfg_in) {
  DevGuard dev_guard;  // the caller's current device is restored on return (ABI 6)
  if (!out) return SW_ERR_ARG;
  *out = nullptr;
  sw_config cfg;
  if (cfg_in)
    cfg = *cfg_in;
  else
    sw_config_default(&cfg);
  if (cfg.alphabet != SW_ALPHABET_DNA && cfg.alphabet != SW_ALPHABET_PROTEIN) return SW_ERR_ARG;
  if (cfg.gap_model != SW_GAP_MERGED && cfg.gap_model != SW_GAP_GOTOH) return SW_ERR_ARG;
  if (cfg.max_query_len > SWB_MAX_QUERY) return SW_ERR_UNSUPPORTED;
  if (cfg.n_devices < 0 || cfg.n_devices > SW_MAX_DEVICES) return SW_ERR_ARG;

  if (cfg.n_devices >= 1) {
    // Multi-device bank (≙ MODULES ScoringModules behind one PrioEncoder, ScoreBank_v2.v:76-148):
    // a child bank per device; every host batch is dealt over them.
    for (int d = 0; d < cfg.n_devices; ++d) {
      const sw_status st = check_device(cfg.devices[d]);
      if (st != SW_OK) return st;
    }
    sw_bank* b = new (std::nothrow) sw_bank();
    if (!b) return SW_ERR_NOMEM;
    b->cfg = cfg;
    b->device = cfg.devices[0];
    b->alpha = cfg.alphabet == SW_ALPHABET_DNA ? SW_DNA_ALPHA : SW_PROTEIN_ALPHA;
    for (int d = 0; d < cfg.n_devices; ++d) {
      sw_config kc = cfg;
      kc.n_devices = 0;
      kc.device = cfg.devices[d];
      sw_bank* k = nullptr;
      const sw_status st = sw_bank_create(&k, &kc);
      if (st != SW_OK) {
        sw_bank_destroy(b);
        return st;
      }
      k->pool_threads = std::max(2u, host_threads() / (unsigned)cfg.n_devices);
      b->kids.push_back(k);
    }
    b->dpool.reset(new (std::nothrow) HostPool((unsigned)cfg.n_devices));
    b->pool.reset(new (std::nothrow) HostPool(host_threads()));
    if (!b->dpool || !b->pool) {
      sw_bank_destroy(b);
      return SW_ERR_NOMEM;
    }
    // RCCL gather when every device is distinct (RCCL refuses two ranks on one device) unless
    // SWBANK_GATHER=copy; SWBANK_GATHER=rccl makes an RCCL failure an error instead of a
    // fallback to device copies.
    const char* gm = std::getenv("SWBANK_GATHER");
    const bool force_copy = gm && std::strcmp(gm, "copy") == 0;
    const bool force_rccl = gm && std::strcmp(gm, "rccl") == 0;
    bool distinct = true;
    for (int i = 0; i < cfg.n_devices; ++i)
      for (int j = 0; j < i; ++j) distinct = distinct && cfg.devices[i] != cfg.devices[j];
    if (!force_copy && (distinct || force_rccl)) {
      const Rccl& r = rccl();
      ncclResult_t nr = ncclSuccess;
      if (r.ok) {
        std::vector<ncclComm_t> comms((size_t)cfg.n_devices);
        nr = r.commInitAll(comms.data(), cfg.n_devices, cfg.devices);
        if (nr == ncclSuccess) b->comms.assign(comms.begin(), comms.end());
      }
      b->rccl_gather = !b->comms.empty();
      if (b->comms.empty() && force_rccl) {
        sw_bank_destroy(b);
        return SW_ERR_UNSUPPORTED;
      }
      if (b->comms.empty())
        snprintf(b->err, sizeof(b->err), "RCCL unavailable (%s), gathering with device copies",
                 r.ok ? r.errorString(nr) : r.err);
    }
    (void)hipSetDevice(b->device);
    *out = b;
    return SW_OK;
  }

  int dev = cfg.device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return SW_ERR_NO_DEVICE;
  const sw_status dst = check_device(dev);
  if (dst != SW_OK) return dst;

  sw_bank* b = new (std::nothrow) sw_bank();
  if (!b) return SW_ERR_NOMEM;
  b->cfg = cfg;
  b->device = dev;
  // The bank's four streams are created together, here: HIP maps streams onto its hardware
  // queues (GPU_MAX_HW_QUEUES, 4 by default) in creation order, so streams the caller creates
  // between the bank's creation and its first host-buffer call (torch's, in bench.py) used to
  // push the feeder's second kernel stream onto the bank stream's queue -- the two chunk
  // streams then serialised: ragged host calls 2.8-3.2 ms instead of 2.2-2.5 (LEDGER §3.2)
  if (hipSetDevice(dev) != hipSuccess ||
      hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&b->out_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking) != hipSuccess) {
    for (hipStream_t* x : {&b->stream, &b->copy_stream, &b->out_stream, &b->stream2})
      if (*x) (void)hipStreamDestroy(*x);
    delete b;
    return SW_ERR_HIP;
  }
  b->alpha = cfg.alphabet == SW_ALPHABET_DNA ? SW_DNA_ALPHA : SW_PROTEIN_ALPHA;
  if (hipDeviceGetAttribute(&b->cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    b->cus = 0;
  if (cfg.alphabet == SW_ALPHABET_PROTEIN) {  // BLOSUM62 -11/-1 until sw_set_matrix is called
    int8_t m[SW_PROTEIN_ALPHA * SW_PROTEIN_ALPHA];
    sw_fill_matrix(SW_ALPHABET_PROTEIN, 0, 0, m);
    b->matrix.assign(m, m + sizeof(m));
    b->gap_open = -11;
    b->gap_extend = -1;
    b->have_pen = true;
  }
  *out = b;
  return SW_OK;
}

// Every buffer of the bank frees itself when the bank is deleted: on the bank's device, after
// everything that may still use one has been waited for.
extern "C" void sw_bank_destroy(sw_bank* b) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return;
  if (b->is_multi() || !b->comms.empty()) {
    const Rccl& r = rccl();
    for (void* c : b->comms) (void)r.commDestroy(static_cast<ncclComm_t>(c));
    (void)hipSetDevice(b->device);
    if (b->ev_used) (void)hipEventSynchronize(b->ev_used);  // the last device call's scatter
    if (b->ev_join) (void)hipEventDestroy(b->ev_join);
    if (b->ev_used) (void)hipEventDestroy(b->ev_used);
    for (sw_bank* k : b->kids) sw_bank_destroy(k);
    b->dpool.reset();
    b->pool.reset();
    (void)hipSetDevice(b->device);
    delete b;
    return;
  }
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->ev_top) (void)hipEventSynchronize(b->ev_top);  // the last top-hits call, on any stream
  if (b->ev_stat) (void)hipEventSynchronize(b->ev_stat);  // ... significance call
  if (b->ev_strand) (void)hipEventSynchronize(b->ev_strand);  // ... strand call
  if (b->ev_frame) (void)hipEventSynchronize(b->ev_frame);  // ... translated-search call
  uint64_t nl;
  double pm, sm;
  (void)sw_bank_timing(b, &nl, &pm, &sm);
  if (b->ev_ready) (void)hipEventDestroy(b->ev_ready);
  if (b->ev_used) (void)hipEventDestroy(b->ev_used);
  if (b->best_ev) (void)hipEventDestroy(b->best_ev);
  if (b->ev_top) (void)hipEventDestroy(b->ev_top);
  if (b->ev_stat) (void)hipEventDestroy(b->ev_stat);
  if (b->ev_strand) (void)hipEventDestroy(b->ev_strand);
  if (b->ev_frame) (void)hipEventDestroy(b->ev_frame);
  if (b->ev_join) (void)hipEventDestroy(b->ev_join);
  for (hipEvent_t e : b->deal_ev) (void)hipEventDestroy(e);
  if (b->copy_stream) (void)hipStreamSynchronize(b->copy_stream);
  if (b->out_stream) (void)hipStreamSynchronize(b->out_stream);
  if (b->stream2) (void)hipStreamSynchronize(b->stream2);
  for (hipEvent_t e : b->out_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->sev) (void)hipEventDestroy(e);
  for (int i = 0; i < sw_bank::NSLOT; ++i)
    if (b->h2d_done[i]) (void)hipEventDestroy(b->h2d_done[i]);
  for (int i = 0; i < sw_bank::NDSLOT; ++i)
    if (b->kern_done[i]) (void)hipEventDestroy(b->kern_done[i]);
  b->launcher.reset();  // (its thread and the pool's touch the pinned slots: gone before those)
  b->pool.reset();
  if (b->copy_stream) (void)hipStreamDestroy(b->copy_stream);
  if (b->out_stream) (void)hipStreamDestroy(b->out_stream);
  if (b->stream2) (void)hipStreamDestroy(b->stream2);
  if (b->kstream) (void)hipStreamDestroy(b->kstream);
  if (b->ev_s2) (void)hipEventDestroy(b->ev_s2);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

extern "C" long swbank_live_buffers(void) {
  return g_live_buffers.load(std::memory_order_relaxed);
}

// ---- what the entries after scoring share (swbank_bank.h) ----------------------------------
sw_status slice_plan(sw_bank* b, const char* budget_env, size_t n, size_t nq, uint32_t max_len,
                     bool codes, SlicePlan& plan) {
  plan.stride = codes ? ((size_t)max_len + 15) / 16 * 16 + 16 : 0;
  if (plan.stride > UINT32_MAX) return fail(b, SW_ERR_ARG, "max_len %u too long", max_len);
  const size_t per = nq * sizeof(int32_t) + (codes ? plan.stride + sizeof(uint64_t) : 0);
  const size_t budget = (size_t)std::max(1, env_int(budget_env, 256)) << 20;
  plan.span = std::min(n, std::max<size_t>(1, budget / per));
  plan.slices = (n + plan.span - 1) / plan.span;
  return SW_OK;
}

sw_status slice_reserve(sw_bank* b, SliceScratch& s, const SlicePlan& plan, size_t nq,
                        hipStream_t hs) {
  if (plan.stride) {
    // (the stride's padding is never written: zeroed once, so whatever a score kernel reads past
    // a target's end is a code of the alphabet, as in a caller's packed batch)
    if (s.codes.cap < plan.span * plan.stride + 64) {
      HIPOK(b, s.codes.reserve(plan.span * plan.stride + 64));
      HIPOK(b, hipMemsetAsync(s.codes.p, 0, s.codes.cap, hs));
    }
    HIPOK(b, s.offs.reserve(plan.span));
  }
  HIPOK(b, s.scores.reserve(plan.span * nq));
  return SW_OK;
}

sw_status stage_host_batch(sw_bank* b, StagedBatch& s, const uint8_t* residues,
                           size_t residues_len, const uint64_t* offsets, const uint32_t* lens,
                           size_t n, const char* coded, bool zero, hipEvent_t after, uint32_t& lo,
                           uint32_t& hi) {
  lo = UINT32_MAX;
  hi = 0;
  for (size_t k = 0; k < n; ++k) {
    if (offsets[k] > residues_len || lens[k] > residues_len - offsets[k])
      return fail(b, SW_ERR_ARG, "target %zu lies outside the %zu residues", k, residues_len);
    if (coded) {
      if (lens[k] && !residues) return fail(b, SW_ERR_ARG, "%s: null residues", coded);
      for (uint32_t i = 0; i < lens[k]; ++i)
        if (residues[offsets[k] + i] >= (uint32_t)b->alpha)
          return fail(b, SW_ERR_ARG, "target %zu code %u at %u outside the alphabet", k,
                      residues[offsets[k] + i], i);
    }
    lo = std::min(lo, lens[k]);
    hi = std::max(hi, lens[k]);
  }
  sw_bank* r = root_of(b);
  HIPOK(b, hipSetDevice(r->device));
  hipStream_t hs = r->stream;
  if (after) HIPOK(b, hipStreamWaitEvent(hs, after, 0));
  HIPOK(b, s.res.reserve(residues_len + 64));
  HIPOK(b, s.offs.reserve(n));
  HIPOK(b, s.lens.reserve(n));
  if (zero) HIPOK(b, hipMemsetAsync(s.res.p, 0, s.res.cap, hs));
  if (residues_len)
    HIPOK(b, hipMemcpyAsync(s.res.p, residues, residues_len, hipMemcpyHostToDevice, hs));
  HIPOK(b, hipMemcpyAsync(s.offs.p, offsets, n * sizeof(uint64_t), hipMemcpyHostToDevice, hs));
  HIPOK(b, hipMemcpyAsync(s.lens.p, lens, n * sizeof(uint32_t), hipMemcpyHostToDevice, hs));
  return SW_OK;
}

extern "C" int32_t sw_bank_devices(const sw_bank* b, int32_t* devices, int32_t cap) {
  if (!b) return 0;
  const int32_t n = b->is_multi() ? (int32_t)b->kids.size() : 1;
  for (int32_t i = 0; devices && i < std::min(n, cap); ++i)
    devices[i] = b->is_multi() ? b->kids[(size_t)i]->device : b->device;
  return n;
}

extern "C" const char* sw_last_error(const sw_bank* b) { return b ? b->err : "null bank"; }

extern "C" const char* sw_last_kernel(const sw_bank* b) { return b ? b->last_kernel : ""; }

uint32_t* fault_word(sw_bank* b) {
  if (!b->faultw.p) {
    if (b->faultw.reserve(64) != hipSuccess) return nullptr;
    std::memset(b->faultw.p, 0, b->faultw.cap);
  }
  return reinterpret_cast<uint32_t*>(b->faultw.p);
}

sw_status take_fault(sw_bank* b, int which) {
  if (b->is_multi()) {
    sw_status st = SW_OK;
    for (sw_bank* k : b->kids) {  // every child's word is cleared, the first fault reported
      const sw_status ks = take_fault(k, which);
      if (ks != SW_OK && st == SW_OK) st = fail(b, ks, "device %d: %s", k->device, k->err);
    }
    return st;
  }
  if (!b->faultw.p) return SW_OK;
  // the call kind's group: one word per fault kind (SWK_FAULT_WORDS, swbank_internal.h)
  volatile uint32_t* w = reinterpret_cast<volatile uint32_t*>(b->faultw.p) + which * SWK_FAULT_WORDS;
  uint32_t f = 0;
  for (int i = 0; i < SWK_FAULT_WORDS; ++i) {
    f |= w[i];
    w[i] = 0;
  }
  if (f == 0) return SW_OK;
  if (f & SWK_FAULT_BAL) ++b->ctr.balanced_timeouts;
  if (f & SWK_FAULT_TAIL) ++b->ctr.tail_timeouts;
  if (f & SWK_FAULT_WBAL) ++b->ctr.wave_balanced_timeouts;
  char kinds[96] = "";
  const char* names[3] = {"balanced ranges", "protein tail", "wave balanced ranges"};
  for (int i = 0; i < 3; ++i)
    if (f & (1u << i)) {
      if (kinds[0]) strncat(kinds, ", ", sizeof(kinds) - strlen(kinds) - 1);
      strncat(kinds, names[i], sizeof(kinds) - strlen(kinds) - 1);
    }
  return fail(b, SW_ERR_TIMEOUT,
              "a cross-workgroup hand-off wait ran out (%s) in a %s call: its scores are invalid",
              kinds, which ? "host-buffer" : "device");
}

extern "C" sw_status sw_bank_sync(sw_bank* b) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (b->is_multi()) {
    for (sw_bank* k : b->kids) {
      const sw_status st = sw_bank_sync(k);
      if (st != SW_OK) {
        (void)take_fault(b, 0);  // (clear the other devices' words too)
        return fail(b, st, "device %d: %s", k->device, k->err);
      }
    }
    if (b->ev_used) {  // the device-call deal's scatter on the root (multi_device)
      int cur = -1;
      HIPOK(b, hipGetDevice(&cur));
      hipError_t e = hipSetDevice(b->device);
      if (e == hipSuccess) e = hipEventSynchronize(b->ev_used);
      (void)hipSetDevice(cur);
      HIPOK(b, e);
    }
    return SW_OK;
  }
  int cur = -1;
  HIPOK(b, hipGetDevice(&cur));
  hipError_t e = hipSetDevice(b->device);
  // ev_used follows every launch of a scoring call on the stream it ran on
  if (e == hipSuccess && b->ev_used) e = hipEventSynchronize(b->ev_used);
  if (e == hipSuccess && b->ev_top) e = hipEventSynchronize(b->ev_top);  // ... of a top-hits call
  if (e == hipSuccess && b->ev_stat) e = hipEventSynchronize(b->ev_stat);  // ... significance
  if (e == hipSuccess && b->ev_strand) e = hipEventSynchronize(b->ev_strand);  // ... strands
  if (e == hipSuccess && b->ev_frame) e = hipEventSynchronize(b->ev_frame);  // ... frames
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  (void)hipSetDevice(cur);
  HIPOK(b, e);
  return take_fault(b, 0);
}

static void sum_counters(sw_counters& c, const sw_bank* b) {
  c.stream_calls += b->ctr.stream_calls;
  c.stream_reruns += b->ctr.stream_reruns;
  c.stream_declined += b->ctr.stream_declined;
  c.chunked_calls += b->ctr.chunked_calls;
  c.device_sorts += b->ctr.device_sorts;
  c.gather_timeouts += b->ctr.gather_timeouts;
  c.mixed_chunks += b->ctr.mixed_chunks;
  c.mixed_runs += b->ctr.mixed_runs;
  c.balanced_calls += b->ctr.balanced_calls;
  c.balanced_timeouts += b->ctr.balanced_timeouts;
  c.tail_timeouts += b->ctr.tail_timeouts;
  c.handoff_reruns += b->ctr.handoff_reruns;
  c.wave_balanced_timeouts += b->ctr.wave_balanced_timeouts;
  c.h2d_bytes += __atomic_load_n(&b->ctr.h2d_bytes, __ATOMIC_RELAXED);
}

// Host-side counts only (no HIP call): a hand-off time-out is counted when a synchronising call
// takes it from the fault word.
extern "C" sw_status sw_bank_counters_ex(const sw_bank* b, sw_counters* out, size_t out_size) {
  if (!b || !out) return SW_ERR_ARG;
  // the struct sizes of ABI 3 (8 counters), ABI 4 (10), ABI 5 (12) and ABI 6 (14)
  if (out_size != 64 && out_size != 80 && out_size != 96 && out_size != sizeof(sw_counters))
    return SW_ERR_ARG;
  sw_counters c{};
  sum_counters(c, b);
  for (const sw_bank* k : b->kids) sum_counters(c, k);
  std::memcpy(out, &c, out_size);
  return SW_OK;
}

// ABI 5: the two-argument form of ABI 3 again, writing the ABI-3 prefix (8 counters), so a
// caller of either earlier ABI never gets more bytes than its struct holds.
extern "C" sw_status sw_bank_counters(const sw_bank* b, sw_counters* out) {
  return sw_bank_counters_ex(b, out, 64);
}

void copy_kernel_name(sw_bank* b, const char* gather) {
  snprintf(b->last_kernel, sizeof(b->last_kernel), "multi[%zu] gather=%s: %s", b->kids.size(),
           gather, b->kids[0]->last_kernel);
}

static sw_status set_matrix_impl(sw_bank* b, const int8_t* m, int alpha, int32_t go,
                                 int32_t ge) {
  if (go > 0 || ge > 0 || go < -32767 || ge < -32767)
    return fail(b, SW_ERR_ARG, "gap penalties must be <= 0 (got open %d, extend %d)", go, ge);
  b->matrix.assign(m, m + (size_t)alpha * alpha);
  b->alpha = alpha;
  b->gap_open = go;
  b->gap_extend = ge;
  b->have_pen = true;
  b->dirty = true;
  return SW_OK;
}


extern "C" sw_status sw_set_penalties(sw_bank* b, int32_t match, int32_t mismatch,
                                      int32_t gap_open, int32_t gap_extend) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (b->is_multi())
    return each_kid(b, [&](sw_bank* k) {
      return sw_set_penalties(k, match, mismatch, gap_open, gap_extend);
    });
  if (b->cfg.alphabet != SW_ALPHABET_DNA)
    return fail(b, SW_ERR_ARG, "sw_set_penalties needs a DNA bank; use sw_set_matrix");
  int8_t m[SW_DNA_ALPHA * SW_DNA_ALPHA];
  if (sw_fill_matrix(SW_ALPHABET_DNA, match, mismatch, m) != SW_OK)
    return fail(b, SW_ERR_ARG, "match/mismatch outside int8 (%d, %d)", match, mismatch);
  return set_matrix_impl(b, m, SW_DNA_ALPHA, gap_open, gap_extend);
}

extern "C" sw_status sw_set_matrix(sw_bank* b, const int8_t* m, int32_t alpha, int32_t gap_open,
                                   int32_t gap_extend) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b || !m) return SW_ERR_ARG;
  if (b->is_multi())
    return each_kid(b, [&](sw_bank* k) { return sw_set_matrix(k, m, alpha, gap_open, gap_extend); });
  const int want = b->cfg.alphabet == SW_ALPHABET_DNA ? SW_DNA_ALPHA : SW_PROTEIN_ALPHA;
  if (alpha != want) return fail(b, SW_ERR_ARG, "matrix alphabet %d, bank expects %d", alpha, want);
  return set_matrix_impl(b, m, alpha, gap_open, gap_extend);
}

extern "C" sw_status sw_load_query(sw_bank* b, uint64_t id, const uint8_t* codes, uint32_t len) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b || (!codes && len)) return SW_ERR_ARG;
  if (b->is_multi()) {  // the query goes to every device (ScoreBank_v2.v:101-102)
    const sw_status st = each_kid(b, [&](sw_bank* k) { return sw_load_query(k, id, codes, len); });
    b->qset.clear();
    b->have_query = st == SW_OK;
    return st;
  }
  const uint32_t cap = b->cfg.max_query_len ? b->cfg.max_query_len : SWB_MAX_QUERY;
  if (len > cap)
    return fail(b, SW_ERR_UNSUPPORTED, "query length %u exceeds the bank maximum %u", len, cap);
  for (uint32_t i = 0; i < len; ++i)
    if (codes[i] >= (uint32_t)b->alpha)
      return fail(b, SW_ERR_ARG, "query code %u at %u outside alphabet %d", codes[i], i, b->alpha);
  b->query.assign(codes, codes + len);
  b->qid = id;
  b->qset.clear();
  b->have_query = true;
  b->dirty = true;
  return SW_OK;
}

// A query set: ld_sequence for several queries that every following device batch is scored
// against (scores query-major, nq x n).  One query = sw_load_query.
extern "C" sw_status sw_load_queries(sw_bank* b, size_t nq, const uint64_t* ids,
                                     const uint8_t* codes, const uint64_t* offsets,
                                     const uint32_t* lens) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b || nq == 0 || !offsets || !lens) return SW_ERR_ARG;
  if (b->is_multi()) {  // the set goes to every device (ScoreBank_v2.v:101-102)
    const sw_status st = each_kid(
        b, [&](sw_bank* k) { return sw_load_queries(k, nq, ids, codes, offsets, lens); });
    b->qset = b->kids[0]->qset;  // (sizes only: the guards and sw_query_count read it)
    b->have_query = st == SW_OK;
    return st;
  }
  if (nq > 65536) return fail(b, SW_ERR_UNSUPPORTED, "more than 65536 queries in one set");
  if (nq == 1) return sw_load_query(b, ids ? ids[0] : 0, codes + offsets[0], lens[0]);
  const uint32_t cap = b->cfg.max_query_len ? b->cfg.max_query_len : SWB_MAX_QUERY;
  size_t longest = 0;
  for (size_t i = 0; i < nq; ++i) {
    if (lens[i] > cap)
      return fail(b, SW_ERR_UNSUPPORTED, "query %zu length %u exceeds the bank maximum %u", i,
                  lens[i], cap);
    if (lens[i] && !codes) return fail(b, SW_ERR_ARG, "null query codes");
    for (uint32_t j = 0; j < lens[i]; ++j)
      if (codes[offsets[i] + j] >= (uint32_t)b->alpha)
        return fail(b, SW_ERR_ARG, "query %zu code %u at %u outside alphabet %d", i,
                    codes[offsets[i] + j], j, b->alpha);
    if (lens[i] > lens[longest]) longest = i;
  }
  b->qset.assign(nq, {});
  for (size_t i = 0; i < nq; ++i)
    b->qset[i].assign(codes + offsets[i], codes + offsets[i] + lens[i]);
  b->query = b->qset[longest];
  b->qid = ids ? ids[longest] : 0;
  b->have_query = true;
  b->dirty = true;
  b->mq_ready = false;
  b->al_ready = false;  // (the alignment calls' copy of the set)
  return SW_OK;
}

extern "C" size_t sw_query_count(const sw_bank* b) {
  return !b || !b->have_query ? 0 : b->qset.size() > 1 ? b->qset.size() : 1;
}

// ---- the query tables: built on the host by swbank_qtab.h, uploaded by TableUpload -------------
// The tuning knobs of the table construction (qtab::Options): the environment is read here only.
static qtab::Options table_options() {
  qtab::Options o;
  o.profile = env_int("SWBANK_PROFILE", 0);
  o.R = env_int("SWBANK_R", 0);
  o.RB = env_int("SWBANK_RB", 0);
  o.seg = env_int("SWBANK_SEG", 0);
  o.f16 = env_int("SWBANK_F16", 1);
  o.mq_pair = env_int("SWBANK_MQ_PAIR", 1);
  o.mq_pair_rows = env_int("SWBANK_MQ_PAIR_ROWS", 128);
  return o;
}

// Build the resident query state (the ScoringModule's query + penalty registers,
// ScoringModule_v1.1.v:110-150): either per-row 4-byte LUTs (DNA fast path) or a query
// profile QP[letter][row] = S - s(q_row, letter) (any alphabet).
sw_status prepare(sw_bank* b) {
  if (!b->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "load penalties (ld_penalties) and a query (ld_sequence) first");
  if (!b->dirty) return SW_OK;
  // analyse
  const int8_t* m = b->matrix.data();
  const qtab::Plan p = qtab::analyse(
      m, b->alpha, b->gotoh(), b->gap_open, b->gap_extend, (int)b->query.size(), table_options(),
      [](const qtab::Plan& q, int f16) {
        return swk_has_variant(q.R, q.RB, q.col0, q.prof, q.gotoh ? 1 : 0, f16) != 0;
      });
  if (p.status != SW_OK) return fail(b, p.status, "%s", p.msg);
  // build
  const qtab::QueryTables t = qtab::build_query(p, m, b->query.data());
  // upload
  HIPOK(b, hipSetDevice(b->device));
  if (!b->ev_ready) {
    HIPOK(b, hipEventCreateWithFlags(&b->ev_ready, hipEventDisableTiming));
    HIPOK(b, hipEventCreateWithFlags(&b->ev_used, hipEventDisableTiming));
    HIPOK(b, hipEventRecord(b->ev_ready, b->stream));
    HIPOK(b, hipEventRecord(b->ev_used, b->stream));
  }
  const std::pair<DevBuf<uint32_t>*, const std::vector<uint32_t>*> tables[] = {
      {&b->wtab16, &t.wt16},       {&b->wtab, &t.wt},       {&b->stab16[0], &t.st16[0]},
      {&b->stab[0], &t.st[0]},     {&b->stab16[1], &t.st16[1]}, {&b->stab[1], &t.st[1]},
      {&b->stab16[2], &t.st16[2]}, {&b->stab[2], &t.st[2]}, {&b->qtab, &t.tab},
      {&b->qtab16, &t.tab16},      {&b->qpair, &t.tpair},   {&b->qpair_skew, &t.tskew},
      {&b->skew_ctab, &t.tfloor}};
  size_t words = 0;
  for (const auto& u : tables) words += u.second->size();
  TableUpload up(b);
  SWOK(up.begin(words * 4));
  for (const auto& u : tables) SWOK(up.put(*u.first, *u.second));
  SWOK(up.end());
  // store
  b->plan = p;
  b->segs = t.segs;
  b->R = p.R;
  b->RB = p.RB;
  b->W = t.segs[0].W;
  b->col0 = p.col0;
  b->prof = p.prof;
  b->S = (uint32_t)p.S;
  b->O = (uint32_t)p.o;
  b->E = (uint32_t)p.e;
  b->smax = p.smax;
  b->nv = p.nv;
  b->PS = p.PS;
  b->pad = p.pad;
  b->f16 = p.f16;
  b->nv16 = p.nv16;
  b->PS16 = p.PS16;
  b->f16_neg = p.f16_neg;
  b->pair_bytes = t.pair_words * 4;  // one segment's table
  b->pS1 = t.pS1;
  b->pS2 = t.pS2;
  b->skew_entries = (uint32_t)t.tfloor.size();
  b->skew_neg = t.skew_neg;
  b->wK = p.wK;
  b->wsegs = p.wsegs;
  b->wPS = p.prof ? (uint32_t)(64 * p.wK) : 0;
  b->wPS16 = p.prof ? (uint32_t)(128 * p.wK) : 0;
  b->wseg_words = t.wt.size() / p.wsegs;
  b->wseg_words16 = t.wt16.size() / p.wsegs;
  for (int i = 0; i < 3; ++i) {
    b->sK[i] = p.sK[i];
    b->sseg_words[i] = t.st[i].size() / (2 << i);
    b->sseg_words16[i] = t.st16[i].size() / (2 << i);
    b->sPS[i] = p.prof ? (uint32_t)(64 * p.sK[i]) : 0;
    b->sPS16[i] = p.prof ? (uint32_t)(128 * p.sK[i]) : 0;
  }
  b->i32_ready = false;
  b->al_ready = false;
  b->mq_ready = false;
  b->dirty = false;
  return SW_OK;
}

// Row-LUT tables of every query of a set in the segment layout of the longest one (prepare()
// ran on it): query i's words at i * mq_words, and the set's letter-pair tables (qtab::SetTables).
sw_status prepare_multi(sw_bank* b) {
  if (b->mq_ready) return SW_OK;
  const qtab::SetTables t =
      qtab::build_set(b->plan, b->segs, b->matrix.data(), b->qset, table_options());
  TableUpload up(b);
  SWOK(up.begin((t.t8.size() + t.t16.size() + t.tp.size()) * 4));
  SWOK(up.put(b->mqtab, t.t8));
  SWOK(up.put(b->mqtab16, t.t16));
  SWOK(up.put(b->mqpair, t.tp));
  SWOK(up.end());
  b->mq_words = t.words;
  b->mq_pair_words = t.pair_words;
  b->mq_pair_segs = t.pair_segs;
  b->mq_pair_rows = t.pair_rows;
  b->mq_pS1 = t.pS1;
  b->mq_pS2 = t.pS2;
  b->mq_ready = true;
  return SW_OK;
}

// int32 re-score state, built on first use per (penalties, query): the per-strip profile of
// swk_launch_i32 (qtab::build_i32), uploaded on the bank stream like the other query tables.
sw_status prepare_i32(sw_bank* b) {
  if (b->i32_ready) return SW_OK;
  if (b->pad + 1 > 25)
    return fail(b, SW_ERR_UNSUPPORTED, "int32 kernel: alphabet %d too large", b->alpha);
  uint32_t strips = 0;
  const std::vector<int16_t> h =
      qtab::build_i32(b->matrix.data(), b->alpha, (int)b->S, b->pad, b->query.data(),
                      (uint32_t)b->query.size(), strips);
  TableUpload up(b);
  SWOK(up.begin(h.size() * 2));
  SWOK(up.put(b->i32prof, h));
  SWOK(up.end());
  b->i32_strips = strips;
  b->i32_ready = true;
  return SW_OK;
}

extern "C" sw_status sw_bank_set_timing(sw_bank* b, int32_t enable) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (b->is_multi()) return each_kid(b, [&](sw_bank* k) { return sw_bank_set_timing(k, enable); });
  b->timing = enable != 0;
  return SW_OK;
}

extern "C" sw_status sw_bank_timing(sw_bank* b, uint64_t* launches, double* pack_ms,
                                    double* score_ms) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  double p = 0, s = 0;
  uint64_t n = 0;
  sw_status st = SW_OK;
  if (b->is_multi()) {  // summed over the devices
    for (sw_bank* k : b->kids) {
      uint64_t kn = 0;
      double kp = 0, ks = 0;
      if ((st = sw_bank_timing(k, &kn, &kp, &ks)) != SW_OK)
        return fail(b, st, "device %d: %s", k->device, k->err);
      n += kn;
      p += kp;
      s += ks;
    }
    if (launches) *launches = n;
    if (pack_ms) *pack_ms = p;
    if (score_ms) *score_ms = s;
    return SW_OK;
  }
  for (auto& ev : b->events) {  // (b == a: the launch had no separate pack interval)
    float t1 = 0, t2 = 0;
    if (st == SW_OK && hipEventSynchronize(ev.c) == hipSuccess &&
        (ev.b == ev.a || hipEventElapsedTime(&t1, ev.a, ev.b) == hipSuccess) &&
        hipEventElapsedTime(&t2, ev.b, ev.c) == hipSuccess) {
      p += t1;
      s += t2;
      ++n;
    } else {
      st = fail(b, SW_ERR_HIP, "event timing failed");
    }
    (void)hipEventDestroy(ev.a);
    if (ev.b != ev.a) (void)hipEventDestroy(ev.b);
    (void)hipEventDestroy(ev.c);
  }
  b->events.clear();
  p += b->host_pack_ms;  // host calls: the feeder's gather / pack time on the host
  b->host_pack_ms = 0;
  if (launches) *launches = n;
  if (pack_ms) *pack_ms = p;
  if (score_ms) *score_ms = s;
  // the launches timed are complete: a device call's latched hand-off fault surfaces here
  if (st == SW_OK && n > 0) st = take_fault(b, 0);
  return st;
}

extern "C" sw_status sw_best_hit_device(sw_bank* b, const int32_t* d_scores, const uint64_t* d_ids,
                                        size_t n, uint64_t* d_out, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (b->is_multi())  // on the root device, where the multi-device calls leave the scores
    return sw_best_hit_device(b->kids[0], d_scores, d_ids, n, d_out,
                              stream ? stream : b->kids[0]->stream);
  if (!d_scores || !d_out || n == 0 || n > 0xFFFFFFFFull)
    return fail(b, SW_ERR_ARG, "sw_best_hit_device: empty, null or > 2^32 scores");
  HIPOK(b, hipSetDevice(b->device));
  HIPOK(b, b->best_key.reserve(1));
  HIPOK(b, swk_best_hit(d_scores, d_ids, n, b->best_key.p, d_out, nullptr,
                        stream ? reinterpret_cast<hipStream_t>(stream) : b->stream));
  return SW_OK;
}

extern "C" sw_status sw_best_hit(sw_bank* b, const int32_t* scores, const uint64_t* ids, size_t n,
                                 uint64_t* best_id, int32_t* best_score) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!scores || !best_id || !best_score || n == 0)
    return b ? fail(b, SW_ERR_ARG, "sw_best_hit: empty or null input") : SW_ERR_ARG;
  size_t bi = 0;
  for (size_t k = 1; k < n; ++k)
    if (scores[k] > scores[bi]) bi = k;
  *best_id = ids ? ids[bi] : (uint64_t)bi;
  *best_score = scores[bi];
  return SW_OK;
}

