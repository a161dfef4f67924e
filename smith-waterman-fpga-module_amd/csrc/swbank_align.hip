// swbank_align.hip — alignments of chosen hits (include/swbank.h "alignments of chosen hits",
// DESIGN.md §3.9): the ABI entries for one query (sw_align_hits*) and for a query set
// (sw_align_set_hits*), and for a set with a strand per pair (sw_align_strand_hits*, DESIGN.md
// §3.13), the chunking of the direction store, the host calls' staging.  All entries run the same
// code; they differ in the pair list.  The kernels are in
// swbank_kalign.hip.  The alignments of frameshift hits (sw_align_fshift_hits*, DESIGN.md §3.16,
// behind them) run the same scaffolding around the kernels of swbank_kfsalign.hip, and so do the
// alignments of global-local hits (sw_align_glocal_hits*, DESIGN.md §3.18, at the end of the file)
// around the kernels of swbank_kglalign.hip, and the non-intersecting local alignments
// (sw_align_disjoint_hits*) around the kernel of swbank_klalign.hip, and those
// over the six reading frames of a translated hit (sw_align_disjoint_frame_hits*, DESIGN.md §3.20,
// last) around the kernels of swbank_klaframes.hip.
#include "swbank_bank.h"

namespace {

// Direction-store budget in dwords (SWBANK_ALIGN_MB, MiB, default 256).
uint64_t dir_budget() {
  return ((uint64_t)std::max(1, env_int("SWBANK_ALIGN_MB", 256)) << 20) / 4;
}

// The pair list of a call.  !set (sw_align_hits*): hit h is the loaded query against target
// hits[h].  set (sw_align_set_hits*): query hit_queries[h], or h / hits_per_query, against target
// hits[h], or h.
struct Pairs {
  bool set;
  const uint32_t* hit_queries;
  size_t hits_per_query;
  const uint64_t* hits;
  size_t n_hits;
  // sw_align_strand_hits*: the nq x n strand matrix (NULL: every hit on the forward strand)
  bool strand_call = false;
  const uint8_t* strands = nullptr;
  // sw_align_frame_hits*: the set call over the translated hits (a protein bank's)
  bool frame_call = false;
};

size_t query_count(const sw_bank* b) { return b->qset.size() > 1 ? b->qset.size() : 1; }

}  // namespace

// The queries' codes and the matrix on the device, built on first use per (penalties, queries)
// and uploaded on the bank stream like the other query tables (prepare_i32): a {offset, length}
// entry per query, the alpha x alpha matrix, then the codes of every query back to back.  The
// frameshift search (swbank_fshift.hip) builds its profiles from the same table.
sw_status prepare_align(sw_bank* b) {
  if (b->al_ready) return SW_OK;
  const size_t nq = query_count(b);
  const std::vector<uint8_t>* queries = nq > 1 ? b->qset.data() : &b->query;
  size_t ql = 0;
  for (size_t i = 0; i < nq; ++i) ql += queries[i].size();
  if (ql > 0xFFFFFFFFull)
    return fail(b, SW_ERR_UNSUPPORTED, "alignments: the query set holds more than 2^32 codes");
  const std::vector<uint8_t> t = qtab::build_align(b->matrix, queries, nq);
  TableUpload up(b);
  SWOK(up.begin(t.size()));
  SWOK(up.put(b->al_tab, t));
  SWOK(up.end());
  b->al_ready = true;
  return SW_OK;
}

namespace {

// The state every entry needs; on return the bank is prepare()d.  The single-query entries
// refuse a loaded set.
sw_status align_ready(sw_bank* b, bool set) {
  if (!b->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  if (!set && b->qset.size() > 1)
    return fail(b, SW_ERR_STATE, "a query set is loaded: alignments take one query");
  const sw_status st = prepare(b);
  if (st != SW_OK) return st;
  if (!b->gotoh() && b->col0)
    return fail(b, SW_ERR_UNSUPPORTED,
                "alignments under merged gaps need max substitution score <= open + extend");
  if ((size_t)b->alpha * b->alpha != b->matrix.size() || b->alpha >= 25 || b->pad >= 25)
    return fail(b, SW_ERR_UNSUPPORTED, "alignment kernels: alphabet %d too large", b->alpha);
  return prepare_align(b);
}

// What a set call's pair list must satisfy whatever its buffers hold; n targets in the batch.
sw_status check_pairs(sw_bank* b, const Pairs& pr, size_t n) {
  if (pr.n_hits > 0xFFFFFFFFull) return fail(b, SW_ERR_ARG, "hit lists hold < 2^32 hits");
  if (!pr.set) return SW_OK;
  const size_t nq = query_count(b);
  if ((pr.hit_queries != nullptr) == (pr.hits_per_query != 0))
    return fail(b, SW_ERR_ARG, "give hit_queries or hits_per_query >= 1, not both");
  if (pr.hits_per_query > 0xFFFFFFFFull ||
      (pr.hits_per_query && (pr.n_hits + pr.hits_per_query - 1) / pr.hits_per_query > nq))
    return fail(b, SW_ERR_ARG, "n_hits = %zu > nq x hits_per_query = %zu x %zu", pr.n_hits, nq,
                pr.hits_per_query);
  if (!pr.hits && pr.n_hits > n)
    return fail(b, SW_ERR_ARG, "no hit list: n_hits = %zu > n = %zu", pr.n_hits, n);
  return SW_OK;
}

// The launch block of a call over `nh` hits of at most `max_len` columns; reserves the scratch.
sw_status align_block(sw_bank* b, SwkAlign& p, size_t nh, uint32_t max_len) {
  const uint32_t scols = std::max(max_len, 1u);
  const size_t budget = (size_t)std::max(1, env_int("SWBANK_EDGE_MB", 2048)) << 20;
  const size_t waves = swk_i32_waves(nh, scols, budget);
  const size_t nq = query_count(b);
  HIPOK(b, b->al_scr.reserve(waves * 2 * scols));
  p.gotoh = b->gotoh() ? 1 : 0;
  p.n_hits = nh;
  p.qtab = reinterpret_cast<const uint2*>(b->al_tab.p);
  p.nq = (uint32_t)nq;
  p.mat = reinterpret_cast<const int8_t*>(b->al_tab.p + nq * sizeof(uint2));
  p.query = b->al_tab.p + nq * sizeof(uint2) + b->matrix.size();
  p.qlen = (uint32_t)b->query.size();  // (a set: its longest query)
  p.alpha = (uint32_t)b->alpha;
  p.pad = b->pad;
  p.padscore = (int32_t)b->S - 255;
  p.O = b->O;
  p.E = b->E;
  p.scratch = b->al_scr.p;
  p.scols = scols;
  p.waves = waves;
  return SW_OK;
}

void name_kernel(sw_bank* b, bool set, size_t hits, size_t chunks, bool strand = false,
                 bool frame = false) {
  if (frame)
    snprintf(b->last_kernel, sizeof(b->last_kernel), "align-frame i32 nq=%zu hits=%zu chunks=%zu",
             query_count(b), hits, chunks);
  else if (strand)
    snprintf(b->last_kernel, sizeof(b->last_kernel), "align-strand i32 nq=%zu hits=%zu chunks=%zu",
             query_count(b), hits, chunks);
  else if (set)
    snprintf(b->last_kernel, sizeof(b->last_kernel), "align-set i32 nq=%zu hits=%zu chunks=%zu",
             query_count(b), hits, chunks);
  else
    snprintf(b->last_kernel, sizeof(b->last_kernel), "align i32 hits=%zu chunks=%zu", hits, chunks);
}

// How every entry opens: a strand call is for DNA banks, a frame call for protein banks; a
// multi-device bank checks the state it holds itself and hands the call to its root
// (call(root, stream)), where the caller's buffers are.  False on a single bank that may go on;
// else the call is over and `st` is its status.
template <class F>
bool align_opening(sw_bank* b, const Pairs& pr, void* stream, sw_status& st, F&& call) {
  if (pr.strand_call && b->cfg.alphabet != SW_ALPHABET_DNA) {
    st = fail(b, SW_ERR_UNSUPPORTED, "strand alignments: DNA banks only");
    return true;
  }
  if (pr.frame_call && b->cfg.alphabet != SW_ALPHABET_PROTEIN) {
    st = fail(b, SW_ERR_UNSUPPORTED, "frame alignments: protein banks only");
    return true;
  }
  if (!b->is_multi()) return false;
  if (!b->have_query)
    st = fail(b, SW_ERR_STATE, "penalties or query not loaded");
  else if (!pr.set && b->qset.size() > 1)
    st = fail(b, SW_ERR_STATE, "a query set is loaded: alignments take one query");
  else
    on_root(b, stream, st, call);
  return true;
}

// Passes C and D of a device call in slots of the largest possible window (nothing is read
// back); a window past the budget: every non-empty hit keeps SW_ALIGN_NO_PATH.
// launch(h0, count): passes C and D of hits [h0, h0 + count) in slots of `slot` dwords of al_dirs.
template <class Launch>
sw_status paths_in_slots(sw_bank* b, size_t n_hits, uint64_t slot, hipStream_t hs, size_t& chunks,
                         Launch&& launch) {
  const uint64_t budget = dir_budget();
  const size_t per =
      slot == 0 || slot > budget ? 0 : (size_t)std::min<uint64_t>(budget / slot, n_hits);
  if (per) HIPOK(b, b->al_dirs.reserve((size_t)(slot * per)));
  return timed_on(b, hs, [&] {
    for (size_t h0 = 0; per && h0 < n_hits; h0 += per, ++chunks) {
      const hipError_t e = launch(h0, std::min(per, n_hits - h0));
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  });
}

sw_status paths_by_slot(sw_bank* b, const SwkAlign& p, uint32_t max_len, hipStream_t hs,
                        size_t& chunks) {
  const uint64_t slot = swk_align_dir_dwords(p.qlen, max_len);
  return paths_in_slots(b, p.n_hits, slot, hs, chunks, [&](size_t h0, size_t count) {
    return swk_launch_align_paths(&p, nullptr, h0, count, nullptr, slot, b->al_dirs.p, hs);
  });
}

sw_status device_launch(sw_bank* b, const uint8_t* d_res, const uint64_t* d_offs,
                        const uint32_t* d_lens, const uint64_t* d_ids, size_t n, uint32_t max_len,
                        const Pairs& pr, sw_alignment* d_out, uint32_t* d_cigar, uint32_t stride,
                        hipStream_t hs) {
  SwkAlign p{};
  p.res = d_res;
  p.offs = d_offs;
  p.lens = d_lens;
  p.ids = d_ids;
  p.hits = pr.hits;
  p.set = pr.set ? 1 : 0;
  p.n = n;
  p.hit_queries = pr.hit_queries;
  p.hits_per_query = (uint32_t)pr.hits_per_query;
  p.strands = pr.strands;
  p.out = d_out;
  p.cigar = d_cigar;
  p.cigar_stride = d_cigar ? stride : 0;
  sw_status st = align_block(b, p, pr.n_hits, max_len);
  if (st != SW_OK) return st;
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_used, 0));   // bank scratch is free
  if ((st = timed_on(b, hs, [&] { return swk_launch_align_ends(&p, hs); })) != SW_OK) return st;
  size_t chunks = 0;
  if (p.cigar_stride && (st = paths_by_slot(b, p, max_len, hs, chunks)) != SW_OK) return st;
  HIPOK(b, swk_launch_align_flip(&p, hs));  // (a strand call: after the last pass)
  HIPOK(b, hipEventRecord(b->ev_used, hs));
  name_kernel(b, pr.set, pr.n_hits, chunks, pr.strand_call, pr.frame_call);
  return SW_OK;
}

// sw_align_hits_device, sw_align_set_hits_device and sw_align_strand_hits_device.
sw_status device_call(sw_bank* b, const uint8_t* d_res, const uint64_t* d_offs,
                      const uint32_t* d_lens, const uint64_t* d_ids, size_t n, uint32_t max_len,
                      const Pairs& pr, sw_alignment* d_out, uint32_t* d_cigar,
                      uint32_t cigar_stride, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  sw_status st;
  if (align_opening(b, pr, stream, st, [&](sw_bank* r, void* s) {
        return device_call(r, d_res, d_offs, d_lens, d_ids, n, max_len, pr, d_out, d_cigar,
                           cigar_stride, s);
      }))
    return st;
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if ((st = align_ready(b, pr.set)) != SW_OK) return st;
  if (pr.n_hits == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || (!pr.set && !pr.hits) || !d_out || n == 0)
    return fail(b, SW_ERR_ARG, "null device buffer or an empty batch");
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  if (d_cigar && cigar_stride && (uint64_t)pr.n_hits * cigar_stride > 0xFFFFFFFFull)
    return fail(b, SW_ERR_ARG, "n_hits x cigar_stride must fit 32 bits (cigar_offset)");
  HIPOK(b, hipSetDevice(b->device));
  return device_launch(b, d_res, d_offs, d_lens, d_ids, n, max_len, pr, d_out, d_cigar,
                       cigar_stride, stream_or(b, stream));
}

// ---- the host calls, step by step ---------------------------------------------------------
// The listed hits of a host call, gathered: hit h's codes at res[offs[h]], lens[h] of them, (a
// set call) its query q[h], SW_QUERY_NONE for a slot that names no pair (nothing is gathered),
// (a strand call) its strand s[h].  A repeated hit is gathered again.
struct Gathered {
  std::vector<uint64_t> offs;
  std::vector<uint32_t> lens, q;
  std::vector<uint8_t> s, res;
  uint32_t max_len = 0;
};

uint64_t target_of(const Pairs& pr, size_t h) { return pr.hits ? pr.hits[h] : (uint64_t)h; }

// Step 1: validate and gather the listed targets.
sw_status gather_hits(sw_bank* b, const uint8_t* residues, size_t residues_len,
                      const uint64_t* offsets, const uint32_t* lens, size_t n, const Pairs& pr,
                      Gathered& g) {
  const size_t n_hits = pr.n_hits, nq = query_count(b);
  g.offs.resize(n_hits);
  g.lens.resize(n_hits);
  g.q.resize(pr.set ? n_hits : 0);
  g.s.resize(pr.strands ? n_hits : 0);
  uint64_t total = 0;
  for (size_t h = 0; h < n_hits; ++h) {
    const uint64_t t = target_of(pr, h);
    g.offs[h] = total;
    g.lens[h] = 0;
    if (pr.set) {
      const uint32_t qi = pr.hit_queries ? pr.hit_queries[h] : (uint32_t)(h / pr.hits_per_query);
      g.q[h] = qi == SW_QUERY_NONE || t == SW_HIT_NONE ? SW_QUERY_NONE : qi;
      if (qi != SW_QUERY_NONE && qi >= nq)
        return fail(b, SW_ERR_ARG, "hit %zu: query %u >= nq = %zu", h, qi, nq);
      if (t == SW_HIT_NONE) continue;
    }
    if (t >= n) return fail(b, SW_ERR_ARG, "hit %zu: target %llu >= n = %zu", h,
                            (unsigned long long)t, n);
    if (pr.set && g.q[h] == SW_QUERY_NONE) continue;
    const uint64_t o = offsets[t], l = lens[t];
    if (l && (!residues || o > residues_len || l > residues_len - o))
      return fail(b, SW_ERR_ARG, "target %llu outside the residues", (unsigned long long)t);
    g.lens[h] = (uint32_t)l;
    if (pr.strands) g.s[h] = pr.strands[(size_t)g.q[h] * n + t] != 0;
    total += l;
    g.max_len = std::max(g.max_len, (uint32_t)l);
  }
  g.res.assign(std::max<uint64_t>(total, 1), 0);
  for (size_t h = 0; h < n_hits; ++h) {
    const uint8_t* src = g.lens[h] ? residues + offsets[target_of(pr, h)] : nullptr;
    for (uint32_t i = 0; i < g.lens[h]; ++i) {
      if (src[i] >= (uint32_t)b->alpha)
        return fail(b, SW_ERR_ARG, "target %llu code %u at %u outside alphabet %d",
                    (unsigned long long)target_of(pr, h), src[i], i, b->alpha);
      g.res[g.offs[h] + i] = src[i];
    }
  }
  return SW_OK;
}

// Step 2: the gathered batch on the device (hit h is target h against query al_hq[h], on strand
// al_hs[h]) and, with `block`, the launch block of the alignment kernels over it (its scratch
// rows included; the frameshift kernels have none and take the staged buffers alone).
sw_status stage_hits(sw_bank* b, const Pairs& pr, const Gathered& g, SwkAlign& p, hipStream_t hs,
                     bool block = true) {
  const size_t n_hits = pr.n_hits;
  HIPOK(b, b->al_res.reserve(g.res.size()));
  HIPOK(b, b->al_offs.reserve(n_hits));
  HIPOK(b, b->al_lens.reserve(n_hits));
  HIPOK(b, b->al_out.reserve(n_hits));
  if (pr.set) HIPOK(b, b->al_hq.reserve(n_hits));
  if (pr.strands) HIPOK(b, b->al_hs.reserve(n_hits));
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_used, 0));  // an earlier call may still read the buffers
  HIPOK(b, hipMemcpyAsync(b->al_res.p, g.res.data(), g.res.size(), hipMemcpyHostToDevice, hs));
  HIPOK(b, hipMemcpyAsync(b->al_offs.p, g.offs.data(), n_hits * 8, hipMemcpyHostToDevice, hs));
  HIPOK(b, hipMemcpyAsync(b->al_lens.p, g.lens.data(), n_hits * 4, hipMemcpyHostToDevice, hs));
  if (pr.set)
    HIPOK(b, hipMemcpyAsync(b->al_hq.p, g.q.data(), n_hits * 4, hipMemcpyHostToDevice, hs));
  if (pr.strands)
    HIPOK(b, hipMemcpyAsync(b->al_hs.p, g.s.data(), n_hits, hipMemcpyHostToDevice, hs));
  __atomic_fetch_add(&b->ctr.h2d_bytes, g.res.size() + n_hits * (pr.set ? 16 : 12),
                     __ATOMIC_RELAXED);
  p.res = b->al_res.p;
  p.offs = b->al_offs.p;
  p.lens = b->al_lens.p;
  p.out = b->al_out.p;
  if (pr.set) {
    p.set = 1;
    p.n = n_hits;
    p.hit_queries = b->al_hq.p;
  }
  if (pr.strands) {
    p.strands = b->al_hs.p;
    p.strand_by_hit = 1;
  }
  return block ? align_block(b, p, n_hits, g.max_len) : SW_OK;
}

// Step 3: the CIGAR windows of pass A's records that fit the budget (dwords of direction store),
// in hit order, in chunks that fit it together; each hit's ops in a slot of rows + columns of the
// window (a path never has more ops).  A pure function of the records and the budget.
struct Windows {
  std::vector<uint32_t> list;      // the planned hits
  std::vector<SwkAlignPlan> plan;  // ... and where each one's window and ops go
  std::vector<size_t> cut{0};      // chunk c = positions [cut[c], cut[c + 1])
  uint64_t most = 0, cig = 0;      // the largest chunk's dwords; ops slots in all
};

// dwords(Q, L): what a window of Q query rows and L target codes takes.
template <class D>
Windows plan_windows(const sw_alignment* out, size_t n_hits, uint64_t budget, D&& dwords) {
  Windows w;
  uint64_t used = 0;
  for (size_t h = 0; h < n_hits; ++h) {
    const sw_alignment& r = out[h];
    // (no window; for the local calls this is score <= 0, a global-local hit with a path may
    // score 0 or less)
    if (r.flags & SW_ALIGN_EMPTY) continue;
    const uint32_t Q = r.q_end - r.q_start + 1, L = r.t_end - r.t_start + 1;
    const uint64_t need = dwords(Q, L);
    if (need > budget) continue;  // SW_ALIGN_NO_PATH, coordinates stay
    if (used + need > budget) {
      w.cut.push_back(w.list.size());
      used = 0;
    }
    w.list.push_back((uint32_t)h);
    w.plan.push_back(SwkAlignPlan{used, need, w.cig, Q + L, 0});
    used += need;
    w.most = std::max(w.most, used);
    w.cig += (uint64_t)Q + L;
  }
  w.cut.push_back(w.list.size());
  return w;
}

// Step 4: the ops back to back in hit order, as many as the caller's buffer takes; their count.
size_t pack_ops(const Windows& w, const std::vector<uint32_t>& ops, sw_alignment* out,
                size_t n_hits, uint32_t* cigar, size_t cigar_cap) {
  size_t at = 0, k = 0;
  for (size_t h = 0; h < n_hits; ++h) {
    sw_alignment& r = out[h];
    const bool planned = k < w.list.size() && w.list[k] == h;
    const uint64_t from = planned ? w.plan[k].cig_off : 0;
    if (planned) ++k;
    r.cigar_offset = 0;
    // (a frameshift record carries its strand and frame bits already)
    if ((r.flags & (SW_ALIGN_EMPTY | SW_ALIGN_NO_PATH | SW_ALIGN_NO_HIT)) || !planned) continue;
    if (r.cigar_len > cigar_cap - at) {
      r.flags |= SW_ALIGN_NO_PATH;
      r.cigar_len = r.n_columns = r.n_identities = 0;
      continue;
    }
    std::memcpy(cigar + at, ops.data() + from, (size_t)r.cigar_len * 4);
    r.cigar_offset = (uint32_t)at;
    at += r.cigar_len;
  }
  return at;
}

// Step 5: the records speak of the caller's batch: index, id, the reverse strand's coordinates.
void rewrite_records(const Pairs& pr, const Gathered& g, const uint64_t* ids, bool with_cigar,
                     sw_alignment* out) {
  for (size_t h = 0; h < pr.n_hits; ++h) {
    if (!with_cigar) out[h].cigar_offset = 0;
    if (out[h].flags & SW_ALIGN_NO_HIT) continue;  // (index = id = SW_HIT_NONE)
    const uint64_t t = target_of(pr, h);
    out[h].index = t;
    out[h].id = ids ? ids[t] : t;
    if (pr.strands && g.s[h]) {  // the reverse strand: coordinates on the forward target
      out[h].flags |= SW_ALIGN_REVERSE;
      if (out[h].score > 0) {
        const uint32_t ts = out[h].t_start, te = out[h].t_end;
        out[h].t_start = g.lens[h] - 1 - te;
        out[h].t_end = g.lens[h] - 1 - ts;
      }
    }
  }
}

// What a host call does once its hits are staged, whichever kernels it runs: ends(hs) launches
// passes A and B over the staged hits (records at al_out); paths(list, count, plan, hs) launches
// passes C and D of one chunk (ops at al_cig by the plan, directions at al_dirs); dwords(Q, L) is
// the direction store of a window.  The records and the packed ops go to the caller's buffers.
template <class Ends, class Paths, class Dwords>
sw_status host_passes(sw_bank* b, const Pairs& pr, const Gathered& g, const uint64_t* ids,
                      hipStream_t hs, Ends&& ends, Paths&& paths, Dwords&& dwords,
                      sw_alignment* out, uint32_t* cigar, size_t cigar_cap, size_t* cigar_used,
                      size_t& chunks) {
  const size_t n_hits = pr.n_hits;
  sw_status st;
  // passes A and B, the records back
  if ((st = timed_on(b, hs, [&] { return ends(hs); })) != SW_OK) return st;
  HIPOK(b, hipMemcpyAsync(out, b->al_out.p, n_hits * sizeof(sw_alignment), hipMemcpyDeviceToHost,
                          hs));
  HIPOK(b, hipStreamSynchronize(hs));
  cigar_cap = std::min<size_t>(cigar_cap, 0xFFFFFFFFu);  // (cigar_offset is 32 bits)
  const bool with_cigar = cigar && cigar_cap;
  if (with_cigar) {
    const Windows w = plan_windows(out, n_hits, dir_budget(), dwords);
    std::vector<uint32_t> ops;
    if (!w.list.empty()) {  // passes C and D chunk by chunk, the records and the ops back
      HIPOK(b, b->al_dirs.reserve((size_t)w.most));
      HIPOK(b, b->al_cig.reserve((size_t)w.cig));
      HIPOK(b, b->al_list.reserve(w.list.size()));
      HIPOK(b, b->al_plan.reserve(w.plan.size()));
      HIPOK(b, hipMemcpyAsync(b->al_list.p, w.list.data(), w.list.size() * 4,
                              hipMemcpyHostToDevice, hs));
      HIPOK(b, hipMemcpyAsync(b->al_plan.p, w.plan.data(), w.plan.size() * sizeof(SwkAlignPlan),
                              hipMemcpyHostToDevice, hs));
      st = timed_on(b, hs, [&] {
        for (size_t c = 0; c + 1 < w.cut.size(); ++c) {
          if (w.cut[c + 1] == w.cut[c]) continue;
          const hipError_t e = paths(b->al_list.p + w.cut[c], w.cut[c + 1] - w.cut[c],
                                     b->al_plan.p + w.cut[c], hs);
          if (e != hipSuccess) return e;
          ++chunks;
        }
        return hipSuccess;
      });
      if (st != SW_OK) return st;
      ops.resize((size_t)w.cig);
      HIPOK(b, hipMemcpyAsync(out, b->al_out.p, n_hits * sizeof(sw_alignment),
                              hipMemcpyDeviceToHost, hs));
      HIPOK(b, hipMemcpyAsync(ops.data(), b->al_cig.p, ops.size() * 4, hipMemcpyDeviceToHost, hs));
      HIPOK(b, hipStreamSynchronize(hs));
    }
    const size_t used = pack_ops(w, ops, out, n_hits, cigar, cigar_cap);
    if (cigar_used) *cigar_used = used;
  }
  HIPOK(b, hipEventRecord(b->ev_used, hs));
  rewrite_records(pr, g, ids, with_cigar, out);
  return SW_OK;
}

// sw_align_hits, sw_align_set_hits and sw_align_strand_hits.
sw_status host_call(sw_bank* b, const uint8_t* residues, size_t residues_len,
                    const uint64_t* offsets, const uint32_t* lens, const uint64_t* ids, size_t n,
                    const Pairs& pr, sw_alignment* out, uint32_t* cigar, size_t cigar_cap,
                    size_t* cigar_used) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (cigar_used) *cigar_used = 0;
  sw_status st;
  if (align_opening(b, pr, nullptr, st, [&](sw_bank* r, void*) {  // (hit lists are small)
        return host_call(r, residues, residues_len, offsets, lens, ids, n, pr, out, cigar,
                         cigar_cap, cigar_used);
      }))
    return st;
  if ((st = align_ready(b, pr.set)) != SW_OK) return st;
  const size_t n_hits = pr.n_hits;
  if (n_hits == 0) return SW_OK;
  if (!offsets || !lens || (!pr.set && !pr.hits) || !out)
    return fail(b, SW_ERR_ARG, "null host buffer");
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  Gathered g;
  if ((st = gather_hits(b, residues, residues_len, offsets, lens, n, pr, g)) != SW_OK) return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = b->stream;
  SwkAlign p{};
  if ((st = stage_hits(b, pr, g, p, hs)) != SW_OK) return st;
  size_t chunks = 0;
  st = host_passes(
      b, pr, g, ids, hs, [&](hipStream_t s) { return swk_launch_align_ends(&p, s); },
      [&](const uint32_t* list, size_t count, const SwkAlignPlan* plan, hipStream_t s) {
        p.cigar = b->al_cig.p;
        p.cigar_stride = 1;  // (places come from the plan)
        return swk_launch_align_paths(&p, list, 0, count, plan, 0, b->al_dirs.p, s);
      },
      swk_align_dir_dwords, out, cigar, cigar_cap, cigar_used, chunks);
  if (st != SW_OK) return st;
  name_kernel(b, pr.set, n_hits, chunks, pr.strand_call, pr.frame_call);
  return SW_OK;
}

}  // namespace

extern "C" sw_status sw_align_hits_device(sw_bank* b, const uint8_t* d_res,
                                          const uint64_t* d_offs, const uint32_t* d_lens,
                                          const uint64_t* d_ids, size_t n, uint32_t max_len,
                                          const uint64_t* d_hits, size_t n_hits,
                                          sw_alignment* d_out, uint32_t* d_cigar,
                                          uint32_t cigar_stride, void* stream) {
  return device_call(b, d_res, d_offs, d_lens, d_ids, n, max_len,
                     Pairs{false, nullptr, 0, d_hits, n_hits}, d_out, d_cigar, cigar_stride,
                     stream);
}

extern "C" sw_status sw_align_hits(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                   const uint64_t* offsets, const uint32_t* lens,
                                   const uint64_t* ids, size_t n, const uint64_t* hits,
                                   size_t n_hits, sw_alignment* out, uint32_t* cigar,
                                   size_t cigar_cap, size_t* cigar_used) {
  return host_call(b, residues, residues_len, offsets, lens, ids, n,
                   Pairs{false, nullptr, 0, hits, n_hits}, out, cigar, cigar_cap, cigar_used);
}

extern "C" sw_status sw_align_set_hits_device(sw_bank* b, const uint8_t* d_res,
                                              const uint64_t* d_offs, const uint32_t* d_lens,
                                              const uint64_t* d_ids, size_t n, uint32_t max_len,
                                              const uint32_t* d_hit_queries,
                                              size_t hits_per_query, const uint64_t* d_hits,
                                              size_t n_hits, sw_alignment* d_out,
                                              uint32_t* d_cigar, uint32_t cigar_stride,
                                              void* stream) {
  return device_call(b, d_res, d_offs, d_lens, d_ids, n, max_len,
                     Pairs{true, d_hit_queries, hits_per_query, d_hits, n_hits}, d_out, d_cigar,
                     cigar_stride, stream);
}

extern "C" sw_status sw_align_set_hits(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                       const uint64_t* offsets, const uint32_t* lens,
                                       const uint64_t* ids, size_t n,
                                       const uint32_t* hit_queries, size_t hits_per_query,
                                       const uint64_t* hits, size_t n_hits, sw_alignment* out,
                                       uint32_t* cigar, size_t cigar_cap, size_t* cigar_used) {
  return host_call(b, residues, residues_len, offsets, lens, ids, n,
                   Pairs{true, hit_queries, hits_per_query, hits, n_hits}, out, cigar, cigar_cap,
                   cigar_used);
}

extern "C" sw_status sw_align_strand_hits_device(sw_bank* b, const uint8_t* d_res,
                                                 const uint64_t* d_offs, const uint32_t* d_lens,
                                                 const uint64_t* d_ids, size_t n, uint32_t max_len,
                                                 const uint8_t* d_strands,
                                                 const uint32_t* d_hit_queries,
                                                 size_t hits_per_query, const uint64_t* d_hits,
                                                 size_t n_hits, sw_alignment* d_out,
                                                 uint32_t* d_cigar, uint32_t cigar_stride,
                                                 void* stream) {
  return device_call(b, d_res, d_offs, d_lens, d_ids, n, max_len,
                     Pairs{true, d_hit_queries, hits_per_query, d_hits, n_hits, true, d_strands},
                     d_out, d_cigar, cigar_stride, stream);
}

extern "C" sw_status sw_align_strand_hits(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                          const uint64_t* offsets, const uint32_t* lens,
                                          const uint64_t* ids, size_t n, const uint8_t* strands,
                                          const uint32_t* hit_queries, size_t hits_per_query,
                                          const uint64_t* hits, size_t n_hits, sw_alignment* out,
                                          uint32_t* cigar, size_t cigar_cap, size_t* cigar_used) {
  return host_call(b, residues, residues_len, offsets, lens, ids, n,
                   Pairs{true, hit_queries, hits_per_query, hits, n_hits, true, strands}, out,
                   cigar, cigar_cap, cigar_used);
}

// ---- the translated search: a hit on its frame ---------------------------------
// Hit h (query i, target k) is aligned against the translation of frame frames[i * n + k] of its
// DNA target: the listed hits are translated, one protein target per hit, the set call above
// aligns query hq[h] against target h of that batch, and the records are rewritten to name the
// DNA target, its frame and nucleotide coordinates.
namespace {

Pairs frame_pairs(const uint32_t* hit_queries, size_t hits_per_query, const uint64_t* hits,
                  size_t n_hits) {
  Pairs pr{true, hit_queries, hits_per_query, hits, n_hits};
  pr.frame_call = true;
  return pr;
}

// Flags and nucleotide coordinates of a record on frame f of a target of L codes.
void frame_record(sw_alignment& r, uint32_t f, uint32_t L) {
  const uint32_t o = f % 3;
  r.flags |= (o << SW_ALIGN_FRAME_SHIFT) | (f >= 3 ? (uint32_t)SW_ALIGN_REVERSE : 0u);
  if (r.score <= 0) return;
  const uint32_t fs = o + 3 * r.t_start, fe = o + 3 * r.t_end + 2;
  r.t_start = f < 3 ? fs : L - 1 - fe;
  r.t_end = f < 3 ? fe : L - 1 - fs;
}

}  // namespace

extern "C" sw_status sw_align_frame_hits_device(sw_bank* b, const uint8_t* d_res,
                                                const uint64_t* d_offs, const uint32_t* d_lens,
                                                const uint64_t* d_ids, size_t n, uint32_t max_len,
                                                const uint8_t* codon_table,
                                                const uint8_t* d_frames,
                                                const uint32_t* d_hit_queries,
                                                size_t hits_per_query, const uint64_t* d_hits,
                                                size_t n_hits, sw_alignment* d_out,
                                                uint32_t* d_cigar, uint32_t cigar_stride,
                                                void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  const Pairs pr = frame_pairs(d_hit_queries, hits_per_query, d_hits, n_hits);
  sw_status st;
  if (align_opening(b, pr, stream, st, [&](sw_bank* r, void* s) {
        return sw_align_frame_hits_device(r, d_res, d_offs, d_lens, d_ids, n, max_len, codon_table,
                                          d_frames, d_hit_queries, hits_per_query, d_hits, n_hits,
                                          d_out, d_cigar, cigar_stride, s);
      }))
    return st;
  uint8_t tab[64];
  if (!swbank_codon_table(codon_table, tab))
    return fail(b, SW_ERR_ARG, "a codon table entry is no protein code (>= %d)", SW_PROTEIN_ALPHA);
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if ((st = align_ready(b, true)) != SW_OK) return st;
  if (!d_frames) return fail(b, SW_ERR_ARG, "frame alignments need the frames of the pairs");
  if (n_hits == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_out || n == 0)
    return fail(b, SW_ERR_ARG, "null device buffer or an empty batch");
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  if (d_cigar && cigar_stride && (uint64_t)n_hits * cigar_stride > 0xFFFFFFFFull)
    return fail(b, SW_ERR_ARG, "n_hits x cigar_stride must fit 32 bits (cigar_offset)");
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  // one translated hit per slot of the scratch, at the stride of the longest frame
  const uint32_t cap = max_len / 3;
  const SlicePlan hp{align16(cap) + 16, n_hits, 1};
  const size_t nq = query_count(b);
  // the previous call's use of the scratch, on whichever stream it ran
  if ((st = scratch_event(b, b->ev_frame, hs)) != SW_OK) return st;
  if ((st = slice_reserve(b, b->fr_hits, hp, 0, hs)) != SW_OK) return st;
  HIPOK(b, b->fr_hit_lens.reserve(n_hits));
  HIPOK(b, b->fr_hit_q.reserve(n_hits));
  st = timed_on(b, hs, [&] {
    return swk_translate_hits(d_res, d_offs, d_lens, n, nq, d_frames, d_hit_queries,
                              hits_per_query, d_hits, n_hits, tab, b->fr_hits.codes.p, hp.stride,
                              cap, b->fr_hits.offs.p, b->fr_hit_lens.p, b->fr_hit_q.p, hs);
  });
  if (st == SW_OK)
    st = device_call(b, b->fr_hits.codes.p, b->fr_hits.offs.p, b->fr_hit_lens.p, nullptr, n_hits,
                     cap, frame_pairs(b->fr_hit_q.p, 0, nullptr, n_hits), d_out, d_cigar,
                     cigar_stride, hs);
  if (st == SW_OK) {
    HIPOK(b, hipSetDevice(b->device));
    st = timed_on(b, hs, [&] {
      return swk_frame_fixup(d_out, d_lens, d_ids, n, nq, d_frames, d_hit_queries, hits_per_query,
                             d_hits, n_hits, hs);
    });
  }
  // whatever was launched uses the scratch: the next call is ordered after it in any case
  const hipError_t er = hipEventRecord(b->ev_frame, hs);
  if (st != SW_OK) return st;
  HIPOK(b, er);
  return SW_OK;
}

extern "C" sw_status sw_align_frame_hits(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                         const uint64_t* offsets, const uint32_t* lens,
                                         const uint64_t* ids, size_t n, const uint8_t* codon_table,
                                         const uint8_t* frames, const uint32_t* hit_queries,
                                         size_t hits_per_query, const uint64_t* hits,
                                         size_t n_hits, sw_alignment* out, uint32_t* cigar,
                                         size_t cigar_cap, size_t* cigar_used) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (cigar_used) *cigar_used = 0;
  const Pairs pr = frame_pairs(hit_queries, hits_per_query, hits, n_hits);
  sw_status st;
  if (align_opening(b, pr, nullptr, st, [&](sw_bank* r, void*) {  // (hit lists are small)
        return sw_align_frame_hits(r, residues, residues_len, offsets, lens, ids, n, codon_table,
                                   frames, hit_queries, hits_per_query, hits, n_hits, out, cigar,
                                   cigar_cap, cigar_used);
      }))
    return st;
  uint8_t tab[64];
  if (!swbank_codon_table(codon_table, tab))
    return fail(b, SW_ERR_ARG, "a codon table entry is no protein code (>= %d)", SW_PROTEIN_ALPHA);
  if ((st = align_ready(b, true)) != SW_OK) return st;
  if (!frames) return fail(b, SW_ERR_ARG, "frame alignments need the frames of the pairs");
  if (n_hits == 0) return SW_OK;
  if (!offsets || !lens || !out) return fail(b, SW_ERR_ARG, "null host buffer");
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  // the listed hits, translated: hit h is target h of a protein batch against query hq[h]
  const size_t nq = query_count(b);
  std::vector<uint64_t> toffs(n_hits);
  std::vector<uint32_t> tlens(n_hits, 0), hq(n_hits, SW_QUERY_NONE), hf(n_hits, 0);
  std::vector<uint8_t> tres;
  for (size_t h = 0; h < n_hits; ++h) {
    toffs[h] = tres.size();
    const uint64_t t = target_of(pr, h);
    const uint32_t qi = hit_queries ? hit_queries[h] : (uint32_t)(h / hits_per_query);
    if (qi != SW_QUERY_NONE && qi >= nq)
      return fail(b, SW_ERR_ARG, "hit %zu: query %u >= nq = %zu", h, qi, nq);
    if (t == SW_HIT_NONE) continue;
    if (t >= n)
      return fail(b, SW_ERR_ARG, "hit %zu: target %llu >= n = %zu", h, (unsigned long long)t, n);
    if (qi == SW_QUERY_NONE) continue;
    const uint32_t f = frames[(size_t)qi * n + t];
    if (f >= SW_FRAME_COUNT) return fail(b, SW_ERR_ARG, "hit %zu: frame %u > 5", h, f);
    const uint64_t o = offsets[t], l = lens[t];
    if (l && (!residues || o > residues_len || l > residues_len - o))
      return fail(b, SW_ERR_ARG, "target %llu outside the residues", (unsigned long long)t);
    for (uint64_t i = 0; i < l; ++i)
      if (residues[o + i] >= SW_DNA_ALPHA)
        return fail(b, SW_ERR_ARG, "target %llu code %u at %llu is no DNA code",
                    (unsigned long long)t, residues[o + i], (unsigned long long)i);
    hq[h] = qi;
    hf[h] = f;
    tres.resize(tres.size() + l / 3);
    tlens[h] = l ? (uint32_t)sw_translate_codes(residues + o, l, f, tab, tres.data() + toffs[h]) : 0;
    tres.resize(toffs[h] + tlens[h]);
  }
  if (tres.empty()) tres.push_back(0);
  st = host_call(b, tres.data(), tres.size(), toffs.data(), tlens.data(), nullptr, n_hits,
                 frame_pairs(hq.data(), 0, nullptr, n_hits), out, cigar, cigar_cap, cigar_used);
  if (st != SW_OK) return st;
  for (size_t h = 0; h < n_hits; ++h) {
    if (out[h].flags & SW_ALIGN_NO_HIT) continue;  // (index = id = SW_HIT_NONE)
    const uint64_t t = target_of(pr, h);
    out[h].index = t;
    out[h].id = ids ? ids[t] : t;
    frame_record(out[h], hf[h], lens[t]);
  }
  return SW_OK;
}

// ---- alignments of frameshift hits -------------------------------------------
// Hit h (query i, target k) is aligned over the three frames of the better strand of its DNA
// target by the kernels of swbank_kfsalign.hip, which read the batch as it lies and write the
// whole record (strand, frame, nucleotide coordinates) themselves; the pair list, the chunks of
// the direction store and the host form's staging are the code above.
namespace {

// The launch block over a batch and a pair list already on the device.
SwkFsAlign fshift_block(sw_bank* b, const uint8_t tab[64], int32_t frameshift,
                        const uint8_t* d_res, const uint64_t* d_offs, const uint32_t* d_lens,
                        const uint64_t* d_ids, size_t n, uint32_t max_len,
                        const uint32_t* d_hit_queries, size_t hits_per_query,
                        const uint64_t* d_hits, size_t n_hits, void* d_out) {
  const size_t nq = query_count(b);
  SwkFsAlign f{};
  f.res = d_res;
  f.offs = d_offs;
  f.lens = d_lens;
  f.ids = d_ids;
  f.hits = d_hits;
  f.n_hits = n_hits;
  f.n = n;
  f.max_len = max_len;
  f.qtab = reinterpret_cast<const uint2*>(b->al_tab.p);
  f.mat = reinterpret_cast<const int8_t*>(b->al_tab.p + nq * sizeof(uint2));
  f.query = b->al_tab.p + nq * sizeof(uint2) + b->matrix.size();
  f.nq = (uint32_t)nq;
  f.qlen = (uint32_t)b->query.size();  // (a set: its longest query)
  f.alpha = (uint32_t)b->alpha;
  f.hit_queries = d_hit_queries;
  f.hits_per_query = (uint32_t)hits_per_query;
  std::memcpy(f.table, tab, 64);
  f.o = b->gap_open + b->gap_extend;
  f.e = b->gap_extend;
  f.fs = frameshift;
  f.out = d_out;
  return f;
}

// The bank after the opening checks: prepare()d, the queries' table on the device.
sw_status fshift_ready(sw_bank* b, const char* what) {
  sw_status st = prepare(b);
  if (st != SW_OK) return st;
  if ((size_t)b->alpha * b->alpha != b->matrix.size() || b->alpha > SW_PROTEIN_ALPHA)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: alphabet %d too large", what, b->alpha);
  return prepare_align(b);
}

// Pass A packs a lane's best cell as step << 4 | row: strands of less than 2^29 codes.
constexpr uint32_t FSALIGN_MAX_LEN = (1u << 29) - 1;

void name_fshift(sw_bank* b, size_t hits, size_t chunks) {
  snprintf(b->last_kernel, sizeof(b->last_kernel), "align-fshift i32 nq=%zu hits=%zu chunks=%zu",
           query_count(b), hits, chunks);
}

}  // namespace

extern "C" sw_status sw_align_fshift_hits_device(sw_bank* b, const uint8_t* d_res,
                                                 const uint64_t* d_offs, const uint32_t* d_lens,
                                                 const uint64_t* d_ids, size_t n, uint32_t max_len,
                                                 const uint8_t* codon_table, int32_t frameshift,
                                                 const uint32_t* d_hit_queries,
                                                 size_t hits_per_query, const uint64_t* d_hits,
                                                 size_t n_hits, sw_alignment* d_out,
                                                 uint32_t* d_cigar, uint32_t cigar_stride,
                                                 void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  uint8_t tab[64];
  sw_status st = fshift_opening(b, "sw_align_fshift_hits_device", codon_table, frameshift, tab);
  if (st != SW_OK) return st;
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_align_fshift_hits_device(r, d_res, d_offs, d_lens, d_ids, n, max_len,
                                           codon_table, frameshift, d_hit_queries, hits_per_query,
                                           d_hits, n_hits, d_out, d_cigar, cigar_stride, s);
      }))
    return st;
  if ((st = fshift_ready(b, "sw_align_fshift_hits_device")) != SW_OK) return st;
  if (n_hits == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_out || n == 0)
    return fail(b, SW_ERR_ARG, "null device buffer or an empty batch");
  const Pairs pr{true, d_hit_queries, hits_per_query, d_hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  if (d_cigar && cigar_stride && (uint64_t)n_hits * cigar_stride > 0xFFFFFFFFull)
    return fail(b, SW_ERR_ARG, "n_hits x cigar_stride must fit 32 bits (cigar_offset)");
  if (max_len > FSALIGN_MAX_LEN)
    return fail(b, SW_ERR_UNSUPPORTED, "sw_align_fshift_hits_device: max_len %u (at most %u)",
                max_len, FSALIGN_MAX_LEN);
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  SwkFsAlign f = fshift_block(b, tab, frameshift, d_res, d_offs, d_lens, d_ids, n, max_len,
                              d_hit_queries, hits_per_query, d_hits, n_hits, d_out);
  f.cigar = d_cigar;
  f.cigar_stride = d_cigar ? cigar_stride : 0;
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_used, 0));   // bank scratch is free
  st = timed_on(b, hs, [&] { return swk_launch_fsalign_ends(&f, hs); });
  size_t chunks = 0;
  if (st == SW_OK && f.cigar_stride) {
    const uint64_t slot = swk_fsalign_dir_dwords(f.qlen, f.qlen, max_len >= 3 ? max_len - 2 : 0);
    st = paths_in_slots(b, n_hits, slot, hs, chunks, [&](size_t h0, size_t count) {
      return swk_launch_fsalign_paths(&f, nullptr, h0, count, nullptr, slot, b->al_dirs.p, hs);
    });
  }
  // whatever was launched reads the table and the scratch: the next use is ordered after it
  const hipError_t er = hipEventRecord(b->ev_used, hs);
  if (st != SW_OK) return st;
  HIPOK(b, er);
  name_fshift(b, n_hits, chunks);
  return SW_OK;
}

extern "C" sw_status sw_align_fshift_hits(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                          const uint64_t* offsets, const uint32_t* lens,
                                          const uint64_t* ids, size_t n,
                                          const uint8_t* codon_table, int32_t frameshift,
                                          const uint32_t* hit_queries, size_t hits_per_query,
                                          const uint64_t* hits, size_t n_hits, sw_alignment* out,
                                          uint32_t* cigar, size_t cigar_cap, size_t* cigar_used) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (cigar_used) *cigar_used = 0;
  uint8_t tab[64];
  sw_status st = fshift_opening(b, "sw_align_fshift_hits", codon_table, frameshift, tab);
  if (st != SW_OK) return st;
  if (on_root(b, nullptr, st, [&](sw_bank* r, void*) {  // (hit lists are small)
        return sw_align_fshift_hits(r, residues, residues_len, offsets, lens, ids, n, codon_table,
                                    frameshift, hit_queries, hits_per_query, hits, n_hits, out,
                                    cigar, cigar_cap, cigar_used);
      }))
    return st;
  if ((st = fshift_ready(b, "sw_align_fshift_hits")) != SW_OK) return st;
  if (n_hits == 0) return SW_OK;
  if (!offsets || !lens || !out) return fail(b, SW_ERR_ARG, "null host buffer");
  const Pairs pr{true, hit_queries, hits_per_query, hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  Gathered g;
  if ((st = gather_hits(b, residues, residues_len, offsets, lens, n, pr, g)) != SW_OK) return st;
  for (size_t h = 0; h < n_hits; ++h)  // (the gathering knows the bank's protein alphabet)
    for (uint32_t i = 0; i < g.lens[h]; ++i)
      if (g.res[g.offs[h] + i] >= SW_DNA_ALPHA)
        return fail(b, SW_ERR_ARG, "target %llu code %u at %u is no DNA code",
                    (unsigned long long)target_of(pr, h), g.res[g.offs[h] + i], i);
  if (g.max_len > FSALIGN_MAX_LEN)
    return fail(b, SW_ERR_UNSUPPORTED, "sw_align_fshift_hits: a target of %u codes (at most %u)",
                g.max_len, FSALIGN_MAX_LEN);
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = b->stream;
  SwkAlign p{};  // (the staged buffers only: no launch block, no scratch rows)
  if ((st = stage_hits(b, pr, g, p, hs, false)) != SW_OK) return st;
  // hit h is target h of the gathered batch against query al_hq[h]
  SwkFsAlign f = fshift_block(b, tab, frameshift, p.res, p.offs, p.lens, nullptr, n_hits,
                              g.max_len, p.hit_queries, 0, nullptr, n_hits, p.out);
  size_t chunks = 0;
  st = host_passes(
      b, pr, g, ids, hs, [&](hipStream_t s) { return swk_launch_fsalign_ends(&f, s); },
      [&](const uint32_t* list, size_t count, const SwkAlignPlan* plan, hipStream_t s) {
        f.cigar = b->al_cig.p;
        f.cigar_stride = 1;  // (places come from the plan)
        return swk_launch_fsalign_paths(&f, list, 0, count, plan, 0, b->al_dirs.p, s);
      },
      [&](uint32_t Q, uint32_t L) {  // (L nucleotides hold L - 2 codon starts)
        return swk_fsalign_dir_dwords(f.qlen, Q, L >= 3 ? L - 2 : 0);
      },
      out, cigar, cigar_cap, cigar_used, chunks);
  if (st != SW_OK) return st;
  name_fshift(b, n_hits, chunks);
  return SW_OK;
}

// ---- alignments of global-local hits -----------------------------------------
// Hit h (query i, target k) is aligned as sw_score_glocal scores it, by the kernels of
// swbank_kglalign.hip, which read the batch as it lies and write the whole record (strand, the
// forward target's coordinates) themselves; the pair list, the chunks of the direction store and
// the host form's staging are the code above.
namespace {

// The launch block over a batch and a pair list already on the device.
SwkGlAlign glocal_block(sw_bank* b, int32_t ends, int32_t both_strands, const uint8_t* d_res,
                        const uint64_t* d_offs, const uint32_t* d_lens, const uint64_t* d_ids,
                        size_t n, uint32_t max_len, const uint32_t* d_hit_queries,
                        size_t hits_per_query, const uint64_t* d_hits, size_t n_hits,
                        void* d_out) {
  const size_t nq = query_count(b);
  SwkGlAlign f{};
  f.res = d_res;
  f.offs = d_offs;
  f.lens = d_lens;
  f.ids = d_ids;
  f.hits = d_hits;
  f.n_hits = n_hits;
  f.n = n;
  f.max_len = max_len;
  f.qtab = reinterpret_cast<const uint2*>(b->al_tab.p);
  f.mat = reinterpret_cast<const int8_t*>(b->al_tab.p + nq * sizeof(uint2));
  f.query = b->al_tab.p + nq * sizeof(uint2) + b->matrix.size();
  f.nq = (uint32_t)nq;
  f.qlen = (uint32_t)b->query.size();  // (a set: its longest query)
  f.alpha = (uint32_t)b->alpha;
  f.hit_queries = d_hit_queries;
  f.hits_per_query = (uint32_t)hits_per_query;
  f.o = b->gap_open + b->gap_extend;
  f.e = b->gap_extend;
  f.ends = ends;
  f.both = both_strands ? 1 : 0;
  f.out = d_out;
  return f;
}

// The bank after the argument checks: prepare()d, inside the range rule of sw_score_glocal for
// targets of at most max_len codes, the queries' table on the device.  The rule bounds every cell
// of a matrix of at most 1,024 rows and max_len columns with penalised boundaries; the reversed
// walk of pass B and the window of pass C are such matrices (both boundaries penalised, which is
// the case the rule is stated for), so it covers them.
sw_status glocal_ready(sw_bank* b, const char* what, uint32_t max_len) {
  sw_status st = prepare(b);
  if (st != SW_OK) return st;
  if (!glocal_in_range(b, max_len))
    return fail(b, SW_ERR_RANGE,
                "%s: |open + extend| + (%d + 64 + max_len %u) x max(|extend|, 128) reaches 2^30",
                what, SW_GLOCAL_MAX_QUERY, max_len);
  if ((size_t)b->alpha * b->alpha != b->matrix.size() || b->alpha > SW_PROTEIN_ALPHA)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: alphabet %d too large", what, b->alpha);
  return prepare_align(b);
}

void name_glocal(sw_bank* b, int32_t ends, size_t hits, size_t chunks) {
  snprintf(b->last_kernel, sizeof(b->last_kernel),
           "align-glocal i32 ends=%d nq=%zu hits=%zu chunks=%zu", ends, query_count(b), hits,
           chunks);
}

}  // namespace

extern "C" sw_status sw_align_glocal_hits_device(sw_bank* b, const uint8_t* d_res,
                                                 const uint64_t* d_offs, const uint32_t* d_lens,
                                                 const uint64_t* d_ids, size_t n, uint32_t max_len,
                                                 int32_t ends, int32_t both_strands,
                                                 const uint32_t* d_hit_queries,
                                                 size_t hits_per_query, const uint64_t* d_hits,
                                                 size_t n_hits, sw_alignment* d_out,
                                                 uint32_t* d_cigar, uint32_t cigar_stride,
                                                 void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  sw_status st = glocal_opening(b, "sw_align_glocal_hits_device", ends, both_strands);
  if (st != SW_OK) return st;
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_align_glocal_hits_device(r, d_res, d_offs, d_lens, d_ids, n, max_len, ends,
                                           both_strands, d_hit_queries, hits_per_query, d_hits,
                                           n_hits, d_out, d_cigar, cigar_stride, s);
      }))
    return st;
  if (n_hits == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_out || n == 0)
    return fail(b, SW_ERR_ARG, "null device buffer or an empty batch");
  const Pairs pr{true, d_hit_queries, hits_per_query, d_hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  if (d_cigar && cigar_stride && (uint64_t)n_hits * cigar_stride > 0xFFFFFFFFull)
    return fail(b, SW_ERR_ARG, "n_hits x cigar_stride must fit 32 bits (cigar_offset)");
  if ((st = glocal_ready(b, "sw_align_glocal_hits_device", max_len)) != SW_OK) return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  SwkGlAlign f = glocal_block(b, ends, both_strands, d_res, d_offs, d_lens, d_ids, n, max_len,
                              d_hit_queries, hits_per_query, d_hits, n_hits, d_out);
  f.cigar = d_cigar;
  f.cigar_stride = d_cigar ? cigar_stride : 0;
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_used, 0));   // bank scratch is free
  st = timed_on(b, hs, [&] { return swk_launch_glalign_ends(&f, hs); });
  size_t chunks = 0;
  if (st == SW_OK && f.cigar_stride) {
    const uint64_t slot = swk_glalign_dir_dwords(f.qlen, f.qlen, max_len);
    st = paths_in_slots(b, n_hits, slot, hs, chunks, [&](size_t h0, size_t count) {
      return swk_launch_glalign_paths(&f, nullptr, h0, count, nullptr, slot, b->al_dirs.p, hs);
    });
  }
  // whatever was launched reads the table and the scratch: the next use is ordered after it
  const hipError_t er = hipEventRecord(b->ev_used, hs);
  if (st != SW_OK) return st;
  HIPOK(b, er);
  name_glocal(b, ends, n_hits, chunks);
  return SW_OK;
}

extern "C" sw_status sw_align_glocal_hits(sw_bank* b, const uint8_t* residues, size_t residues_len,
                                          const uint64_t* offsets, const uint32_t* lens,
                                          const uint64_t* ids, size_t n, int32_t ends,
                                          int32_t both_strands, const uint32_t* hit_queries,
                                          size_t hits_per_query, const uint64_t* hits,
                                          size_t n_hits, sw_alignment* out, uint32_t* cigar,
                                          size_t cigar_cap, size_t* cigar_used) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (cigar_used) *cigar_used = 0;
  sw_status st = glocal_opening(b, "sw_align_glocal_hits", ends, both_strands);
  if (st != SW_OK) return st;
  if (on_root(b, nullptr, st, [&](sw_bank* r, void*) {  // (hit lists are small)
        return sw_align_glocal_hits(r, residues, residues_len, offsets, lens, ids, n, ends,
                                    both_strands, hit_queries, hits_per_query, hits, n_hits, out,
                                    cigar, cigar_cap, cigar_used);
      }))
    return st;
  if (n_hits == 0) return SW_OK;
  if (!offsets || !lens || !out) return fail(b, SW_ERR_ARG, "null host buffer");
  const Pairs pr{true, hit_queries, hits_per_query, hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  // (alpha is the bank's before prepare(): the gathering checks the listed targets' codes)
  Gathered g;
  if ((st = gather_hits(b, residues, residues_len, offsets, lens, n, pr, g)) != SW_OK) return st;
  if ((st = glocal_ready(b, "sw_align_glocal_hits", g.max_len)) != SW_OK) return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = b->stream;
  SwkAlign p{};  // (the staged buffers only: no launch block, no scratch rows)
  if ((st = stage_hits(b, pr, g, p, hs, false)) != SW_OK) return st;
  // hit h is target h of the gathered batch against query al_hq[h]
  SwkGlAlign f = glocal_block(b, ends, both_strands, p.res, p.offs, p.lens, nullptr, n_hits,
                              g.max_len, p.hit_queries, 0, nullptr, n_hits, p.out);
  size_t chunks = 0;
  st = host_passes(
      b, pr, g, ids, hs, [&](hipStream_t s) { return swk_launch_glalign_ends(&f, s); },
      [&](const uint32_t* list, size_t count, const SwkAlignPlan* plan, hipStream_t s) {
        f.cigar = b->al_cig.p;
        f.cigar_stride = 1;  // (places come from the plan)
        return swk_launch_glalign_paths(&f, list, 0, count, plan, 0, b->al_dirs.p, s);
      },
      [&](uint32_t Q, uint32_t L) { return swk_glalign_dir_dwords(f.qlen, Q, L); }, out, cigar,
      cigar_cap, cigar_used, chunks);
  if (st != SW_OK) return st;
  name_glocal(b, ends, n_hits, chunks);
  return SW_OK;
}

// ---- non-intersecting local alignments ----------------------------------------
// Hit h (query i, target k) gets up to `rounds` records, out[h * rounds + r], from the kernel of
// swbank_klalign.hip: one launch per round over a chunk of hits, each hit with a direction store
// of its whole matrix that carries the used cells from round to round.  The pair list, the
// gathering and staging of the host form and the brackets are the code above.
namespace {

// What both entries check first, in the order of the header's list.
sw_status disjoint_opening(sw_bank* b, const char* what, uint32_t rounds, int32_t min_score) {
  if (!b->gotoh()) return fail(b, SW_ERR_UNSUPPORTED, "%s: the Gotoh gap model only", what);
  if (!root_of(b)->have_pen || !b->have_query)
    return fail(b, SW_ERR_STATE, "penalties or query not loaded");
  if (b->query.size() > SW_DISJOINT_MAX_QUERY)  // (a set: its longest query)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: a query of %zu rows (at most %d)", what,
                b->query.size(), SW_DISJOINT_MAX_QUERY);
  if (rounds < 1 || rounds > SW_DISJOINT_MAX_ROUNDS)
    return fail(b, SW_ERR_ARG, "%s: rounds = %u (1 .. %d)", what, rounds, SW_DISJOINT_MAX_ROUNDS);
  if (min_score < 1) return fail(b, SW_ERR_ARG, "%s: min_score = %d (at least 1)", what, min_score);
  return SW_OK;
}

sw_status disjoint_sizes(sw_bank* b, const char* what, size_t n_hits, uint32_t rounds,
                         uint64_t stride) {
  if ((uint64_t)n_hits * rounds > 0xFFFFFFFFull)
    return fail(b, SW_ERR_ARG, "%s: n_hits x rounds must fit 32 bits", what);
  if (stride && (uint64_t)n_hits * rounds * stride > 0xFFFFFFFFull)
    return fail(b, SW_ERR_ARG, "%s: n_hits x rounds x cigar_stride must fit 32 bits (cigar_offset)",
                what);
  return SW_OK;
}

sw_status disjoint_slot_refused(sw_bank* b, const char* what, uint64_t slot) {
  return fail(b, SW_ERR_UNSUPPORTED,
              "%s: the direction store of one hit (%llu MiB) exceeds SWBANK_ALIGN_MB", what,
              (unsigned long long)((slot * 4 + ((1u << 20) - 1)) >> 20));
}

// The bank after the argument checks: prepare()d, the queries' table on the device.
sw_status disjoint_ready(sw_bank* b, const char* what) {
  const sw_status st = prepare(b);
  if (st != SW_OK) return st;
  if ((size_t)b->alpha * b->alpha != b->matrix.size() || b->alpha > SW_PROTEIN_ALPHA)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: alphabet %d too large", what, b->alpha);
  return prepare_align(b);
}

// The launch block over a batch and a pair list already on the device.
SwkLaAlign disjoint_block(sw_bank* b, uint32_t rounds, int32_t min_score, const uint8_t* d_res,
                          const uint64_t* d_offs, const uint32_t* d_lens, const uint64_t* d_ids,
                          size_t n, uint32_t max_len, const uint32_t* d_hit_queries,
                          size_t hits_per_query, const uint64_t* d_hits, size_t n_hits,
                          void* d_out) {
  const size_t nq = query_count(b);
  SwkLaAlign f{};
  f.res = d_res;
  f.offs = d_offs;
  f.lens = d_lens;
  f.ids = d_ids;
  f.hits = d_hits;
  f.n_hits = n_hits;
  f.n = n;
  f.max_len = max_len;
  f.qtab = reinterpret_cast<const uint2*>(b->al_tab.p);
  f.mat = reinterpret_cast<const int8_t*>(b->al_tab.p + nq * sizeof(uint2));
  f.query = b->al_tab.p + nq * sizeof(uint2) + b->matrix.size();
  f.nq = (uint32_t)nq;
  f.qlen = (uint32_t)b->query.size();  // (a set: its longest query)
  f.alpha = (uint32_t)b->alpha;
  f.hit_queries = d_hit_queries;
  f.hits_per_query = (uint32_t)hits_per_query;
  f.o = b->gap_open + b->gap_extend;
  f.e = b->gap_extend;
  f.min_score = min_score;
  f.rounds = rounds;
  f.out = d_out;
  return f;
}

// The rounds of hits [h0, h0 + count), one bracket.
sw_status disjoint_rounds(sw_bank* b, const SwkLaAlign& f, size_t h0, size_t count,
                          hipStream_t hs) {
  return timed_on(b, hs, [&] {
    for (uint32_t r = 0; r < f.rounds; ++r) {
      const hipError_t e = swk_launch_lalign_round(&f, h0, count, r, hs);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  });
}

// The end of a host form: the records and the planned ops slots back from the device (al_out,
// al_cig; ncig ops slots in all); the records speak of the caller's batch, the ops are packed
// back to back in record order into cigar[0, cigar_cap).
sw_status disjoint_collect(sw_bank* b, const Pairs& pr, const uint64_t* ids,
                           const std::vector<SwkAlignPlan>& plan, uint32_t rounds, uint64_t ncig,
                           hipStream_t hs, sw_alignment* out, uint32_t* cigar, size_t cigar_cap,
                           size_t* cigar_used) {
  const size_t n_hits = pr.n_hits, n_rec = n_hits * rounds;
  std::vector<sw_alignment> recs(n_rec);
  std::vector<uint32_t> ops((size_t)ncig);
  HIPOK(b, hipMemcpyAsync(recs.data(), b->al_out.p, n_rec * sizeof(sw_alignment),
                          hipMemcpyDeviceToHost, hs));
  if (ncig)
    HIPOK(b, hipMemcpyAsync(ops.data(), b->al_cig.p, ops.size() * 4, hipMemcpyDeviceToHost, hs));
  HIPOK(b, hipStreamSynchronize(hs));
  HIPOK(b, hipEventRecord(b->ev_used, hs));
  size_t at = 0;
  for (size_t h = 0; h < n_hits; ++h) {
    const uint64_t t = target_of(pr, h);
    for (uint32_t r = 0; r < rounds; ++r) {
      sw_alignment& x = recs[h * rounds + r];
      x.cigar_offset = 0;
      if (x.flags & SW_ALIGN_NO_HIT) continue;  // (index = id = SW_HIT_NONE)
      x.index = t;
      x.id = ids ? ids[t] : t;
      if (x.flags & (SW_ALIGN_EMPTY | SW_ALIGN_NO_PATH)) continue;
      if (x.cigar_len > cigar_cap - at) {
        x.flags |= SW_ALIGN_NO_PATH;
        x.cigar_len = x.n_columns = x.n_identities = 0;
        continue;
      }
      std::memcpy(cigar + at, ops.data() + plan[h].cig_off + (uint64_t)r * plan[h].cig_cap,
                  (size_t)x.cigar_len * 4);
      x.cigar_offset = (uint32_t)at;
      at += x.cigar_len;
    }
  }
  std::memcpy(out, recs.data(), n_rec * sizeof(sw_alignment));
  if (cigar_used) *cigar_used = at;
  return SW_OK;
}

void name_disjoint(sw_bank* b, uint32_t rounds, size_t hits, size_t chunks) {
  snprintf(b->last_kernel, sizeof(b->last_kernel),
           "align-disjoint i32 rounds=%u nq=%zu hits=%zu chunks=%zu", rounds, query_count(b), hits,
           chunks);
}

}  // namespace

extern "C" sw_status sw_align_disjoint_hits_device(sw_bank* b, const uint8_t* d_res,
                                                   const uint64_t* d_offs, const uint32_t* d_lens,
                                                   const uint64_t* d_ids, size_t n,
                                                   uint32_t max_len, uint32_t rounds,
                                                   int32_t min_score,
                                                   const uint32_t* d_hit_queries,
                                                   size_t hits_per_query, const uint64_t* d_hits,
                                                   size_t n_hits, sw_alignment* d_out,
                                                   uint32_t* d_cigar, uint32_t cigar_stride,
                                                   void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  const char* what = "sw_align_disjoint_hits_device";
  sw_status st = disjoint_opening(b, what, rounds, min_score);
  if (st != SW_OK) return st;
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_align_disjoint_hits_device(r, d_res, d_offs, d_lens, d_ids, n, max_len, rounds,
                                             min_score, d_hit_queries, hits_per_query, d_hits,
                                             n_hits, d_out, d_cigar, cigar_stride, s);
      }))
    return st;
  if (n_hits == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_out || n == 0)
    return fail(b, SW_ERR_ARG, "null device buffer or an empty batch");
  const Pairs pr{true, d_hit_queries, hits_per_query, d_hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  if ((st = disjoint_sizes(b, what, n_hits, rounds, d_cigar ? cigar_stride : 0)) != SW_OK)
    return st;
  // every slot holds the matrix of the longest query against max_len columns (a pair with no
  // cell takes none)
  const uint64_t slot = std::max<uint64_t>(
      swk_lalign_dir_dwords((uint32_t)b->query.size(), (uint32_t)b->query.size(), max_len), 64);
  const uint64_t budget = dir_budget();
  if (slot > budget) return disjoint_slot_refused(b, what, slot);
  if ((st = disjoint_ready(b, what)) != SW_OK) return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  const size_t per = (size_t)std::min<uint64_t>(budget / slot, n_hits);
  HIPOK(b, b->al_dirs.reserve((size_t)(slot * per)));
  SwkLaAlign f = disjoint_block(b, rounds, min_score, d_res, d_offs, d_lens, d_ids, n, max_len,
                                d_hit_queries, hits_per_query, d_hits, n_hits, d_out);
  f.cigar = d_cigar;
  f.cigar_stride = d_cigar ? cigar_stride : 0;
  f.slot = slot;
  f.dirs = b->al_dirs.p;
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_used, 0));   // bank scratch is free
  size_t chunks = 0;
  for (size_t h0 = 0; st == SW_OK && h0 < n_hits; h0 += per, ++chunks)
    st = disjoint_rounds(b, f, h0, std::min(per, n_hits - h0), hs);
  // whatever was launched reads the table and the scratch: the next use is ordered after it
  const hipError_t er = hipEventRecord(b->ev_used, hs);
  if (st != SW_OK) return st;
  HIPOK(b, er);
  name_disjoint(b, rounds, n_hits, chunks);
  return SW_OK;
}

extern "C" sw_status sw_align_disjoint_hits(sw_bank* b, const uint8_t* residues,
                                            size_t residues_len, const uint64_t* offsets,
                                            const uint32_t* lens, const uint64_t* ids, size_t n,
                                            uint32_t rounds, int32_t min_score,
                                            const uint32_t* hit_queries, size_t hits_per_query,
                                            const uint64_t* hits, size_t n_hits,
                                            sw_alignment* out, uint32_t* cigar, size_t cigar_cap,
                                            size_t* cigar_used) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (cigar_used) *cigar_used = 0;
  const char* what = "sw_align_disjoint_hits";
  sw_status st = disjoint_opening(b, what, rounds, min_score);
  if (st != SW_OK) return st;
  if (on_root(b, nullptr, st, [&](sw_bank* r, void*) {  // (hit lists are small)
        return sw_align_disjoint_hits(r, residues, residues_len, offsets, lens, ids, n, rounds,
                                      min_score, hit_queries, hits_per_query, hits, n_hits, out,
                                      cigar, cigar_cap, cigar_used);
      }))
    return st;
  if (n_hits == 0) return SW_OK;
  if (!offsets || !lens || !out || n == 0) return fail(b, SW_ERR_ARG, "null host buffer or n = 0");
  const Pairs pr{true, hit_queries, hits_per_query, hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  // (alpha is the bank's before prepare(): the gathering checks the listed targets' codes)
  Gathered g;
  if ((st = gather_hits(b, residues, residues_len, offsets, lens, n, pr, g)) != SW_OK) return st;
  if ((st = disjoint_sizes(b, what, n_hits, rounds, 0)) != SW_OK) return st;
  // every hit's store and ops slots from its own rows and columns; the chunks that fit the budget
  cigar_cap = std::min<size_t>(cigar_cap, 0xFFFFFFFFu);  // (cigar_offset is 32 bits)
  const bool with_cigar = cigar && cigar_cap;
  const size_t nq = query_count(b);
  const std::vector<uint8_t>* queries = nq > 1 ? b->qset.data() : &b->query;
  const uint64_t budget = dir_budget();
  std::vector<SwkAlignPlan> plan(n_hits);
  std::vector<size_t> cut{0};
  uint64_t used = 0, most = 64, ncig = 0;
  for (size_t h = 0; h < n_hits; ++h) {
    const uint32_t m = g.q[h] == SW_QUERY_NONE ? 0u : (uint32_t)queries[g.q[h]].size();
    const uint32_t L = g.lens[h];
    const uint64_t need = swk_lalign_dir_dwords((uint32_t)b->query.size(), m, L);
    if (need > budget) return disjoint_slot_refused(b, what, need);
    if (used + need > budget) {
      cut.push_back(h);
      used = 0;
    }
    // (runs of M alternate with gap runs, and an M run takes a row and a column)
    const uint32_t cap = with_cigar && m && L ? 2 * std::min(m, L) - 1 : 0u;
    plan[h] = SwkAlignPlan{used, need, ncig, cap, 0};
    used += need;
    most = std::max(most, used);
    ncig += (uint64_t)cap * rounds;
  }
  cut.push_back(n_hits);
  if ((st = disjoint_ready(b, what)) != SW_OK) return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = b->stream;
  const size_t n_rec = n_hits * rounds;
  HIPOK(b, b->al_out.reserve(n_rec));  // (before the staging takes its address)
  SwkAlign p{};  // (the staged buffers only: no launch block, no scratch rows)
  if ((st = stage_hits(b, pr, g, p, hs, false)) != SW_OK) return st;
  HIPOK(b, b->al_dirs.reserve((size_t)most));
  HIPOK(b, b->al_cig.reserve((size_t)std::max<uint64_t>(ncig, 1)));
  HIPOK(b, b->al_plan.reserve(n_hits));
  HIPOK(b, hipMemcpyAsync(b->al_plan.p, plan.data(), n_hits * sizeof(SwkAlignPlan),
                          hipMemcpyHostToDevice, hs));
  // hit h is target h of the gathered batch against query al_hq[h]
  SwkLaAlign f = disjoint_block(b, rounds, min_score, p.res, p.offs, p.lens, nullptr, n_hits,
                                g.max_len, p.hit_queries, 0, nullptr, n_hits, b->al_out.p);
  f.cigar = with_cigar ? b->al_cig.p : nullptr;
  f.cigar_stride = 0;
  f.plan = b->al_plan.p;
  f.dirs = b->al_dirs.p;
  size_t chunks = 0;
  for (size_t c = 0; st == SW_OK && c + 1 < cut.size(); ++c) {
    if (cut[c + 1] == cut[c]) continue;
    st = disjoint_rounds(b, f, cut[c], cut[c + 1] - cut[c], hs);
    ++chunks;
  }
  if (st != SW_OK) {
    (void)hipStreamSynchronize(hs);  // (the uploads have left the host vectors)
    (void)hipEventRecord(b->ev_used, hs);
    return st;
  }
  if ((st = disjoint_collect(b, pr, ids, plan, rounds, ncig, hs, out, cigar, cigar_cap,
                             cigar_used)) != SW_OK)
    return st;
  name_disjoint(b, rounds, n_hits, chunks);
  return SW_OK;
}

// ---- non-intersecting alignments over the six reading frames -------------------
// Hit h (protein query i, DNA target k) gets up to `rounds` records, out[h * rounds + r], from the
// kernels of swbank_klaframes.hip: the merge, best first, of the non-intersecting alignments of
// the query with each of the target's six translations.  A hit's direction store holds its six
// matrices back to back; its six pending candidates live in al_state.  Everything else is the
// code of the disjoint entries above.
namespace {

// What both entries check first, in the order of the header's list.
sw_status disjoint_frames_opening(sw_bank* b, const char* what, const uint8_t* codon_table,
                                  uint32_t rounds, int32_t min_score, uint8_t tab[64]) {
  if (b->cfg.alphabet != SW_ALPHABET_PROTEIN)
    return fail(b, SW_ERR_UNSUPPORTED, "%s: protein banks only", what);
  const sw_status st = disjoint_opening(b, what, rounds, min_score);
  if (st != SW_OK) return st;
  if (!swbank_codon_table(codon_table, tab))
    return fail(b, SW_ERR_ARG, "a codon table entry is no protein code (>= %d)", SW_PROTEIN_ALPHA);
  return SW_OK;
}

// The rounds of hits [h0, h0 + count), one bracket.
sw_status disjoint_frames_rounds(sw_bank* b, const SwkLaFrames& f, size_t h0, size_t count,
                                 hipStream_t hs) {
  return timed_on(b, hs, [&] {
    for (uint32_t r = 0; r < f.a.rounds; ++r) {
      const hipError_t e = swk_launch_laframes_round(&f, h0, count, r, hs);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  });
}

void name_disjoint_frames(sw_bank* b, uint32_t rounds, size_t hits, size_t chunks) {
  snprintf(b->last_kernel, sizeof(b->last_kernel),
           "align-disjoint-frames i32 rounds=%u nq=%zu hits=%zu chunks=%zu", rounds,
           query_count(b), hits, chunks);
}

}  // namespace

extern "C" sw_status sw_align_disjoint_frame_hits_device(
    sw_bank* b, const uint8_t* d_res, const uint64_t* d_offs, const uint32_t* d_lens,
    const uint64_t* d_ids, size_t n, uint32_t max_len, const uint8_t* codon_table, uint32_t rounds,
    int32_t min_score, const uint32_t* d_hit_queries, size_t hits_per_query,
    const uint64_t* d_hits, size_t n_hits, sw_alignment* d_out, uint32_t* d_cigar,
    uint32_t cigar_stride, void* stream) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  const char* what = "sw_align_disjoint_frame_hits_device";
  SwkLaFrames f{};
  sw_status st = disjoint_frames_opening(b, what, codon_table, rounds, min_score, f.table);
  if (st != SW_OK) return st;
  // a hand-off fault latched by an earlier device call is returned before anything runs
  if (const sw_status fs = take_fault(b, 0); fs != SW_OK) return fs;
  if (on_root(b, stream, st, [&](sw_bank* r, void* s) {
        return sw_align_disjoint_frame_hits_device(r, d_res, d_offs, d_lens, d_ids, n, max_len,
                                                   codon_table, rounds, min_score, d_hit_queries,
                                                   hits_per_query, d_hits, n_hits, d_out, d_cigar,
                                                   cigar_stride, s);
      }))
    return st;
  if (n_hits == 0) return SW_OK;
  if (!d_res || !d_offs || !d_lens || !d_out || n == 0)
    return fail(b, SW_ERR_ARG, "null device buffer or an empty batch");
  const Pairs pr{true, d_hit_queries, hits_per_query, d_hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  if ((st = disjoint_sizes(b, what, n_hits, rounds, d_cigar ? cigar_stride : 0)) != SW_OK)
    return st;
  // every slot holds six matrices of the longest query against the codons of max_len codes
  const uint64_t slot = std::max<uint64_t>(
      6 * swk_lalign_dir_dwords((uint32_t)b->query.size(), (uint32_t)b->query.size(), max_len / 3),
      64);
  const uint64_t budget = dir_budget();
  if (slot > budget) return disjoint_slot_refused(b, what, slot);
  if ((st = disjoint_ready(b, what)) != SW_OK) return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = stream_or(b, stream);
  const size_t per = (size_t)std::min<uint64_t>(budget / slot, n_hits);
  HIPOK(b, b->al_dirs.reserve((size_t)(slot * per)));
  HIPOK(b, b->al_state.reserve(per * SWK_LAFRAMES_STATE));
  f.a = disjoint_block(b, rounds, min_score, d_res, d_offs, d_lens, d_ids, n, max_len,
                       d_hit_queries, hits_per_query, d_hits, n_hits, d_out);
  f.a.cigar = d_cigar;
  f.a.cigar_stride = d_cigar ? cigar_stride : 0;
  f.a.slot = slot;
  f.a.dirs = b->al_dirs.p;
  f.state = b->al_state.p;
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_ready, 0));  // the queries' codes are uploaded
  HIPOK(b, hipStreamWaitEvent(hs, b->ev_used, 0));   // bank scratch is free
  size_t chunks = 0;
  for (size_t h0 = 0; st == SW_OK && h0 < n_hits; h0 += per, ++chunks)
    st = disjoint_frames_rounds(b, f, h0, std::min(per, n_hits - h0), hs);
  // whatever was launched reads the table and the scratch: the next use is ordered after it
  const hipError_t er = hipEventRecord(b->ev_used, hs);
  if (st != SW_OK) return st;
  HIPOK(b, er);
  name_disjoint_frames(b, rounds, n_hits, chunks);
  return SW_OK;
}

extern "C" sw_status sw_align_disjoint_frame_hits(
    sw_bank* b, const uint8_t* residues, size_t residues_len, const uint64_t* offsets,
    const uint32_t* lens, const uint64_t* ids, size_t n, const uint8_t* codon_table,
    uint32_t rounds, int32_t min_score, const uint32_t* hit_queries, size_t hits_per_query,
    const uint64_t* hits, size_t n_hits, sw_alignment* out, uint32_t* cigar, size_t cigar_cap,
    size_t* cigar_used) {
  DevGuard dev_guard(b);  // on the bank's device; the caller's is restored on return (ABI 6)
  if (!b) return SW_ERR_ARG;
  if (cigar_used) *cigar_used = 0;
  const char* what = "sw_align_disjoint_frame_hits";
  SwkLaFrames f{};
  sw_status st = disjoint_frames_opening(b, what, codon_table, rounds, min_score, f.table);
  if (st != SW_OK) return st;
  if (on_root(b, nullptr, st, [&](sw_bank* r, void*) {  // (hit lists are small)
        return sw_align_disjoint_frame_hits(r, residues, residues_len, offsets, lens, ids, n,
                                            codon_table, rounds, min_score, hit_queries,
                                            hits_per_query, hits, n_hits, out, cigar, cigar_cap,
                                            cigar_used);
      }))
    return st;
  if (n_hits == 0) return SW_OK;
  if (!offsets || !lens || !out || n == 0) return fail(b, SW_ERR_ARG, "null host buffer or n = 0");
  const Pairs pr{true, hit_queries, hits_per_query, hits, n_hits};
  if ((st = check_pairs(b, pr, n)) != SW_OK) return st;
  Gathered g;
  if ((st = gather_hits(b, residues, residues_len, offsets, lens, n, pr, g)) != SW_OK) return st;
  for (size_t h = 0; h < n_hits; ++h)  // (the gathering knows the bank's protein alphabet)
    for (uint32_t i = 0; i < g.lens[h]; ++i)
      if (g.res[g.offs[h] + i] >= SW_DNA_ALPHA)
        return fail(b, SW_ERR_ARG, "target %llu code %u at %u is no DNA code",
                    (unsigned long long)target_of(pr, h), g.res[g.offs[h] + i], i);
  if ((st = disjoint_sizes(b, what, n_hits, rounds, 0)) != SW_OK) return st;
  // every hit's six stores from its own rows and codons, its ops slots from the longest frame's
  // codons; the chunks that fit the budget
  cigar_cap = std::min<size_t>(cigar_cap, 0xFFFFFFFFu);  // (cigar_offset is 32 bits)
  const bool with_cigar = cigar && cigar_cap;
  const size_t nq = query_count(b);
  const std::vector<uint8_t>* queries = nq > 1 ? b->qset.data() : &b->query;
  const uint64_t budget = dir_budget();
  std::vector<SwkAlignPlan> plan(n_hits);
  std::vector<size_t> cut{0};
  uint64_t used = 0, most = 64, ncig = 0;
  size_t widest = 1;
  for (size_t h = 0; h < n_hits; ++h) {
    const uint32_t m = g.q[h] == SW_QUERY_NONE ? 0u : (uint32_t)queries[g.q[h]].size();
    const uint32_t L = g.lens[h];
    const uint64_t need = swk_laframes_dir_dwords((uint32_t)b->query.size(), m, L);
    if (need > budget) return disjoint_slot_refused(b, what, need);
    if (used + need > budget) {
      widest = std::max(widest, h - cut.back());
      cut.push_back(h);
      used = 0;
    }
    // (runs of M alternate with gap runs, and an M run takes a row and a column)
    const uint32_t cap = with_cigar && m && L / 3 ? 2 * std::min(m, L / 3) - 1 : 0u;
    plan[h] = SwkAlignPlan{used, need, ncig, cap, 0};
    used += need;
    most = std::max(most, used);
    ncig += (uint64_t)cap * rounds;
  }
  widest = std::max(widest, n_hits - cut.back());
  cut.push_back(n_hits);
  if ((st = disjoint_ready(b, what)) != SW_OK) return st;
  HIPOK(b, hipSetDevice(b->device));
  hipStream_t hs = b->stream;
  const size_t n_rec = n_hits * rounds;
  HIPOK(b, b->al_out.reserve(n_rec));  // (before the staging takes its address)
  SwkAlign p{};  // (the staged buffers only: no launch block, no scratch rows)
  if ((st = stage_hits(b, pr, g, p, hs, false)) != SW_OK) return st;
  HIPOK(b, b->al_dirs.reserve((size_t)most));
  HIPOK(b, b->al_state.reserve(widest * SWK_LAFRAMES_STATE));
  HIPOK(b, b->al_cig.reserve((size_t)std::max<uint64_t>(ncig, 1)));
  HIPOK(b, b->al_plan.reserve(n_hits));
  HIPOK(b, hipMemcpyAsync(b->al_plan.p, plan.data(), n_hits * sizeof(SwkAlignPlan),
                          hipMemcpyHostToDevice, hs));
  // hit h is target h of the gathered batch against query al_hq[h]
  f.a = disjoint_block(b, rounds, min_score, p.res, p.offs, p.lens, nullptr, n_hits, g.max_len,
                       p.hit_queries, 0, nullptr, n_hits, b->al_out.p);
  f.a.cigar = with_cigar ? b->al_cig.p : nullptr;
  f.a.cigar_stride = 0;
  f.a.plan = b->al_plan.p;
  f.a.dirs = b->al_dirs.p;
  f.state = b->al_state.p;
  size_t chunks = 0;
  for (size_t c = 0; st == SW_OK && c + 1 < cut.size(); ++c) {
    if (cut[c + 1] == cut[c]) continue;
    st = disjoint_frames_rounds(b, f, cut[c], cut[c + 1] - cut[c], hs);
    ++chunks;
  }
  if (st != SW_OK) {
    (void)hipStreamSynchronize(hs);  // (the uploads have left the host vectors)
    (void)hipEventRecord(b->ev_used, hs);
    return st;
  }
  if ((st = disjoint_collect(b, pr, ids, plan, rounds, ncig, hs, out, cigar, cigar_cap,
                             cigar_used)) != SW_OK)
    return st;
  name_disjoint_frames(b, rounds, n_hits, chunks);
  return SW_OK;
}
