// swbank_kglalign.hip — the kernels behind the alignments of global-local hits (include/swbank.h
// "alignments of global-local hits").
//
// One workgroup per hit.  Every pass but the last is the walk of swbank_kglwalk.h, which the score
// kernel runs too, so a record's score, end and strand are the score call's by construction.  A
// query has at most 64 x 16 rows, so there are no strips and no scratch rows.  What differs per
// pass is which rows and columns the walk sees and what it records:
//   A  (glalign_ends, two waves)  gl_walk<K, ENDS, Score> over q[0..m) and the forward strand in
//      wave 0 and, with both_strands, the reverse strand in wave 1; the waves meet once.
//   B  (the same kernel, wave 0)  gl_walk<K, ENDS, Anchored> over the rows q[q_end..0] and the
//      columns c[t_end..0] of the winning strand: both boundaries penalised, the result taken from
//      the last row (QUERY) or the last column (TARGET).  Its maximum is the score and its
//      smallest position is the start.  Skipped for BOTH, whose window is the whole matrix.
//   C  (glalign_paths, one wave)  gl_walk<K, GL_BOTH, Dirs> over the window, whatever `ends` was;
//      per cell one direction byte, stored by walk step.
//   D  (the same kernel, lane 0)  follows the bytes from the end cell in state H to the window's
//      (-1, -1), re-scores what it walks, emits the ops backwards and reverses them in place.
// Nothing waits across workgroups; every result is written with ordinary vector stores.
#include "swbank.h"
#include "swbank_align.h"
#include "swbank_kcommon.h"
#include "swbank_kglwalk.h"

namespace swk {
struct GlaArgs {
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint64_t* ids;
  const uint64_t* hits;
  size_t n_hits, n;
  uint32_t max_len;
  const uint2* qtab;
  const int8_t* mat;
  const uint8_t* query;
  uint32_t nq, alpha;
  const uint32_t* hit_queries;
  uint32_t hits_per_query;
  int32_t o, e;
  uint32_t both;
  sw_alignment* out;
  uint32_t* cigar;
  uint32_t cigar_stride;
  // passes A and B: hits h0 + [0, gridDim.x).  Passes C and D: position k of [0, count) is hit
  // list ? list[k] : h0 + k
  const uint32_t* list;
  size_t h0, count;
  const SwkAlignPlan* plan;  // optional, per position; else slot k of `slot` dwords
  uint64_t slot;
  uint32_t* dirs;
};

constexpr uint32_t GLA_NO_QUERY = 0xFFFFFFFFu;

// The strand walked: position x of the target, or of its reverse complement read from the far
// end; a code past the alphabet reads as its last code, as the score kernel reads it.
struct GlaStrand {
  const uint8_t* tp;
  uint32_t L, last;
  bool reverse;
  __device__ __forceinline__ uint32_t operator()(uint32_t x) const {
    uint32_t c = tp[reverse ? L - 1 - x : x];
    c = reverse && c < 4 ? c ^ 2u : c;
    return min(c, last);
  }
};

// Hit h's pair: the query's codes and length (GLA_NO_QUERY: the hit names no pair) and target.
struct GlaPair {
  const uint8_t* qp;
  uint32_t qlen;
  uint64_t t;
};
__device__ __forceinline__ GlaPair gla_pair(const GlaArgs& a, size_t h) {
  GlaPair pr{a.query, GLA_NO_QUERY, a.hits ? a.hits[h] : (uint64_t)h};
  const uint32_t qi = a.hit_queries ? a.hit_queries[h] : (uint32_t)h / a.hits_per_query;
  if (qi >= a.nq || pr.t >= a.n) return pr;
  const uint2 e = a.qtab[qi];
  pr.qp = a.query + e.x;
  pr.qlen = e.y;
  return pr;
}

// Passes A and B: one workgroup of two waves per hit; the whole record except the path fields.
template <int K, int ENDS>
__global__ void __launch_bounds__(128) glalign_ends(const GlaArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[GL_MAX_ALPHA * ROWS];
  __shared__ int32_t sbest[2];
  __shared__ uint32_t spos[2];
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t h = a.h0 + blockIdx.x;  // (< n_hits: the grid is a slice of the hit list)
  const GlaPair pr = gla_pair(a, h);   // (the same in every thread)
  sw_alignment r;
  r.score = 0;
  r.q_start = r.q_end = r.t_start = r.t_end = 0u;
  r.n_columns = r.n_identities = 0;
  r.cigar_offset = a.cigar_stride ? (uint32_t)(h * a.cigar_stride) : 0u;
  r.cigar_len = 0;
  if (pr.qlen == GLA_NO_QUERY) {
    r.index = r.id = SW_HIT_NONE;
    r.flags = (uint32_t)SW_ALIGN_EMPTY | (uint32_t)SW_ALIGN_NO_HIT;
    if (tid == 0) a.out[h] = r;
    return;
  }
  r.index = pr.t;
  r.id = a.ids ? a.ids[pr.t] : pr.t;
  r.flags = (uint32_t)SW_ALIGN_EMPTY;
  const uint32_t m = __builtin_amdgcn_readfirstlane(min(pr.qlen, (uint32_t)ROWS));
  const uint32_t L = __builtin_amdgcn_readfirstlane(min(a.lens[pr.t], a.max_len));
  if (m == 0) {
    if (tid == 0) a.out[h] = r;
    return;
  }
  gl_profile<K>(a.mat, a.alpha, prof, pr.qp, m, 128);
  __syncthreads();
  const uint8_t* tp = a.res + (L ? a.offs[pr.t] : 0);
  const uint32_t last = a.alpha - 1;
  if (wave == 0 || a.both) {
    const GlBest b = gl_walk<K, ENDS>(prof, GlaStrand{tp, L, last, wave != 0}, L, m, a.o, a.e);
    if ((tid & 63) == 0) {
      sbest[wave] = b.v;
      spos[wave] = b.pos;
    }
  }
  __syncthreads();  // (both waves are done with the profile)
  const bool rev = a.both && sbest[1] > sbest[0];
  const int32_t score = sbest[rev];
  const uint32_t pos = spos[rev];  // end index + 1 on the strand walked; 0: the boundary
  r.score = score;
  if (ENDS == GL_BOTH ? L == 0 : pos == 0) {  // the boundary won: the empty pair
    if (tid == 0) a.out[h] = r;
    return;
  }
  uint32_t qs = 0, qe = m - 1, ts = 0, te = L - 1;  // on the strand walked
  if constexpr (ENDS != GL_BOTH) {
    if (ENDS == GL_QUERY) te = min(pos - 1, L - 1);
    else qe = min(pos - 1, m - 1);
    // pass B: rows q[qe..0], columns c[te..0] of the winning strand
    gl_profile<K, -1>(a.mat, a.alpha, prof, pr.qp + qe, qe + 1, 128);
    __syncthreads();
    if (wave) return;
    const GlaStrand strand{tp, L, last, rev};
    const auto code = [&](uint32_t j) { return strand(te - j); };
    const GlBest s = gl_walk<K, ENDS, GlMode::Anchored>(prof, code, te + 1, qe + 1, a.o, a.e);
    // (s.pos >= 1: the boundary of the reversed walk scores less than a hit's score)
    const uint32_t back = s.pos ? s.pos - 1 : 0u;
    if (ENDS == GL_QUERY) ts = te - min(back, te);
    else qs = qe - min(back, qe);
  }
  if (tid == 0) {
    r.flags = (uint32_t)SW_ALIGN_NO_PATH | (rev ? (uint32_t)SW_ALIGN_REVERSE : 0u);
    r.q_start = qs;
    r.q_end = qe;
    r.t_start = rev ? L - 1 - te : ts;
    r.t_end = rev ? L - 1 - ts : te;
    a.out[h] = r;
  }
}

// Passes C and D: one wave per position; the direction bytes of the window, then lane 0 walks.
template <int K>
__global__ void __launch_bounds__(64) glalign_paths(const GlaArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[GL_MAX_ALPHA * ROWS];
  const uint32_t tid = threadIdx.x;
  const size_t k = blockIdx.x;  // (< count)
  const size_t h = a.list ? (size_t)a.list[k] : a.h0 + k;
  sw_alignment& r = a.out[h];
  const int32_t score = r.score;
  const uint32_t flags = r.flags;
  // (a hit with a path may score 0 or less: the flags say whether there is one)
  if (flags & ((uint32_t)SW_ALIGN_EMPTY | (uint32_t)SW_ALIGN_NO_HIT)) return;
  uint64_t dir_off, dir_cap, cig_off;
  uint32_t cig_cap;
  if (a.plan) {
    dir_off = a.plan[k].dir_off;
    dir_cap = a.plan[k].dir_cap;
    cig_off = a.plan[k].cig_off;
    cig_cap = a.plan[k].cig_cap;
  } else {
    dir_off = (uint64_t)k * a.slot;
    dir_cap = a.slot;
    cig_off = (uint64_t)h * a.cigar_stride;
    cig_cap = a.cigar_stride;
  }
  const GlaPair pr = gla_pair(a, h);
  if (pr.qlen == GLA_NO_QUERY || cig_cap == 0) return;
  const uint32_t L = min(a.lens[pr.t], a.max_len);
  const bool rev = (flags & (uint32_t)SW_ALIGN_REVERSE) != 0;
  const uint32_t qs = r.q_start, qe = r.q_end, t0 = r.t_start, t1 = r.t_end;
  // the window on the strand; a record this call's passes A and B did not write has no path
  if (qe < qs || qe >= pr.qlen || qe - qs >= (uint32_t)ROWS || t1 >= L || t1 < t0) return;
  const uint32_t ts = rev ? L - 1 - t1 : t0;
  const uint32_t Q = __builtin_amdgcn_readfirstlane(qe - qs + 1);
  const uint32_t C = __builtin_amdgcn_readfirstlane(t1 - t0 + 1);
  if (gl_dir_dwords(K, Q, C) > dir_cap) return;  // SW_ALIGN_NO_PATH stays
  gl_profile<K>(a.mat, a.alpha, prof, pr.qp + qs, Q, 64);
  __syncthreads();
  const GlaStrand strand{a.res + a.offs[pr.t], L, a.alpha - 1, rev};
  const auto code = [&](uint32_t j) { return strand(ts + j); };
  uint32_t* dirs = a.dirs + dir_off;
  gl_walk<K, GL_BOTH, GlMode::Dirs>(prof, code, C, Q, a.o, a.e, dirs);
  __threadfence();  // lane 0 reads what the other lanes stored
  __syncthreads();
  if (tid != 0) return;

  // pass D
  const uint8_t* db = reinterpret_cast<const uint8_t*>(dirs);
  uint32_t* cig = a.cigar + cig_off;
  int64_t i = (int64_t)Q - 1, c = (int64_t)C - 1;
  uint32_t nops = 0, cur = 0, run = 0, cols = 0, idn = 0;
  int32_t acc = 0;  // what the walked path scores
  int state = 3;    // 0 M, 1 E, 2 F, 3 H (the end cell is walked in state H)
  const auto flush = [&] {
    if (run) {
      if (nops < cig_cap) cig[nops] = run << 4 | cur;
      ++nops;
    }
    run = 0;
  };
  const auto emit = [&](uint32_t op, uint32_t len) {
    if (run && op == cur) {
      run += len;
    } else {
      flush();
      cur = op;
      run = len;
    }
    cols += len;
  };
  for (uint64_t it = 0, lim = (uint64_t)Q + C + 2; it < lim && i >= 0 && c >= 0; ++it) {
    const uint32_t ln = (uint32_t)i / K, rr = (uint32_t)i % K;
    const uint64_t t = (uint64_t)c + ln;
    const uint32_t bits = db[((t * (K / 4) + rr / 4) * 64 + ln) * 4 + rr % 4];
    if (state == 3) state = (int)(bits & 3u);
    if (state == 0) {
      const uint32_t tc = code((uint32_t)c);
      emit(SW_CIGAR_M, 1);
      idn += pr.qp[qs + i] == tc;
      acc += prof[tc * ROWS + i];
      --i;
      --c;
      state = 3;
    } else if (state == 1) {
      emit(SW_CIGAR_D, 1);
      acc += (bits & GL_E_EXT) ? a.e : a.o;
      state = (bits & GL_E_EXT) ? 1 : 3;
      --c;
    } else {
      emit(SW_CIGAR_I, 1);
      acc += (bits & GL_F_EXT) ? a.e : a.o;
      state = (bits & GL_F_EXT) ? 2 : 3;
      --i;
    }
  }
  // the boundary: on row -1 the rest is D ops, on column -1 I ops (a cell is left in state H)
  const bool done = state == 3 && (i < 0 || c < 0);
  if (done && c >= 0) {
    emit(SW_CIGAR_D, (uint32_t)c + 1);
    acc += a.o + (int32_t)c * a.e;
  } else if (done && i >= 0) {
    emit(SW_CIGAR_I, (uint32_t)i + 1);
    acc += a.o + (int32_t)i * a.e;
  }
  flush();
  if (!done || acc != score || nops > cig_cap) return;  // SW_ALIGN_NO_PATH stays
  for (uint32_t x = 0; x < nops / 2; ++x) {
    const uint32_t v = cig[x];
    cig[x] = cig[nops - 1 - x];
    cig[nops - 1 - x] = v;
  }
  r.flags = flags & ~(uint32_t)SW_ALIGN_NO_PATH;
  r.n_columns = cols;
  r.n_identities = idn;
  r.cigar_len = nops;
}

static GlaArgs gla_args(const SwkGlAlign* p) {
  GlaArgs a{};
  a.res = p->res;
  a.offs = p->offs;
  a.lens = p->lens;
  a.ids = p->ids;
  a.hits = p->hits;
  a.n_hits = p->n_hits;
  a.n = p->n;
  a.max_len = p->max_len;
  a.qtab = p->qtab;
  a.mat = p->mat;
  a.query = p->query;
  a.nq = p->nq;
  a.alpha = p->alpha;
  a.hit_queries = p->hit_queries;
  a.hits_per_query = p->hits_per_query;
  a.o = p->o;
  a.e = p->e;
  a.both = p->both ? 1u : 0u;
  a.out = static_cast<sw_alignment*>(p->out);
  a.cigar = p->cigar;
  a.cigar_stride = p->cigar_stride;
  return a;
}

static bool gla_args_ok(const SwkGlAlign* p) {
  return p && p->res && p->offs && p->lens && p->qtab && p->mat && p->query && p->out && p->n &&
         p->nq && p->qlen && p->qlen <= 1024 && p->alpha && p->alpha <= (uint32_t)GL_MAX_ALPHA &&
         (p->hit_queries != nullptr) != (p->hits_per_query != 0) && p->n_hits <= 0xFFFFFFFFull &&
         p->o <= 0 && p->e <= 0 && p->o >= -65534 && p->e >= -32767 && p->ends >= GL_QUERY &&
         p->ends <= GL_BOTH;
}

template <int K>
static void gla_ends_launch(const GlaArgs& a, int ends, dim3 grid, hipStream_t st) {
  switch (ends) {
    case GL_QUERY:
      hipLaunchKernelGGL((glalign_ends<K, GL_QUERY>), grid, dim3(128), 0, st, a);
      break;
    case GL_TARGET:
      hipLaunchKernelGGL((glalign_ends<K, GL_TARGET>), grid, dim3(128), 0, st, a);
      break;
    default: hipLaunchKernelGGL((glalign_ends<K, GL_BOTH>), grid, dim3(128), 0, st, a); break;
  }
}
}  // namespace swk

extern "C" uint64_t swk_glalign_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t cols) {
  return swk::gl_dir_dwords(swk::gl_rows(qlen), rows, cols);
}

extern "C" hipError_t swk_launch_glalign_ends(const SwkGlAlign* p, hipStream_t st) {
  using namespace swk;
  if (!p || p->n_hits == 0) return hipSuccess;
  if (!gla_args_ok(p)) return hipErrorInvalidValue;
  GlaArgs a = gla_args(p);
  const size_t XS = (size_t)1 << 24;  // hits of a launch
  for (size_t h0 = 0; h0 < p->n_hits; h0 += XS) {
    a.h0 = h0;
    const dim3 grid((unsigned)std::min(XS, p->n_hits - h0));
    switch (gl_rows(p->qlen)) {
      case 4: gla_ends_launch<4>(a, p->ends, grid, st); break;
      case 8: gla_ends_launch<8>(a, p->ends, grid, st); break;
      default: gla_ends_launch<16>(a, p->ends, grid, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" hipError_t swk_launch_glalign_paths(const SwkGlAlign* p, const uint32_t* list,
                                               size_t h0, size_t count, const SwkAlignPlan* plan,
                                               uint64_t slot, uint32_t* dirs, hipStream_t st) {
  using namespace swk;
  if (!p || count == 0) return hipSuccess;
  if (!gla_args_ok(p) || !dirs || !p->cigar || count > ((size_t)1 << 30) ||
      (list == nullptr && h0 + count > p->n_hits))
    return hipErrorInvalidValue;
  GlaArgs a = gla_args(p);
  a.list = list;
  a.h0 = h0;
  a.count = count;
  a.plan = plan;
  a.slot = slot;
  a.dirs = dirs;
  const dim3 grid((unsigned)count);
  switch (gl_rows(p->qlen)) {
    case 4: hipLaunchKernelGGL(glalign_paths<4>, grid, dim3(64), 0, st, a); break;
    case 8: hipLaunchKernelGGL(glalign_paths<8>, grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL(glalign_paths<16>, grid, dim3(64), 0, st, a); break;
  }
  return hipGetLastError();
}
