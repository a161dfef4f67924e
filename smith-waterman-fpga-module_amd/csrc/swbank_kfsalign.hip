// swbank_kfsalign.hip — the kernels behind the alignments of frameshift hits (include/swbank.h
// "alignments of frameshift hits").
//
// One workgroup per hit.  Every pass but the last is the walk of swbank_kfswalk.h, which the score
// kernel runs too, so a record's score is the score call's.  A query has at most 64 x 16 rows, so
// there are no strips and no scratch rows.  What differs per pass is which rows and columns the
// walk sees and what it records:
//   A  (fsalign_ends, two waves)  rows q[0..m), columns p = 0 .. L - 3 of the forward (wave 0) and
//      of the reverse strand (wave 1); every lane keeps its best cell per frame, a wave reduction
//      picks the highest H, then the smallest p, then the smallest i; the waves meet once.
//   B  (the same kernel, wave 0)  rows q[q_end..0], columns p_end .. 0 of the winning strand, each
//      column keeping its forward codon: the best cell under the same rule is the start.
//   C  (fsalign_paths, one wave)  rows q[q_start..q_end], columns p_start .. p_end, no floor and a
//      0 diagonal at the first cell only; per cell one direction byte, stored by walk step: at
//      step t lane l writes its 3K bytes (frame-major) as 3K/4 dwords at [t][word][lane].
//   D  (the same kernel, lane 0)  follows the bytes from the end cell, re-scores what it walks,
//      emits the ops backwards and reverses them in place.
// Nothing waits across workgroups; every result is written with ordinary vector stores.
#include "swbank.h"
#include "swbank_align.h"
#include "swbank_kcommon.h"
#include "swbank_kfswalk.h"

namespace swk {
struct FsaArgs {
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
  int32_t o, e, fs;
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
  FsTable table;
};

constexpr uint32_t FSA_NO_QUERY = 0xFFFFFFFFu;

// The columns of a pass: column c is the codon start p0 + pstep * c of the strand (the target, or
// its reverse complement read from the far end), c < ncols; every such codon lies in the strand.
struct FsaSeq {
  const uint8_t* tp;
  uint32_t L;
  bool reverse;
  int64_t p0;
  int32_t pstep;
  uint32_t ncols;
};
__device__ __forceinline__ uint32_t fsa_base(const FsaSeq& s, int64_t x) {
  const uint32_t v = s.tp[s.reverse ? (int64_t)s.L - 1 - x : x];
  return s.reverse && v < 4 ? v ^ 2u : v;
}
// The amino acid of the codon at strand position p (0 <= p <= L - 3).
__device__ __forceinline__ uint32_t fsa_amino(const uint8_t* tab, const FsaSeq& s, int64_t p) {
  return fs_codon(tab, fsa_base(s, p), fsa_base(s, p + 1), fsa_base(s, p + 2));
}
// The amino acids of codon index j, frame f at bits 8f; FS_OFF past the pass's columns.
__device__ __forceinline__ uint32_t fsa_aminos(const uint8_t* tab, const FsaSeq& s, uint32_t j) {
  uint32_t w = 0;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const uint64_t c = 3ull * j + f;
    uint32_t a = FS_OFF;
    if (c < s.ncols) a = fsa_amino(tab, s, s.p0 + (int64_t)s.pstep * (int64_t)c);
    w |= a << (8 * f);
  }
  return w;
}
// The walk over `rows` rows (the profile's) and the columns of sq.
template <int K, FsMode MODE>
__device__ __forceinline__ auto fsa_walk(const FsaArgs& a, const int8_t* prof, const uint8_t* tab,
                                         const FsaSeq& sq, uint32_t rows, uint32_t* dirs) {
  const auto aminos = [&](uint32_t j) { return fsa_aminos(tab, sq, j); };
  return fs_walk<K, MODE>(prof, aminos, (sq.ncols + 2) / 3, rows, a.o, a.e, a.fs, dirs);
}

// Hit h's pair: the query's codes and length (FSA_NO_QUERY: the hit names no pair) and target.
struct FsaPair {
  const uint8_t* qp;
  uint32_t qlen;
  uint64_t t;
};
__device__ __forceinline__ FsaPair fsa_pair(const FsaArgs& a, size_t h) {
  FsaPair pr{a.query, FSA_NO_QUERY, a.hits ? a.hits[h] : (uint64_t)h};
  const uint32_t qi = a.hit_queries ? a.hit_queries[h] : (uint32_t)h / a.hits_per_query;
  if (qi >= a.nq || pr.t >= a.n) return pr;
  const uint2 e = a.qtab[qi];
  pr.qp = a.query + e.x;
  pr.qlen = e.y;
  return pr;
}

// Passes A and B: one workgroup of two waves per hit; the whole record except the path fields.
template <int K>
__global__ void __launch_bounds__(128) fsalign_ends(const FsaArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[(FS_AMINO + 1) * ROWS];
  __shared__ uint32_t tabw[16];
  __shared__ uint32_t sbest[2][3];
  const uint32_t tid = threadIdx.x;
  const bool wave1 = tid >= 64;
  const size_t h = a.h0 + blockIdx.x;  // (< n_hits: the grid is a slice of the hit list)
  const FsaPair pr = fsa_pair(a, h);  // (the same in every thread)
  sw_alignment r;
  r.score = 0;
  r.q_start = r.q_end = r.t_start = r.t_end = 0u;
  r.n_columns = r.n_identities = 0;
  r.cigar_offset = a.cigar_stride ? (uint32_t)(h * a.cigar_stride) : 0u;
  r.cigar_len = 0;
  if (pr.qlen == FSA_NO_QUERY) {
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
  if (L < 3 || m == 0) {
    if (tid == 0) a.out[h] = r;
    return;
  }
  if (tid < 16) tabw[tid] = a.table.w[tid];
  fs_profile<K>(a.mat, a.alpha, prof, pr.qp, 1, m, 128);
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  const uint8_t* tp = a.res + a.offs[pr.t];
  const FsBest end =
      fsa_walk<K, FsMode::Best>(a, prof, tab, FsaSeq{tp, L, wave1, 0, 1, L - 2}, m, nullptr);
  if ((tid & 63) == 0) {
    sbest[wave1][0] = (uint32_t)end.v;
    sbest[wave1][1] = end.c;
    sbest[wave1][2] = end.i;
  }
  __syncthreads();  // (both waves are done with the profile)
  const bool rev = (int32_t)sbest[1][0] > (int32_t)sbest[0][0];
  const int32_t score = (int32_t)sbest[rev][0];
  const uint32_t pe = min(sbest[rev][1], L - 3), qe = min(sbest[rev][2], m - 1);
  if (score <= 0) {
    if (tid == 0) a.out[h] = r;
    return;
  }
  // pass B: rows q[qe..0], columns pe .. 0 of the winning strand
  fs_profile<K>(a.mat, a.alpha, prof, pr.qp + qe, -1, qe + 1, 128);
  __syncthreads();
  if (wave1) return;
  const FsBest start = fsa_walk<K, FsMode::Best>(
      a, prof, tab, FsaSeq{tp, L, rev, (int64_t)pe, -1, pe + 1}, qe + 1, nullptr);
  if (tid == 0) {
    const uint32_t ps = pe - min(start.c, pe), qs = qe - min(start.i, qe);
    r.score = score;
    r.flags = (uint32_t)SW_ALIGN_NO_PATH | (rev ? (uint32_t)SW_ALIGN_REVERSE : 0u) |
              (ps % 3) << SW_ALIGN_FRAME_SHIFT;
    r.q_start = qs;
    r.q_end = qe;
    r.t_start = rev ? L - 1 - (pe + 2) : ps;
    r.t_end = rev ? L - 1 - ps : pe + 2;
    a.out[h] = r;
  }
}

// Passes C and D: one wave per position; the direction bytes of the window, then lane 0 walks.
template <int K>
__global__ void __launch_bounds__(64) fsalign_paths(const FsaArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[(FS_AMINO + 1) * ROWS];
  __shared__ uint32_t tabw[16];
  const uint32_t tid = threadIdx.x;
  const size_t k = blockIdx.x;  // (< count)
  const size_t h = a.list ? (size_t)a.list[k] : a.h0 + k;
  sw_alignment& r = a.out[h];
  const int32_t score = r.score;
  const uint32_t flags = r.flags;
  if (score <= 0 || (flags & ((uint32_t)SW_ALIGN_EMPTY | (uint32_t)SW_ALIGN_NO_HIT))) return;
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
  const FsaPair pr = fsa_pair(a, h);
  if (pr.qlen == FSA_NO_QUERY || cig_cap == 0) return;
  const uint32_t L = min(a.lens[pr.t], a.max_len);
  const bool rev = (flags & (uint32_t)SW_ALIGN_REVERSE) != 0;
  const uint32_t qs = r.q_start, qe = r.q_end, ts = r.t_start, te = r.t_end;
  // the window on the strand; a record this call's pass B did not write has no path
  if (qe < qs || qe >= pr.qlen || qe - qs >= (uint32_t)ROWS || te >= L || te < ts || te - ts < 2)
    return;
  const uint32_t ps = rev ? L - 1 - te : ts, pe = rev ? L - 1 - ts - 2 : te - 2;
  const uint32_t Q = __builtin_amdgcn_readfirstlane(qe - qs + 1);
  const uint32_t C = __builtin_amdgcn_readfirstlane(pe - ps + 1);
  if (fs_dir_dwords(K, Q, C) > dir_cap) return;  // SW_ALIGN_NO_PATH stays
  if (tid < 16) tabw[tid] = a.table.w[tid];
  fs_profile<K>(a.mat, a.alpha, prof, pr.qp + qs, 1, Q, 64);
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  const FsaSeq sq{a.res + a.offs[pr.t], L, rev, (int64_t)ps, 1, C};
  uint32_t* dirs = a.dirs + dir_off;
  fsa_walk<K, FsMode::Dirs>(a, prof, tab, sq, Q, dirs);
  __threadfence();  // lane 0 reads what the other lanes stored
  __syncthreads();
  if (tid != 0) return;

  // pass D
  const uint8_t* db = reinterpret_cast<const uint8_t*>(dirs);
  uint32_t* cig = a.cigar + cig_off;
  int64_t i = (int64_t)Q - 1, c = (int64_t)C - 1;
  uint32_t nops = 0, cur = 0, run = 0, cols = 0, idn = 0;
  int32_t acc = 0;  // what the walked path scores
  int state = 0;    // 0 M (the end cell is walked as one), 1 E, 2 F, 3 H
  bool done = false;
  const auto flush = [&] {
    if (run) {
      if (nops < cig_cap) cig[nops] = run << 4 | cur;
      ++nops;
    }
    run = 0;
  };
  const auto emit = [&](uint32_t code) {  // (a shift op is never merged)
    if (run && code == cur && code < (uint32_t)SW_CIGAR_FS_SKIP) {
      ++run;
    } else {
      flush();
      cur = code;
      run = 1;
    }
  };
  for (uint64_t it = 0, lim = (uint64_t)Q + C + 2; it < lim && i >= 0 && c >= 0; ++it) {
    const uint32_t ln = (uint32_t)i / K, rr = (uint32_t)i % K;
    const uint32_t f = (uint32_t)(c % 3), x = f * K + rr;
    const uint64_t t = (uint64_t)(c / 3) + ln;
    const uint32_t bits = db[((t * (3 * K / 4) + x / 4) * 64 + ln) * 4 + x % 4];
    if (state == 3) state = (int)(bits & 3u);
    if (state == 0) {
      const uint32_t am = fsa_amino(tab, sq, (int64_t)ps + c);
      emit(SW_CIGAR_M);
      ++cols;
      idn += pr.qp[qs + i] == am;
      acc += prof[am * ROWS + i];
      const uint32_t link = bits >> 2 & 3u;
      if (link == 0) {
        done = i == 0 && c == 0;
        break;
      }
      if (link != 1) {
        emit(link == 2 ? SW_CIGAR_FS_BACK : SW_CIGAR_FS_SKIP);
        acc += a.fs;
      }
      c -= link == 1 ? 3 : link == 2 ? 2 : 4;
      --i;
      state = 3;
    } else if (state == 1) {
      emit(SW_CIGAR_D);
      ++cols;
      acc += (bits & 16u) ? a.e : a.o;
      state = (bits & 16u) ? 1 : 3;
      c -= 3;
    } else {
      emit(SW_CIGAR_I);
      ++cols;
      acc += (bits & 32u) ? a.e : a.o;
      state = (bits & 32u) ? 2 : 3;
      --i;
    }
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

static FsaArgs fsa_args(const SwkFsAlign* p) {
  FsaArgs a{};
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
  a.fs = p->fs;
  a.out = static_cast<sw_alignment*>(p->out);
  a.cigar = p->cigar;
  a.cigar_stride = p->cigar_stride;
  a.table = fs_table(p->table);
  return a;
}

static bool fsa_args_ok(const SwkFsAlign* p) {
  return p && p->res && p->offs && p->lens && p->qtab && p->mat && p->query && p->out && p->n &&
         p->nq && p->qlen && p->qlen <= 1024 && p->alpha && p->alpha <= (uint32_t)FS_AMINO &&
         (p->hit_queries != nullptr) != (p->hits_per_query != 0) && p->n_hits <= 0xFFFFFFFFull &&
         fs_penalties_ok(p->o, p->e, p->fs) &&
         p->max_len < (1u << 29);  // (the walk packs a best cell as step << 4 | row)
}
}  // namespace swk

extern "C" uint64_t swk_fsalign_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t cols) {
  return swk::fs_dir_dwords(swk::fs_rows(qlen), rows, cols);
}

extern "C" hipError_t swk_launch_fsalign_ends(const SwkFsAlign* p, hipStream_t st) {
  using namespace swk;
  if (!p || p->n_hits == 0) return hipSuccess;
  if (!fsa_args_ok(p)) return hipErrorInvalidValue;
  FsaArgs a = fsa_args(p);
  const size_t XS = (size_t)1 << 24;  // hits of a launch
  for (size_t h0 = 0; h0 < p->n_hits; h0 += XS) {
    a.h0 = h0;
    const dim3 grid((unsigned)std::min(XS, p->n_hits - h0));
    switch (fs_rows(p->qlen)) {
      case 4: hipLaunchKernelGGL(fsalign_ends<4>, grid, dim3(128), 0, st, a); break;
      case 8: hipLaunchKernelGGL(fsalign_ends<8>, grid, dim3(128), 0, st, a); break;
      default: hipLaunchKernelGGL(fsalign_ends<16>, grid, dim3(128), 0, st, a); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" hipError_t swk_launch_fsalign_paths(const SwkFsAlign* p, const uint32_t* list,
                                               size_t h0, size_t count, const SwkAlignPlan* plan,
                                               uint64_t slot, uint32_t* dirs, hipStream_t st) {
  using namespace swk;
  if (!p || count == 0) return hipSuccess;
  if (!fsa_args_ok(p) || !dirs || !p->cigar || count > ((size_t)1 << 30) ||
      (list == nullptr && h0 + count > p->n_hits))
    return hipErrorInvalidValue;
  FsaArgs a = fsa_args(p);
  a.list = list;
  a.h0 = h0;
  a.count = count;
  a.plan = plan;
  a.slot = slot;
  a.dirs = dirs;
  const dim3 grid((unsigned)count);
  switch (fs_rows(p->qlen)) {
    case 4: hipLaunchKernelGGL(fsalign_paths<4>, grid, dim3(64), 0, st, a); break;
    case 8: hipLaunchKernelGGL(fsalign_paths<8>, grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL(fsalign_paths<16>, grid, dim3(64), 0, st, a); break;
  }
  return hipGetLastError();
}
