// swbank_kfsalign.hip — the kernels behind the alignments of frameshift hits (include/swbank.h
// "alignments of frameshift hits").
//
// One workgroup per hit.  The walk is fshift_score's (swbank_kfshift.hip): lane l owns the K rows
// [lK, lK + K), at step t it is at codon index j = t - l and computes the columns 3j, 3j + 1,
// 3j + 2 of its rows; the bottom row's H and F go one lane down per step with DPP wave_shr:1, the
// three amino acids of a codon index travel the same way, the profile lies in LDS, all arithmetic
// is int32.  A query has at most 64 x 16 rows, so there are no strips and no scratch rows.  What
// differs per pass is which rows and columns the walk sees:
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
  uint32_t tablew[16];  // 64 amino acids, c0 * 16 + c1 * 4 + c2 (little-endian words)
};

constexpr int FSA_AMINO = 24;      // the profile's real columns (SW_PROTEIN_ALPHA)
constexpr uint32_t FSA_OFF = 24;   // the column of a codon outside the pass's columns
constexpr uint32_t FSA_X = 22;     // a codon holding N (or any code past it)
constexpr int32_t FSA_PAD = -128;  // rows past the pass's rows, codons outside its columns
constexpr int32_t FSA_NEG = -(1 << 29);
constexpr uint32_t FSA_OFFW = FSA_OFF | FSA_OFF << 8 | FSA_OFF << 16;
constexpr uint32_t FSA_NO_QUERY = 0xFFFFFFFFu;

// Direction byte of a cell: bits 0-1 the source of H (0 M, 1 E, 2 F), bits 2-3 the link of M
// (0 the start, 1 p - 3, 2 p - 2, 3 p - 4), bit 4 E extends, bit 5 F extends.  Ties: M, then E,
// then F; p - 3, then p - 2, then p - 4; a gap opens rather than extends.

__host__ __device__ inline int fsa_rows(uint32_t qlen) {
  return qlen <= 256 ? 4 : qlen <= 512 ? 8 : 16;
}
__host__ __device__ inline uint64_t fsa_dir_dwords(int K, uint32_t rows, uint32_t cols) {
  if (rows == 0 || cols == 0) return 0;
  const uint64_t J = ((uint64_t)cols + 2) / 3, nl = ((uint64_t)rows + K - 1) / K;
  return (J + nl - 1) * (uint64_t)(48 * K);
}

__device__ __forceinline__ int32_t fsa_shr1(int32_t lane0_value, int32_t v) {  // wave_shr:1
  return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int32_t fsa_max3(int32_t a, int32_t b, int32_t c) {
  return max(max(a, b), c);
}

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
  const uint32_t c0 = fsa_base(s, p), c1 = fsa_base(s, p + 1), c2 = fsa_base(s, p + 2);
  const bool ok = (c0 | c1 | c2) < 4;  // all three are T, C, A or G
  return ok ? tab[c0 * 16 + c1 * 4 + c2] : FSA_X;
}
// The amino acids of codon index j, frame f at bits 8f; FSA_OFF past the pass's columns.
__device__ __forceinline__ uint32_t fsa_aminos(const uint8_t* tab, const FsaSeq& s, uint32_t j) {
  uint32_t w = 0;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const uint64_t c = 3ull * j + f;
    uint32_t a = FSA_OFF;
    if (c < s.ncols) a = fsa_amino(tab, s, s.p0 + (int64_t)s.pstep * (int64_t)c);
    w |= a << (8 * f);
  }
  return w;
}

// prof[c][row], row < 64K: the score of the pass's row `row` (query code qp[row * qstep], row <
// rows) against amino acid c; FSA_PAD past the rows and in column FSA_OFF.  All `nthreads`
// threads of the workgroup call it; the caller synchronises.
template <int K>
__device__ __forceinline__ void fsa_profile(const FsaArgs& a, int8_t* prof, const uint8_t* qp,
                                            int32_t qstep, uint32_t rows, uint32_t nthreads) {
  constexpr int ROWS = 64 * K;
  for (uint32_t row = threadIdx.x; row < (uint32_t)ROWS; row += nthreads) {
    const bool in_q = row < rows;
    const uint32_t q = in_q ? qp[(int64_t)row * qstep] : 0u;
    const int8_t* mr = a.mat + (q < a.alpha ? q : 0u) * a.alpha;
#pragma unroll
    for (int c = 0; c < FSA_AMINO; ++c)
      prof[c * ROWS + row] = in_q && (uint32_t)c < a.alpha ? mr[c] : (int8_t)FSA_PAD;
    prof[FSA_OFF * ROWS + row] = (int8_t)FSA_PAD;
  }
}

// One cell.  d3, bk, sk: H of the row above at p - 3, p - 2, p - 4; hl, el: H and E of this row at
// p - 3; nu, fu: H and F of the row above at p.  DIRS: the anchored matrix (no floor; `first`: the
// window's first cell, whose diagonal is 0) and the cell's direction byte.
template <bool DIRS>
__device__ __forceinline__ void fsa_cell(int32_t s, int32_t d3, int32_t bk, int32_t sk, bool first,
                                         int32_t hl, int32_t el, int32_t nu, int32_t fu, int32_t o,
                                         int32_t e, int32_t fs, int32_t& H, int32_t& E, int32_t& F,
                                         uint32_t& dir) {
  const int32_t sh = max(bk, sk) + fs;
  const int32_t eo = hl + o, ex = el + e, fo = nu + o, fx = fu + e;
  E = max(eo, ex);
  F = max(fo, fx);
  if constexpr (DIRS) {
    // cells no path reaches stay at the floor: without it their E would fall by e per column and
    // wrap after about 2^30 / |e| columns.  A cell of the preferred path lies above -2^18 (the
    // rest of the query gains at most 1,024 x 127), so the floor never touches one.
    E = max(E, FSA_NEG);
    F = max(F, FSA_NEG);
    const int32_t M = s + (first ? 0 : max(d3, sh));
    H = fsa_max3(M, E, F);
    const uint32_t link = first ? 0u : d3 >= sh ? 1u : bk >= sk ? 2u : 3u;
    const uint32_t src = H == M ? 0u : H == E ? 1u : 2u;
    dir = src | link << 2 | (ex > eo ? 16u : 0u) | (fx > fo ? 32u : 0u);
  } else {
    const int32_t M = s + fsa_max3(0, d3, sh);
    H = max(fsa_max3(0, M, E), F);
  }
}

// The walk of one wave over `rows` rows (the profile's) and the columns of sq.
// !DIRS: the local matrix; (bv, bc, bi) = the best cell: the highest H, then the smallest column,
// then the smallest row; bv = 0 when no cell is positive.  The same in every lane.
// DIRS: the anchored matrix; the direction bytes go to dirs (fsa_dir_dwords(K, rows, ncols)).
template <int K, bool DIRS>
__device__ __forceinline__ void fsa_walk(const int8_t* prof, const uint8_t* tab, const FsaSeq& sq,
                                         uint32_t rows, int32_t o, int32_t e, int32_t fs,
                                         uint32_t* dirs, int32_t& bv, uint32_t& bc, uint32_t& bi) {
  constexpr int ROWS = 64 * K;
  constexpr int32_t OUT = DIRS ? FSA_NEG : 0;  // H outside the matrix
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t J = (sq.ncols + 2) / 3;      // codon indices
  const uint32_t nl = (rows + K - 1) / K;     // lanes that hold rows
  const uint32_t steps = J && nl ? J + nl - 1 : 0u;

  int32_t h0[K], h1[K], h2[K], g2[K], e0[K], e1[K], e2[K];
#pragma unroll
  for (int r = 0; r < K; ++r) {
    h0[r] = h1[r] = h2[r] = g2[r] = OUT;
    e0[r] = e1[r] = e2[r] = FSA_NEG;
  }
  // the row above this lane's first: H and F of the three frames at this step's codon index (un,
  // uf), H at the index before it (ud), H of frame 2 two indices back (udd2)
  int32_t un0 = OUT, un1 = OUT, un2 = OUT, uf0 = FSA_NEG, uf1 = FSA_NEG, uf2 = FSA_NEG;
  int32_t ud0 = OUT, ud1 = OUT, ud2 = OUT, udd2 = OUT;
  int32_t best0 = 0, best1 = 0, best2 = 0;     // per frame: within one the visiting order is
  uint32_t pos0 = 0, pos1 = 0, pos2 = 0;       // column-major, so the first best is the rule's
  uint32_t aw = FSA_OFFW;  // this lane's three amino acids
  const int8_t* myprof = prof + lane * K;

  for (uint32_t t0 = 0; t0 < steps; t0 += 64) {
    const uint32_t jn = t0 + lane;
    const uint32_t nxt = jn < J ? fsa_aminos(tab, sq, jn) : FSA_OFFW;
    const uint32_t cnt = min(64u, steps - t0);
    for (uint32_t s = 0; s < cnt; ++s) {
      aw = (uint32_t)fsa_shr1(__builtin_amdgcn_readlane((int32_t)nxt, (int)s), (int32_t)aw);
      const int8_t* p0 = myprof + (aw & 0xFF) * ROWS;
      const int8_t* p1 = myprof + ((aw >> 8) & 0xFF) * ROWS;
      const int8_t* p2 = myprof + ((aw >> 16) & 0xFF) * ROWS;
      uint32_t w0[K / 4], w1[K / 4], w2[K / 4];
#pragma unroll
      for (int i = 0; i < K / 4; ++i) {
        w0[i] = reinterpret_cast<const uint32_t*>(p0)[i];
        w1[i] = reinterpret_cast<const uint32_t*>(p1)[i];
        w2[i] = reinterpret_cast<const uint32_t*>(p2)[i];
      }
      const uint32_t t = t0 + s;
      [[maybe_unused]] const bool start = DIRS && t == 0 && lane == 0;
      [[maybe_unused]] uint32_t dw[3 * K / 4];
      if constexpr (DIRS) {
#pragma unroll
        for (int i = 0; i < 3 * K / 4; ++i) dw[i] = 0;
      }
      // running down the rows: the row above at this index (n, f) and its state before this
      // step (d: H at j - 1, dd2: H of frame 2 at j - 2)
      int32_t n0 = un0, n1 = un1, n2 = un2, f0 = uf0, f1 = uf1, f2 = uf2;
      int32_t d0 = ud0, d1 = ud1, d2 = ud2, dd2 = udd2;
#pragma unroll
      for (int r = 0; r < K; ++r) {
        const int32_t s0 = (int32_t)(int8_t)(w0[r / 4] >> (8 * (r % 4)));
        const int32_t s1 = (int32_t)(int8_t)(w1[r / 4] >> (8 * (r % 4)));
        const int32_t s2 = (int32_t)(int8_t)(w2[r / 4] >> (8 * (r % 4)));
        int32_t H0, H1, H2, E0, E1, E2, F0, F1, F2;
        uint32_t b0 = 0, b1 = 0, b2 = 0;
        // frame 0: p - 3 frame 0 at j - 1, p - 2 frame 1 at j - 1, p - 4 frame 2 at j - 2
        fsa_cell<DIRS>(s0, d0, d1, dd2, r == 0 && start, h0[r], e0[r], n0, f0, o, e, fs, H0, E0,
                       F0, b0);
        // frame 1: p - 3 frame 1 at j - 1, p - 2 frame 2 at j - 1, p - 4 frame 0 at j - 1
        fsa_cell<DIRS>(s1, d1, d2, d0, false, h1[r], e1[r], n1, f1, o, e, fs, H1, E1, F1, b1);
        // frame 2: p - 3 frame 2 at j - 1, p - 2 frame 0 at j (the row above, this step),
        // p - 4 frame 1 at j - 1
        fsa_cell<DIRS>(s2, d2, n0, d1, false, h2[r], e2[r], n2, f2, o, e, fs, H2, E2, F2, b2);
        if constexpr (DIRS) {
          dw[r / 4] |= b0 << (8 * (r % 4));
          dw[K / 4 + r / 4] |= b1 << (8 * (r % 4));
          dw[2 * (K / 4) + r / 4] |= b2 << (8 * (r % 4));
        } else {
          const uint32_t at = t << 4 | (uint32_t)r;
          pos0 = H0 > best0 ? at : pos0;
          best0 = max(best0, H0);
          pos1 = H1 > best1 ? at : pos1;
          best1 = max(best1, H1);
          pos2 = H2 > best2 ? at : pos2;
          best2 = max(best2, H2);
        }
        // this row's state before the step is the next row's "row above"
        d0 = h0[r];
        d1 = h1[r];
        d2 = h2[r];
        dd2 = g2[r];
        g2[r] = d2;
        h0[r] = n0 = H0;
        h1[r] = n1 = H1;
        h2[r] = n2 = H2;
        e0[r] = E0;
        e1[r] = E1;
        e2[r] = E2;
        f0 = F0;
        f1 = F1;
        f2 = F2;
      }
      if constexpr (DIRS) {
        uint32_t* at = dirs + (size_t)t * (3 * K / 4) * 64 + lane;
#pragma unroll
        for (int i = 0; i < 3 * K / 4; ++i) at[(size_t)i * 64] = dw[i];
      }
      // the bottom row goes one lane down; above lane 0 lies the matrix's edge
      udd2 = ud2;
      ud0 = un0;
      ud1 = un1;
      ud2 = un2;
      un0 = fsa_shr1(OUT, n0);
      un1 = fsa_shr1(OUT, n1);
      un2 = fsa_shr1(OUT, n2);
      uf0 = fsa_shr1(FSA_NEG, f0);
      uf1 = fsa_shr1(FSA_NEG, f1);
      uf2 = fsa_shr1(FSA_NEG, f2);
    }
  }
  if constexpr (!DIRS) {
    // the lane's best of the three frames, then the wave's: value, then column, then row
    int32_t v = 0;
    uint32_t c = 0, i = 0;
    const auto take = [&](int32_t bv2, uint32_t c2, uint32_t i2) {
      const bool better = bv2 > v || (bv2 == v && v > 0 && (c2 < c || (c2 == c && i2 < i)));
      v = better ? bv2 : v;
      c = better ? c2 : c;
      i = better ? i2 : i;
    };
    take(best0, 3 * ((pos0 >> 4) - lane), lane * K + (pos0 & 15u));
    take(best1, 3 * ((pos1 >> 4) - lane) + 1, lane * K + (pos1 & 15u));
    take(best2, 3 * ((pos2 >> 4) - lane) + 2, lane * K + (pos2 & 15u));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
      take(__shfl_xor(v, d, 64), __shfl_xor(c, d, 64), __shfl_xor(i, d, 64));
    bv = __builtin_amdgcn_readfirstlane(v);
    bc = __builtin_amdgcn_readfirstlane(c);
    bi = __builtin_amdgcn_readfirstlane(i);
  }
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
  __shared__ __attribute__((aligned(16))) int8_t prof[(FSA_AMINO + 1) * ROWS];
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
  if (tid < 16) tabw[tid] = a.tablew[tid];
  fsa_profile<K>(a, prof, pr.qp, 1, m, 128);
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  const uint8_t* tp = a.res + a.offs[pr.t];
  int32_t bv;
  uint32_t bc, bi;
  fsa_walk<K, false>(prof, tab, FsaSeq{tp, L, wave1, 0, 1, L - 2}, m, a.o, a.e, a.fs, nullptr, bv,
                     bc, bi);
  if ((tid & 63) == 0) {
    sbest[wave1][0] = (uint32_t)bv;
    sbest[wave1][1] = bc;
    sbest[wave1][2] = bi;
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
  fsa_profile<K>(a, prof, pr.qp + qe, -1, qe + 1, 128);
  __syncthreads();
  if (wave1) return;
  fsa_walk<K, false>(prof, tab, FsaSeq{tp, L, rev, (int64_t)pe, -1, pe + 1}, qe + 1, a.o, a.e,
                     a.fs, nullptr, bv, bc, bi);
  if (tid == 0) {
    const uint32_t ps = pe - min(bc, pe), qs = qe - min(bi, qe);
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
  __shared__ __attribute__((aligned(16))) int8_t prof[(FSA_AMINO + 1) * ROWS];
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
  if (fsa_dir_dwords(K, Q, C) > dir_cap) return;  // SW_ALIGN_NO_PATH stays
  if (tid < 16) tabw[tid] = a.tablew[tid];
  fsa_profile<K>(a, prof, pr.qp + qs, 1, Q, 64);
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  const FsaSeq sq{a.res + a.offs[pr.t], L, rev, (int64_t)ps, 1, C};
  uint32_t* dirs = a.dirs + dir_off;
  int32_t b0;
  uint32_t b1, b2;
  fsa_walk<K, true>(prof, tab, sq, Q, a.o, a.e, a.fs, dirs, b0, b1, b2);
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
  for (int i = 0; i < 16; ++i)  // (little-endian words: byte i of the table is byte i of LDS)
    a.tablew[i] = (uint32_t)p->table[4 * i] | (uint32_t)p->table[4 * i + 1] << 8 |
                  (uint32_t)p->table[4 * i + 2] << 16 | (uint32_t)p->table[4 * i + 3] << 24;
  return a;
}

static bool fsa_args_ok(const SwkFsAlign* p) {
  return p && p->res && p->offs && p->lens && p->qtab && p->mat && p->query && p->out && p->n &&
         p->nq && p->qlen && p->qlen <= 1024 && p->alpha && p->alpha <= (uint32_t)FSA_AMINO &&
         (p->hit_queries != nullptr) != (p->hits_per_query != 0) && p->n_hits <= 0xFFFFFFFFull &&
         p->o <= 0 && p->e <= 0 && p->fs <= 0 && p->o >= -65534 && p->e >= -32767 &&
         p->fs >= -32767 && p->max_len < (1u << 29);  // (pass A packs step << 4 | row)
}
}  // namespace swk

extern "C" uint64_t swk_fsalign_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t cols) {
  return swk::fsa_dir_dwords(swk::fsa_rows(qlen), rows, cols);
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
    switch (fsa_rows(p->qlen)) {
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
  switch (fsa_rows(p->qlen)) {
    case 4: hipLaunchKernelGGL(fsalign_paths<4>, grid, dim3(64), 0, st, a); break;
    case 8: hipLaunchKernelGGL(fsalign_paths<8>, grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL(fsalign_paths<16>, grid, dim3(64), 0, st, a); break;
  }
  return hipGetLastError();
}
