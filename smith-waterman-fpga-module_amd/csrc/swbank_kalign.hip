// swbank_kalign.hip — alignments of chosen hits: exact end and start cells,
// the direction store and the CIGAR walk.  The int32 re-score kernel (score_i32,
// swbank_kaux.hip) is the model: one wave per pair, strips of 256 query rows, lane l owns rows
// [4l, 4l+4) of a strip and walks anti-diagonals (step st: column st - l) with DPP wave_shr:1,
// the strip's bottom row {H, X} goes to the next strip through a per-wave HBM scratch row, the
// substitution profile sits in the wave's own LDS slice (each lane reads only its own entries:
// no barrier).  Unlike there the profile is built per pair and strip from the alpha x alpha
// matrix (LDS), because the rows a lane owns depend on the pass: the forward pass reads
// q[0..), the reverse pass q[q_end..0], the direction pass q[q_start..q_end].
//
// One recurrence serves the three passes, each cell reading its left, upper and diagonal
// neighbours (floor f = 0 in the local passes A and B; in pass C f = -2^29, "no path", and only
// the window's first cell starts a path: its diagonal is 0):
//   Gotoh   E = max(Hleft - o - e, Eleft - e)   F = max(Hup - o - e, Fup - e)
//           H = max(f, Hdiag + s, E, F)
//   merged  M = max(f, Hdiag + s)   I = max(Tup, Tleft)   H = max(M, I)
//           T = max(f, M - o - e, I - e)
// (merged: the HDL's first-column rule is not applied; the host refuses the one case in which
// it changes a score, max(s) > o + e.)
//
// The kernels are templated on SET: the SET instances serve sw_align_set_hits* and take each
// hit's query from a table of the loaded set (al_query); the others are the single-query
// kernels, which the set costs nothing.  STRAND (with SET; sw_align_strand_hits*): a hit whose
// strand is 1 is aligned against the reverse complement of its target without a copy of it: the
// walks read the target from its far end with the opposite step (AlSeq.tstep) under a
// column-complemented copy of the matrix, so the profile build and al_walk are what they are;
// the records keep the coordinates of the reverse-complemented target until align_flip, after
// the last pass that reads them.
#include "swbank.h"
#include "swbank_align.h"
#include "swbank_kcommon.h"

namespace swk {
constexpr int AL_K = 4, AL_LETTERS = 25;  // rows per lane; profile letters incl. padding
constexpr int32_t AL_NEG = -(1 << 29);

// Direction bits of a cell (one byte per row, 4 rows per dword):
//   Gotoh   bits 0-1 source of H (0 diagonal, 1 E, 2 F), bit 2 E extends, bit 3 F extends
//   merged  bit 0 H is the gap value, bit 1 the gap comes from above, bit 2 T extends
// Ties: the diagonal first, then the gap from the left (D), then from above (I); a gap opens
// rather than extends.

struct AlignArgs {
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint64_t* ids;    // optional
  const uint64_t* hits;   // optional: hit h aligns target hits[h], else target h
  size_t n_hits;
  const uint8_t* query;
  uint32_t qlen;
  const int8_t* mat;      // alpha x alpha
  uint32_t alpha, pad;
  int32_t padscore;       // score of the padding letter (codes past the alphabet)
  uint32_t O, E;
  sw_alignment* out;
  uint32_t* cigar;
  uint32_t cigar_stride;  // 0: coordinates only
  uint2* scratch;         // per wave: 2 x scols uint2
  uint32_t scols;
  // passes C and D: position k of [0, count) is hit list ? list[k] : h0 + k
  const uint32_t* list;
  size_t h0, count;
  const SwkAlignPlan* plan;  // optional, per position; else slot k of `slot` dwords
  uint64_t slot;
  uint32_t* dirs;
  // a query set (the SET kernels): query i's codes at query + qtab[i].x, qtab[i].y of them; hit
  // h's query is hit_queries[h], or h / hits_per_query; n targets in the batch
  const uint2* qtab;
  const uint32_t* hit_queries;
  uint32_t nq, hits_per_query;
  size_t n;
  // the STRAND kernels: hit h (query i, target t) is on the reverse strand when strands[h]
  // (strand_by_hit: the host call's gathered list) or strands[i * n + t] is not 0
  const uint8_t* strands;
  uint32_t strand_by_hit;
};

// Hit h's query.  !SET: the one loaded query.  SET: the hit's own; len = 0xFFFFFFFF when the hit
// names no query (SW_QUERY_NONE, or any index past the set: nothing is read for it).
struct AlQuery {
  const uint8_t* p;
  uint32_t len;
};
constexpr uint32_t AL_NO_QUERY = 0xFFFFFFFFu;
// UNIFORM: h is the same in every lane of the wave (passes A-C); the entry goes to SGPRs.
template <bool SET, bool UNIFORM>
__device__ __forceinline__ AlQuery al_query(const AlignArgs& a, size_t h) {
  if constexpr (!SET) return AlQuery{a.query, a.qlen};
  uint32_t qi = a.hit_queries ? a.hit_queries[h] : (uint32_t)h / a.hits_per_query;
  if constexpr (UNIFORM) qi = __builtin_amdgcn_readfirstlane(qi);
  if (qi >= a.nq) return AlQuery{a.query, AL_NO_QUERY};
  uint2 e = a.qtab[qi];
  if constexpr (UNIFORM) {
    e.x = __builtin_amdgcn_readfirstlane(e.x);
    e.y = __builtin_amdgcn_readfirstlane(e.y);
  }
  return AlQuery{a.query + e.x, e.y};
}

// Whether hit h (target t) lies on the reverse strand; the hit names a pair.
__device__ __forceinline__ bool al_reverse(const AlignArgs& a, size_t h, uint64_t t) {
  if (a.strand_by_hit) return a.strands[h] != 0;
  const uint32_t qi = a.hit_queries ? a.hit_queries[h] : (uint32_t)h / a.hits_per_query;
  return a.strands[(size_t)qi * a.n + t] != 0;
}
__device__ __forceinline__ uint32_t al_comp(uint32_t c) { return c < 4 ? c ^ 2u : c; }

__device__ __forceinline__ int32_t al_lane0(int32_t inj, int32_t v) {  // wave_shr:1
  return __builtin_amdgcn_update_dpp(inj, v, 0x138, 0xF, 0xF, false);
}

struct AlSeq {  // rows: code r at qp[r * qstep]; columns: code c at tp[c * tstep]
  const uint8_t* qp;
  const uint8_t* tp;
  int32_t qstep, tstep;
  uint32_t Q, L;
};

__host__ __device__ __forceinline__ uint64_t al_dir_dwords(uint32_t Q, uint32_t L) {
  return (uint64_t)((Q + 255) / 256) * ((uint64_t)L + 63) * 64;
}

// The walk over Q rows x L columns.  !DIRS: local, returns the lane's best cell under the end
// rule (highest value, then lowest column, then lowest row).  DIRS: anchored at cell (0, 0),
// stores the direction dwords at dirs[(strip * (L + 63) + step) * 64 + lane].
template <bool GOTOH, bool DIRS>
__device__ __forceinline__ void al_walk(const AlignArgs& a, const int8_t* smat,
                                        uint2 (&mine)[AL_LETTERS][64], uint2* const (&scr)[2],
                                        const AlSeq& q, uint32_t* dirs, int32_t& best,
                                        uint32_t& bi, uint32_t& bj) {
  const int lane = threadIdx.x & 63;
  const int32_t oe = (int32_t)(a.O + a.E), e = (int32_t)a.E;
  const uint32_t pad = a.pad, A = a.alpha, L = q.L;
  const int32_t fl = DIRS ? AL_NEG : 0;
  const uint32_t nstrips = (q.Q + 255) / 256;
  const uint32_t nsteps = L + 63;
  best = 0;
  bi = 0;
  bj = 0xFFFFFFFFu;
  for (uint32_t s = 0; s < nstrips && L; ++s) {
    int32_t vmask[AL_K];
    uint32_t qc[AL_K];
#pragma unroll
    for (int k = 0; k < AL_K; ++k) {
      const uint32_t r = s * 256u + (uint32_t)lane * AL_K + k;
      vmask[k] = r < q.Q ? -1 : 0;
      qc[k] = r < q.Q ? q.qp[(int64_t)r * q.qstep] : 0u;
    }
    for (uint32_t c = 0; c <= pad; ++c) {  // this lane's 4 rows of the strip's profile
      int32_t v[AL_K];
#pragma unroll
      for (int k = 0; k < AL_K; ++k)
        v[k] = !vmask[k] ? 0 : c < A ? (int32_t)smat[qc[k] * A + c] : a.padscore;
      mine[c][lane] = make_uint2(((uint32_t)v[0] & 0xFFFFu) | ((uint32_t)v[1] << 16),
                                 ((uint32_t)v[2] & 0xFFFFu) | ((uint32_t)v[3] << 16));
    }
    const bool seg_in = s > 0, seg_out = s + 1 < nstrips;
    const uint2* ein = scr[(s + 1) & 1];
    uint2* eout = scr[s & 1];
    int32_t H[AL_K], X[AL_K];  // H and E (Gotoh) / T (merged) of the column to the left
#pragma unroll
    for (int k = 0; k < AL_K; ++k) H[k] = X[k] = fl;
    int32_t botH = fl, botX = fl;
    int32_t prevUpH = DIRS && s == 0 && lane == 0 ? 0 : fl;  // the window's first cell starts
    uint32_t code = pad, buf = pad;
    uint2 ebuf = make_uint2((uint32_t)fl, (uint32_t)fl), obuf = make_uint2(0u, 0u);
    for (uint32_t st = 0; st < nsteps; ++st) {
      if ((st & 63) == 0) {  // the next 64 columns: codes (and the previous strip's row)
        const uint32_t c = st + lane;
        buf = c < L ? min((uint32_t)q.tp[(int64_t)c * q.tstep], pad) : pad;
        if (seg_in) ebuf = c < L ? ein[c] : make_uint2((uint32_t)fl, (uint32_t)fl);
      }
      const uint32_t j = st - (uint32_t)lane;  // this lane's column (wraps when not started)
      code = (uint32_t)al_lane0((int32_t)__builtin_amdgcn_readlane(buf, st & 63), (int32_t)code);
      const int32_t upH =
          al_lane0(seg_in ? (int32_t)__builtin_amdgcn_readlane(ebuf.x, st & 63) : fl, botH);
      const int32_t upX =
          al_lane0(seg_in ? (int32_t)__builtin_amdgcn_readlane(ebuf.y, st & 63) : fl, botX);
      const uint2 w = mine[code][lane];
      const int32_t sc[AL_K] = {(int32_t)(w.x << 16) >> 16, (int32_t)w.x >> 16,
                                (int32_t)(w.y << 16) >> 16, (int32_t)w.y >> 16};
      if (j < L) {  // active: column j of the lane's 4 rows
        int32_t diag = prevUpH, up = upH, ux = upX, hv[AL_K];
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < AL_K; ++k) {
          const int32_t D = diag + sc[k];
          diag = H[k];
          int32_t h;
          if constexpr (GOTOH) {
            const int32_t eo = H[k] - oe, ee = X[k] - e, fo = up - oe, fe = ux - e;
            const int32_t Ev = max(eo, ee), Fv = max(fo, fe), G = max(Ev, Fv);
            h = max(max(D, fl), G);
            if constexpr (DIRS)
              bits |= ((D >= G ? 0u : Ev >= Fv ? 1u : 2u) | (ee > eo ? 4u : 0u) |
                       (fe > fo ? 8u : 0u)) << (8 * k);
            X[k] = Ev;
            ux = Fv;
          } else {
            const int32_t M = max(D, fl);
            const int32_t I = max(ux, X[k]);
            h = max(M, I);
            const int32_t to = M - oe, te = I - e;
            if constexpr (DIRS)
              bits |= ((I > M ? 1u : 0u) | (ux > X[k] ? 2u : 0u) | (te > to ? 4u : 0u)) << (8 * k);
            ux = max(max(to, te), fl);
            X[k] = ux;
          }
          H[k] = h;
          up = h;
          hv[k] = h & vmask[k];
        }
        botH = H[AL_K - 1];
        botX = ux;
        if constexpr (DIRS) {
          dirs[((size_t)s * nsteps + st) * 64 + lane] = bits;
        } else {
          const int32_t hm = max(max(hv[0], hv[1]), max(hv[2], hv[3]));
          // (a lane meets a column's rows in rising order: an equal value in the same column
          // never replaces)
          if (hm > best || (hm == best && j < bj)) {
            best = hm;
            bj = j;
            const uint32_t k = hv[0] == hm ? 0u : hv[1] == hm ? 1u : hv[2] == hm ? 2u : 3u;
            bi = s * 256u + (uint32_t)lane * AL_K + k;
          }
        }
      }
      prevUpH = upH;
      if (seg_out) {  // lane 63's bottom row of column st - 63 -> eout
        const uint32_t c = st - 63;
        if (st >= 63) {
          const int32_t vh = __builtin_amdgcn_readlane(botH, 63);
          const int32_t vx = __builtin_amdgcn_readlane(botX, 63);
          const bool here = (uint32_t)lane == (c & 63);
          obuf.x = here ? (uint32_t)vh : obuf.x;
          obuf.y = here ? (uint32_t)vx : obuf.y;
          if ((c & 63) == 63 || c + 1 == L) {
            const uint32_t col = (c & ~63u) + lane;
            if (col < L) eout[col] = obuf;
          }
        }
      }
    }
    // the next strip's loads follow these stores in the same wave (score_i32)
    if (seg_out) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  if constexpr (!DIRS) {
    // the wave's best cell: highest value, then lowest column, then lowest row
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int32_t ob = __shfl_xor(best, off);
      const uint32_t oj = (uint32_t)__shfl_xor((int)bj, off);
      const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off);
      if (ob > best || (ob == best && (oj < bj || (oj == bj && oi < bi)))) {
        best = ob;
        bj = oj;
        bi = oi;
      }
    }
  }
}

__device__ __forceinline__ void al_load_matrix(const AlignArgs& a, int8_t* smat) {
  for (uint32_t i = threadIdx.x; i < a.alpha * a.alpha; i += blockDim.x) smat[i] = a.mat[i];
  __syncthreads();
}
// The matrix and its column complement: smat[1][q * A + c] scores q against the complement of c.
__device__ __forceinline__ void al_load_matrices(const AlignArgs& a,
                                                 int8_t (&smat)[2][AL_LETTERS * AL_LETTERS]) {
  for (uint32_t i = threadIdx.x; i < a.alpha * a.alpha; i += blockDim.x) {
    const uint32_t q = i / a.alpha, c = i % a.alpha, cc = al_comp(c);
    smat[0][i] = a.mat[i];
    smat[1][i] = a.mat[q * a.alpha + (cc < a.alpha ? cc : c)];
  }
  __syncthreads();
}

// Passes A and B: score and end cell (forward), start cell (the same walk over the reversed
// prefixes q[q_end..0] x t[t_end..0]); writes the hit's whole record, without a path.
// SET: the hit's own query of a set; a hit that names no pair gets its record here (index = id =
// SW_HIT_NONE, SW_ALIGN_EMPTY | SW_ALIGN_NO_HIT) and nothing of the batch is read for it.
template <bool GOTOH, bool SET, bool STRAND = false>
__global__ void __launch_bounds__(256) align_ends(const AlignArgs a) {
  static_assert(SET || !STRAND, "the strand kernels are set kernels");
  __shared__ uint2 lp[4][AL_LETTERS][64];
  __shared__ int8_t smats[STRAND ? 2 : 1][AL_LETTERS * AL_LETTERS];
  if constexpr (STRAND) al_load_matrices(a, smats);
  else al_load_matrix(a, smats[0]);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t gw = (size_t)blockIdx.x * 4 + wave, GW = (size_t)gridDim.x * 4;
  uint2* const scr[2] = {a.scratch + gw * 2 * a.scols, a.scratch + gw * 2 * a.scols + a.scols};
  for (size_t h = gw; h < a.n_hits; h += GW) {
    const uint64_t t = a.hits ? a.hits[h] : (uint64_t)h;
    const AlQuery qy = al_query<SET, true>(a, h);
    if constexpr (SET) {
      if (qy.len == AL_NO_QUERY || t >= a.n) {
        if (lane == 0) {
          sw_alignment r;
          r.index = r.id = SW_HIT_NONE;
          r.score = 0;
          r.flags = (uint32_t)SW_ALIGN_EMPTY | (uint32_t)SW_ALIGN_NO_HIT;
          r.q_start = r.q_end = r.t_start = r.t_end = 0u;
          r.n_columns = r.n_identities = 0;
          r.cigar_offset = a.cigar_stride ? (uint32_t)(h * a.cigar_stride) : 0u;
          r.cigar_len = 0;
          a.out[h] = r;
        }
        continue;
      }
    }
    uint32_t L = a.lens[t];
    const uint8_t* tp = a.res + (L ? a.offs[t] : 0);
    int32_t td = 1;  // the step along the target: -1 from its far end on the reverse strand
    const int8_t* smat = smats[0];
    if constexpr (STRAND) {
      if (L && __builtin_amdgcn_readfirstlane((int)al_reverse(a, h, t))) {
        tp += L - 1;
        td = -1;
        smat = smats[1];
      }
    }
    L = __builtin_amdgcn_readfirstlane(min(L, a.scols));
    int32_t score, rs;
    uint32_t qe, te, ri, rj;
    al_walk<GOTOH, false>(a, smat, lp[wave], scr, AlSeq{qy.p, tp, 1, td, qy.len, L}, nullptr,
                          score, qe, te);
    score = __builtin_amdgcn_readfirstlane(score);
    qe = __builtin_amdgcn_readfirstlane(qe);
    te = __builtin_amdgcn_readfirstlane(te);
    uint32_t qs = 0, ts = 0;
    if (score > 0) {
      al_walk<GOTOH, false>(a, smat, lp[wave], scr,
                            AlSeq{qy.p + qe, tp + (int64_t)td * te, -1, -td, qe + 1, te + 1},
                            nullptr, rs, ri, rj);
      qs = qe - min(ri, qe);
      ts = te - min(rj, te);
    }
    if (lane == 0) {
      sw_alignment r;
      r.index = t;
      r.id = a.ids ? a.ids[t] : t;
      r.score = score;
      r.flags = score > 0 ? (uint32_t)SW_ALIGN_NO_PATH : (uint32_t)SW_ALIGN_EMPTY;
      r.q_start = score > 0 ? qs : 0u;
      r.q_end = score > 0 ? qe : 0u;
      r.t_start = score > 0 ? ts : 0u;
      r.t_end = score > 0 ? te : 0u;
      r.n_columns = r.n_identities = 0;
      r.cigar_offset = a.cigar_stride ? (uint32_t)(h * a.cigar_stride) : 0u;
      r.cigar_len = 0;
      a.out[h] = r;
    }
  }
}

struct AlWindow {
  size_t h;
  const uint8_t* qp;  // the hit's query (valid when ok)
  uint32_t qs, ts, Q, L;
  uint64_t dir_off, cig_off;
  uint32_t cig_cap;
  bool ok;
};
// Position k's hit, window and places in the direction store and the CIGAR buffer; !ok when the
// hit has no path to store (score 0, a slot that names no pair, or a window past its slot).
template <bool SET, bool UNIFORM>
__device__ __forceinline__ AlWindow al_window(const AlignArgs& a, size_t k) {
  AlWindow w;
  w.h = a.list ? (size_t)a.list[k] : a.h0 + k;
  const sw_alignment& r = a.out[w.h];
  w.qs = r.q_start;
  w.ts = r.t_start;
  w.Q = r.q_end - r.q_start + 1;
  w.L = r.t_end - r.t_start + 1;
  uint64_t cap;
  if (a.plan) {
    w.dir_off = a.plan[k].dir_off;
    cap = a.plan[k].dir_cap;
    w.cig_off = a.plan[k].cig_off;
    w.cig_cap = a.plan[k].cig_cap;
  } else {
    w.dir_off = (uint64_t)k * a.slot;
    cap = a.slot;
    w.cig_off = (uint64_t)w.h * a.cigar_stride;
    w.cig_cap = a.cigar_stride;
  }
  w.qp = a.query;
  w.ok = r.score > 0 && r.q_end >= r.q_start && r.t_end >= r.t_start && w.L <= a.scols &&
         al_dir_dwords(w.Q, w.L) <= cap;
  if (w.ok) {  // (the record of a slot without a pair scores 0: its query is never looked up)
    const AlQuery qy = al_query<SET, UNIFORM>(a, w.h);
    w.qp = qy.p;
    w.ok = qy.len != AL_NO_QUERY && r.q_end < qy.len;
  }
  return w;
}

// Pass C: the direction store of each window.
template <bool GOTOH, bool SET, bool STRAND = false>
__global__ void __launch_bounds__(256) align_dirs(const AlignArgs a) {
  static_assert(SET || !STRAND, "the strand kernels are set kernels");
  __shared__ uint2 lp[4][AL_LETTERS][64];
  __shared__ int8_t smats[STRAND ? 2 : 1][AL_LETTERS * AL_LETTERS];
  if constexpr (STRAND) al_load_matrices(a, smats);
  else al_load_matrix(a, smats[0]);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t gw = (size_t)blockIdx.x * 4 + wave, GW = (size_t)gridDim.x * 4;
  uint2* const scr[2] = {a.scratch + gw * 2 * a.scols, a.scratch + gw * 2 * a.scols + a.scols};
  for (size_t k = gw; k < a.count; k += GW) {
    const AlWindow w = al_window<SET, true>(a, k);
    if (!w.ok) continue;
    const uint64_t t = a.out[w.h].index;
    const uint8_t* tp = a.res + a.offs[t] + w.ts;
    int32_t td = 1;
    const int8_t* smat = smats[0];
    if constexpr (STRAND) {
      if (__builtin_amdgcn_readfirstlane((int)al_reverse(a, w.h, t))) {
        tp = a.res + a.offs[t] + (a.lens[t] - 1 - w.ts);
        td = -1;
        smat = smats[1];
      }
    }
    int32_t b0;
    uint32_t b1, b2;
    al_walk<GOTOH, true>(a, smat, lp[wave], scr,
                         AlSeq{w.qp + w.qs, tp, 1, td,
                               (uint32_t)__builtin_amdgcn_readfirstlane(w.Q),
                               (uint32_t)__builtin_amdgcn_readfirstlane(w.L)},
                         a.dirs + w.dir_off, b0, b1, b2);
  }
}

// Pass D: one lane per hit follows the bits from the end cell to the start cell, counts columns
// and identities, emits run-length ops backwards and reverses them in place.
template <bool GOTOH, bool SET, bool STRAND = false>
__global__ void __launch_bounds__(64) align_path(const AlignArgs a) {
  static_assert(SET || !STRAND, "the strand kernels are set kernels");
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (k >= a.count) return;
  const AlWindow w = al_window<SET, false>(a, k);
  if (!w.ok || w.cig_cap == 0) return;
  sw_alignment& r = a.out[w.h];
  const uint8_t* tp = a.res + a.offs[r.index] + w.ts;
  [[maybe_unused]] bool rv = false;  // the reverse strand: column j is the complement of tp[-j]
  if constexpr (STRAND) {
    rv = al_reverse(a, w.h, r.index);
    if (rv) tp = a.res + a.offs[r.index] + (a.lens[r.index] - 1 - w.ts);
  }
  const uint8_t* qp = w.qp + w.qs;
  const uint8_t* db = reinterpret_cast<const uint8_t*>(a.dirs + w.dir_off);
  uint32_t* cig = a.cigar + w.cig_off;
  const uint64_t nsteps = (uint64_t)w.L + 63;
  int64_t i = (int64_t)w.Q - 1, j = (int64_t)w.L - 1;
  uint32_t nops = 0, cur = 0, run = 0, cols = 0, idn = 0;
  int state = 3;  // 0 H, 1 E / gap, 2 F, 3 a forced diagonal (the end column; merged: an open)
  bool done = false;
  const auto emit = [&](uint32_t code) {
    if (run && code == cur) {
      ++run;
    } else {
      if (run) {
        if (nops < w.cig_cap) cig[nops] = run << 4 | cur;
        ++nops;
      }
      cur = code;
      run = 1;
    }
    ++cols;
  };
  for (uint64_t it = 0, lim = (uint64_t)w.Q + w.L + 2; it < lim && i >= 0 && j >= 0; ++it) {
    const uint32_t ln = ((uint32_t)i & 255u) >> 2;
    const uint32_t bits =
        db[(((uint64_t)i >> 8) * nsteps + (uint64_t)j + ln) * 256 + ln * 4 + ((uint32_t)i & 3u)];
    if (state == 0) {
      if constexpr (GOTOH) state = (bits & 3u) == 0 ? 3 : (bits & 3u) == 1 ? 1 : 2;
      else state = (bits & 1u) ? 1 : 3;
    }
    if (state == 3) {
      emit(SW_CIGAR_M);
      if constexpr (STRAND) idn += qp[i] == (rv ? al_comp(tp[-j]) : (uint32_t)tp[j]);
      else idn += qp[i] == tp[j];
      if (i == 0 && j == 0) {
        done = true;
        break;
      }
      --i;
      --j;
      state = 0;
    } else if constexpr (GOTOH) {
      if (state == 1) {
        emit(SW_CIGAR_D);
        --j;
        state = (bits & 4u) ? 1 : 0;
      } else {
        emit(SW_CIGAR_I);
        --i;
        state = (bits & 8u) ? 2 : 0;
      }
    } else {  // merged: the gap value of (i, j) came from T above or T to the left
      if (bits & 2u) {
        emit(SW_CIGAR_I);
        --i;
      } else {
        emit(SW_CIGAR_D);
        --j;
      }
      if (i < 0 || j < 0) break;
      const uint32_t l2 = ((uint32_t)i & 255u) >> 2;
      const uint32_t b2 =
          db[(((uint64_t)i >> 8) * nsteps + (uint64_t)j + l2) * 256 + l2 * 4 + ((uint32_t)i & 3u)];
      state = (b2 & 4u) ? 1 : 3;  // T extends the gap, or opened from this cell's M
    }
  }
  if (run) {
    if (nops < w.cig_cap) cig[nops] = run << 4 | cur;
    ++nops;
  }
  if (!done || nops > w.cig_cap) return;  // SW_ALIGN_NO_PATH stays
  for (uint32_t x = 0; x < nops / 2; ++x) {
    const uint32_t v = cig[x];
    cig[x] = cig[nops - 1 - x];
    cig[nops - 1 - x] = v;
  }
  r.flags = 0;
  r.n_columns = cols;
  r.n_identities = idn;
  r.cigar_len = nops;
}

// After the last pass: a reverse-strand hit gets SW_ALIGN_REVERSE and, when it scored, its
// target coordinates on the forward target (t_start = L - 1 - t_end', t_end = L - 1 - t_start').
__global__ void __launch_bounds__(256) align_flip(const AlignArgs a) {
  const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= a.n_hits) return;
  sw_alignment& r = a.out[h];
  if ((r.flags & (uint32_t)SW_ALIGN_NO_HIT) || !al_reverse(a, h, r.index)) return;
  r.flags |= (uint32_t)SW_ALIGN_REVERSE;
  if (r.score <= 0) return;
  const uint32_t L = a.lens[r.index], ts = r.t_start, te = r.t_end;
  r.t_start = L - 1 - te;
  r.t_end = L - 1 - ts;
}
}  // namespace swk

extern "C" uint64_t swk_align_dir_dwords(uint32_t rows, uint32_t cols) {
  return swk::al_dir_dwords(rows, cols);
}

static swk::AlignArgs align_args(const SwkAlign* p) {
  swk::AlignArgs a{};
  a.res = p->res;
  a.offs = p->offs;
  a.lens = p->lens;
  a.ids = p->ids;
  a.hits = p->hits;
  a.n_hits = p->n_hits;
  a.query = p->query;
  a.qlen = p->qlen;
  a.mat = p->mat;
  a.alpha = p->alpha;
  a.pad = p->pad;
  a.padscore = p->padscore;
  a.O = p->O;
  a.E = p->E;
  a.out = static_cast<sw_alignment*>(p->out);
  a.cigar = p->cigar;
  a.cigar_stride = p->cigar_stride;
  a.scratch = static_cast<uint2*>(p->scratch);
  a.scols = p->scols;
  a.qtab = p->qtab;
  a.hit_queries = p->hit_queries;
  a.nq = p->nq;
  a.hits_per_query = p->hits_per_query;
  a.n = p->n;
  a.strands = p->strands;
  a.strand_by_hit = p->strand_by_hit ? 1u : 0u;
  return a;
}

static bool align_args_ok(const SwkAlign* p) {
  return p && p->alpha >= 1 && p->alpha < (uint32_t)swk::AL_LETTERS &&
         p->pad < (uint32_t)swk::AL_LETTERS && p->waves && p->waves % 4 == 0 && p->scols &&
         (!p->set || (p->qtab && p->nq && (p->hit_queries != nullptr) != (p->hits_per_query != 0) &&
                      p->n_hits <= 0xFFFFFFFFull)) &&
         (!p->strands || p->set);
}

// Passes A and B for hits [0, n_hits): every record written, paths left out.
extern "C" hipError_t swk_launch_align_ends(const SwkAlign* p, hipStream_t st) {
  if (!p || p->n_hits == 0) return hipSuccess;
  if (!align_args_ok(p)) return hipErrorInvalidValue;
  const swk::AlignArgs a = align_args(p);
  const dim3 grid((unsigned)(p->waves / 4));
  // (the single-query kernels are their own instantiation: the set's lookups cost them nothing)
  if (p->strands && p->gotoh)
    hipLaunchKernelGGL((swk::align_ends<true, true, true>), grid, dim3(256), 0, st, a);
  else if (p->strands)
    hipLaunchKernelGGL((swk::align_ends<false, true, true>), grid, dim3(256), 0, st, a);
  else if (p->gotoh && p->set)
    hipLaunchKernelGGL((swk::align_ends<true, true>), grid, dim3(256), 0, st, a);
  else if (p->gotoh)
    hipLaunchKernelGGL((swk::align_ends<true, false>), grid, dim3(256), 0, st, a);
  else if (p->set)
    hipLaunchKernelGGL((swk::align_ends<false, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((swk::align_ends<false, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// Passes C and D for `count` positions (hit list[k], or h0 + k) whose windows sit at plan[k], or
// in slots of `slot` dwords, of the direction store `dirs`.
extern "C" hipError_t swk_launch_align_paths(const SwkAlign* p, const uint32_t* list, size_t h0,
                                             size_t count, const SwkAlignPlan* plan,
                                             uint64_t slot, uint32_t* dirs, hipStream_t st) {
  if (!p || count == 0) return hipSuccess;
  if (!align_args_ok(p) || !dirs || !p->cigar) return hipErrorInvalidValue;
  swk::AlignArgs a = align_args(p);
  a.list = list;
  a.h0 = h0;
  a.count = count;
  a.plan = plan;
  a.slot = slot;
  a.dirs = dirs;
  const dim3 grid((unsigned)(std::min<size_t>(p->waves, (count + 3) / 4 * 4) / 4));
  const dim3 pgrid((unsigned)((count + 63) / 64));
  if (p->strands && p->gotoh) {
    hipLaunchKernelGGL((swk::align_dirs<true, true, true>), grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL((swk::align_path<true, true, true>), pgrid, dim3(64), 0, st, a);
  } else if (p->strands) {
    hipLaunchKernelGGL((swk::align_dirs<false, true, true>), grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL((swk::align_path<false, true, true>), pgrid, dim3(64), 0, st, a);
  } else if (p->gotoh && p->set) {
    hipLaunchKernelGGL((swk::align_dirs<true, true>), grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL((swk::align_path<true, true>), pgrid, dim3(64), 0, st, a);
  } else if (p->gotoh) {
    hipLaunchKernelGGL((swk::align_dirs<true, false>), grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL((swk::align_path<true, false>), pgrid, dim3(64), 0, st, a);
  } else if (p->set) {
    hipLaunchKernelGGL((swk::align_dirs<false, true>), grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL((swk::align_path<false, true>), pgrid, dim3(64), 0, st, a);
  } else {
    hipLaunchKernelGGL((swk::align_dirs<false, false>), grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL((swk::align_path<false, false>), pgrid, dim3(64), 0, st, a);
  }
  return hipGetLastError();
}

// The strand call's last launch: SW_ALIGN_REVERSE and the forward target coordinates of the
// reverse-strand hits of [0, n_hits).
extern "C" hipError_t swk_launch_align_flip(const SwkAlign* p, hipStream_t st) {
  if (!p || p->n_hits == 0 || !p->strands) return hipSuccess;
  if (!align_args_ok(p)) return hipErrorInvalidValue;
  const swk::AlignArgs a = align_args(p);
  hipLaunchKernelGGL(swk::align_flip, dim3((unsigned)((p->n_hits + 255) / 256)), dim3(256), 0, st,
                     a);
  return hipGetLastError();
}
