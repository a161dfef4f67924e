// swbank_klawalk.h — the walk of the non-intersecting local aligner (swbank_klalign.hip);
// include/swbank.h "non-intersecting local alignments", DESIGN.md §3.19.
//
// A wave walks the whole matrix of one pair, the m rows of a query against the L columns of its
// target, under the local Gotoh recurrence with a set of used cells: a used cell has H = 0 and
// E = F = -infinity, so nothing passes through it.  The shape is that of gl_walk in mode Dirs
// (swbank_kglwalk.h), whose helpers it shares: lane l owns the K rows [lK, lK + K) and is at
// column j = t - l at step t; a row keeps H, H + o and E at j - 1 between steps; F and the new H
// run down the rows of a step in registers; the bottom row's H and F move one lane down per step
// with DPP wave_shr:1; every 64 steps the lanes fetch the next 64 target codes together.  All
// arithmetic is int32.
//
// What differs from gl_walk:
//
//   The floor and -infinity.  H = max(0, M, E, F); the boundaries are H = 0 and E = F = LA_NEG.
//     H >= 0 everywhere, so E(i,j) >= H(i,j-1) + o >= o: a LA_NEG never travels further than the
//     one cell beside a boundary or a used cell, where LA_NEG + e < o loses to opening.  o >=
//     -65,534 and e >= -32,767 (sw_set_matrix), so nothing leaves int32.
//
//   The direction byte.  One per cell of the whole matrix, in gl_walk's step-major layout
//     [t][word][lane].  Bits 0-1: the source of H, LA_SRC_ZERO first (H = 0 ends a path), then M,
//     E, F as in gl_walk; GL_E_EXT / GL_F_EXT; bit 7 (LA_USED): the cell belongs to an earlier
//     round's path.  The first round (FIRST) reads nothing.  A later round loads, one step ahead,
//     the dwords it is about to overwrite and keeps their bit 7; the path kernel's lane 0 sets the
//     bit on the cells it walks.  Every cell of the matrix is written by every round, so what the
//     store held before the first round does not matter.
//
//   Pad rows.  The rows past m in the last lane are treated as used in every round: they hold 0
//     and cannot be the best cell, and nothing runs up from them.
//
//   The best cell.  The end rule of sw_align_hits: the largest H, then the smallest column, then
//     the smallest row.  A lane visits its columns in order and compares the largest of a step's K
//     values once, strictly; the row is resolved under that (rare) branch.  The lanes are merged
//     by value, then column, then row.
#pragma once
#include "swbank_kglwalk.h"

namespace swk {
constexpr int32_t LA_NEG = -(1 << 30);
constexpr uint32_t LA_SRC_ZERO = 3, LA_USED = 0x80, LA_USED4 = 0x80808080u;

struct LaBest {
  int32_t v;      // the largest H of the matrix; 0: no cell is positive
  uint32_t j, i;  // its column and row under the end rule (v > 0)
};

// The walk of one wave over m rows (1 <= m <= 64K, the profile's) and L >= 1 columns; code(j),
// j < L, is the target's code at column j (< alpha).  dirs holds gl_dir_dwords(K, m, L) dwords.
// The same result in every lane.
template <int K, bool FIRST, class Code>
__device__ __forceinline__ LaBest la_walk(const int8_t* prof, const Code& code, uint32_t L,
                                          uint32_t m, int32_t o, int32_t e, uint32_t* dirs) {
  constexpr int ROWS = 64 * K;
  constexpr int W = K / 4;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nl = (m + K - 1) / K;  // lanes that hold rows
  const uint32_t steps = L + nl - 1;
  const uint32_t mycols = lane < nl ? L : 0u;

  int32_t h[K], ho[K], eg[K];  // H, H + o and E at j - 1
  uint32_t padm[W];            // bit 7 of the bytes of rows past m
#pragma unroll
  for (int i = 0; i < W; ++i) padm[i] = 0;
#pragma unroll
  for (int r = 0; r < K; ++r) {
    h[r] = 0;
    ho[r] = o;
    eg[r] = LA_NEG;
    padm[r / 4] |= lane * K + r >= m ? LA_USED << (8 * (r % 4)) : 0u;
  }
  // the row above this lane's first: H and F at this step's column (un, uf), H at the column
  // before it (ud); above lane 0 lies the boundary row
  int32_t un = 0, uf = LA_NEG, ud = 0, fbot = LA_NEG;
  int32_t bv = 0;
  uint32_t bj = 0, br = 0;
  uint32_t cw = 0;  // this lane's target code
  const int8_t* myprof = prof + lane * K;
  uint32_t* mydirs = dirs + lane;

  uint32_t pn[W];  // the previous round's bytes of the coming step
#pragma unroll
  for (int i = 0; i < W; ++i) pn[i] = FIRST ? 0u : mydirs[(size_t)i * 64];

  for (uint32_t t0 = 0; t0 < steps; t0 += 64) {
    const uint32_t jn = t0 + lane;
    const uint32_t nxt = jn < L ? code(jn) : 0u;
    const uint32_t cnt = min(64u, steps - t0);
    for (uint32_t s = 0; s < cnt; ++s) {
      cw = (uint32_t)gl_shr1(__builtin_amdgcn_readlane((int32_t)nxt, (int)s), (int32_t)cw);
      const uint32_t t = t0 + s;
      uint32_t ub[W];
#pragma unroll
      for (int i = 0; i < W; ++i) ub[i] = (pn[i] & LA_USED4) | padm[i];
      if constexpr (!FIRST) {
        // (every step below `steps` lies in the store, whichever lanes compute at it)
        if (t + 1 < steps) {
          const uint32_t* nx = mydirs + (size_t)(t + 1) * W * 64;
#pragma unroll
          for (int i = 0; i < W; ++i) pn[i] = nx[(size_t)i * 64];
        }
      }
      const uint32_t j = t - lane;
      if (j < mycols) {
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(myprof + cw * ROWS);
        uint32_t w[W], dw[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
          w[i] = pw[i];
          dw[i] = 0;
        }
        int32_t no = un + o, f = uf, d = ud, hm = 0;
#pragma unroll
        for (int r = 0; r < K; ++r) {
          const int32_t sc = (int32_t)(int8_t)(w[r / 4] >> (8 * (r % 4)));
          const int32_t E = max(ho[r], eg[r] + e);
          const int32_t F = max(no, f + e);
          const int32_t M = sc + d;
          const int32_t H = max(max(M, E), max(F, 0));
          const bool used = (ub[r / 4] >> (8 * (r % 4)) & LA_USED) != 0;
          // H = 0 ends a path whatever else ties with it; a tie of open and extend opens
          const uint32_t src = H == 0 ? LA_SRC_ZERO : M == H ? GL_SRC_M : E == H ? GL_SRC_E
                                                                                  : GL_SRC_F;
          const uint32_t bits = src | (eg[r] + e > ho[r] ? GL_E_EXT : 0u) |
                                (f + e > no ? GL_F_EXT : 0u);
          dw[r / 4] |= (used ? LA_USED | LA_SRC_ZERO : bits) << (8 * (r % 4));
          const int32_t Hn = used ? 0 : H;
          d = h[r];
          h[r] = Hn;
          ho[r] = no = Hn + o;
          eg[r] = used ? LA_NEG : E;
          f = used ? LA_NEG : F;
          hm = max(hm, Hn);
        }
        fbot = f;
        uint32_t* at = mydirs + (size_t)t * W * 64;
#pragma unroll
        for (int i = 0; i < W; ++i) at[(size_t)i * 64] = dw[i];
        if (hm > bv) {  // strictly: the smallest column stays; then the smallest row
          bv = hm;
          bj = j;
#pragma unroll
          for (int r = K - 1; r >= 0; --r) br = h[r] == hm ? (uint32_t)r : br;
        }
      }
      // the bottom row goes one lane down; above lane 0 lies the boundary row
      ud = un;
      un = gl_shr1(0, h[K - 1]);
      uf = gl_shr1(LA_NEG, fbot);
    }
  }
  uint32_t bi = lane * K + br;
#pragma unroll
  for (int dd = 32; dd >= 1; dd >>= 1) {
    const int32_t v2 = __shfl_xor(bv, dd, 64);
    const uint32_t j2 = (uint32_t)__shfl_xor((int32_t)bj, dd, 64);
    const uint32_t i2 = (uint32_t)__shfl_xor((int32_t)bi, dd, 64);
    const bool better = v2 > bv || (v2 == bv && (j2 < bj || (j2 == bj && i2 < bi)));
    bv = better ? v2 : bv;
    bj = better ? j2 : bj;
    bi = better ? i2 : bi;
  }
  return LaBest{bv, bj, bi};
}
}  // namespace swk
