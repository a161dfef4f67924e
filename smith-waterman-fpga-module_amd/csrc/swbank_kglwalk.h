// swbank_kglwalk.h — the walk of the global-local search's score kernel (swbank_kglocal.hip) and
// of the aligner of its hits (swbank_kglalign.hip); include/swbank.h "global-local search",
// DESIGN.md §3.17 and §3.18.
//
// A wave walks one matrix: the m rows of a query against the L columns of a strand, under the
// Gotoh recurrence WITHOUT a floor and with the penalised boundaries that `ENDS` selects.  Lane l
// owns the K rows [lK, lK + K) and walks anti-diagonals as the frameshift walk of
// swbank_kfswalk.h does: at step t it is at column j = t - l.  A row keeps three words between
// steps (H, H + o and E at j - 1); F and the new H run down the rows of a step in registers; the bottom
// row's new H and F move one lane down per step with DPP wave_shr:1, where the receiving lane
// also keeps the H before it for its diagonal.  The target codes travel down the lanes the same
// way: every 64 steps the lanes fetch the next 64 codes together and lane 0 takes them one per
// step with v_readlane.  All arithmetic is int32.
//
// What differs from the local walks, and why the result is exact:
//
//   -infinity.  E and F outside the matrix are -infinity in the definition.  The walk starts them
//     at E(i,-1) = H(i,-1) + o - e and F(-1,j) = H(-1,j) + o - e: the first cell then forms
//     max(H + o, (H + o - e) + e), a tie, which is what -infinity gives.  No value leaves the
//     range the entry's rule guarantees, and no cell needs a floor.
//
//   Lanes outside their columns.  A lane computes a step only while 0 <= j < L and while it holds
//     a row of the query (one unsigned compare, (t - l) < L or 0; the cells sit under that branch,
//     the DPP moves outside it).  Before its first column a lane therefore still holds what it was
//     initialised with, the boundary column H(i,-1) and E(i,-1), and hands down H(i,-1) of its
//     bottom row: the lane below takes exactly that for the diagonal of its first cell, one step
//     after it arrived.  Whatever an idle lane hands down is read by an idle lane only: lane l + 1
//     reads at step t what lane l made at step t - 1, and it computes at t only if t - 1 - l lies
//     in [0, L) as well, except for that diagonal.  Pad columns are never computed; the pad rows
//     of the last lane (scored -128) lie below every real row, and links only run down and right.
//
//   Where the result is taken.  QUERY: row m - 1 only, in lane (m - 1) / K, at every step of that
//     lane, strictly-greater so the smallest column stays; it starts from H(m-1,-1).  TARGET:
//     column L - 1 only, at the one step t = L - 1 + l of each lane, rows below m, strictly
//     greater in row order; H(-1,L-1) is lane 0's start.  BOTH: that step, row m - 1 alone.
//     Positions are kept as index + 1, so the boundary (index -1) is 0 and wins every tie; the
//     lanes are merged by value, then by the smaller position.
//
// The aligner of global-local hits (swbank_kglalign.hip) runs the same walk in
// two more modes (GlMode): `Anchored` penalises both boundaries whatever ENDS says and takes the
// result as ENDS does (QUERY: the last row; TARGET: the last column), which is what finds a hit's
// start on the reversed rows and columns; `Dirs` (ENDS = BOTH) stores one direction byte per cell.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swk {
constexpr int GL_MAX_ALPHA = 24;   // the profile's columns (SW_PROTEIN_ALPHA)
constexpr int32_t GL_PAD = -128;   // rows past the query's
constexpr int GL_QUERY = 1, GL_TARGET = 2, GL_BOTH = 3;  // SW_ENDS_*

// Rows per lane for queries of at most qlen rows: 4, 8 or 16 (SW_GLOCAL_MAX_QUERY = 64 x 16).
__host__ __device__ inline int gl_rows(uint32_t qlen) {
  return qlen <= 256 ? 4 : qlen <= 512 ? 8 : 16;
}

__device__ __forceinline__ int32_t gl_shr1(int32_t lane0_value, int32_t v) {  // wave_shr:1
  return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xF, 0xF, false);
}

// prof[c][row], row < 64K: the score of query row `row` against target code c < alpha; GL_PAD past
// the query.  All `nthreads` threads of the workgroup call it; the caller synchronises.
// STEP = -1 reads the query backwards from qp (the rows of a reversed walk).
template <int K, int STEP = 1>
__device__ __forceinline__ void gl_profile(const int8_t* mat, uint32_t alpha, int8_t* prof,
                                           const uint8_t* qp, uint32_t rows, uint32_t nthreads) {
  constexpr int ROWS = 64 * K;
  for (uint32_t row = threadIdx.x; row < (uint32_t)ROWS; row += nthreads) {
    const bool in_q = row < rows;
    const uint32_t q = in_q ? qp[STEP == 1 ? (int32_t)row : STEP * (int32_t)row] : 0u;
    const int8_t* mr = mat + (q < alpha ? q : alpha - 1) * alpha;
    for (uint32_t c = 0; c < alpha; ++c) prof[c * ROWS + row] = in_q ? mr[c] : (int8_t)GL_PAD;
  }
}

// Score: the search's walk, boundaries and result by ENDS.  Anchored: both boundaries penalised,
// the result where ENDS takes it.  Dirs: the anchored matrix (ENDS = GL_BOTH) with one direction
// byte per cell, stored by walk step: at step t lane l writes its K bytes as K / 4 dwords at
// dirs[t][word][lane], one coalesced store per word.
enum class GlMode { Score, Anchored, Dirs };
// A direction byte: bits 0-1 the source of H (M, then E, then F on a tie), GL_E_EXT / GL_F_EXT:
// E / F extends (strictly better than opening: a gap run opens when both are optimal).
constexpr uint32_t GL_SRC_M = 0, GL_SRC_E = 1, GL_SRC_F = 2, GL_E_EXT = 16, GL_F_EXT = 32;

// Dwords of direction store a window of rows x cols cells takes at K rows per lane.
__host__ __device__ inline uint64_t gl_dir_dwords(int K, uint32_t rows, uint32_t cols) {
  if (rows == 0 || cols == 0) return 0;
  return ((uint64_t)cols + ((uint64_t)rows + K - 1) / K - 1) * (uint64_t)(K / 4) * 64;
}

struct GlBest {
  int32_t v;     // the strand's score
  uint32_t pos;  // its end index + 1; 0: the boundary (SW_END_NONE)
};

// The walk of one wave over m rows (1 <= m <= 64K, the profile's) and L columns; code(j), j < L,
// is the strand's code at column j (< alpha).  The same result in every lane.
template <int K, int ENDS, GlMode MODE = GlMode::Score, class Code>
__device__ __forceinline__ GlBest gl_walk(const int8_t* prof, const Code& code, uint32_t L,
                                          uint32_t m, int32_t o, int32_t e,
                                          uint32_t* dirs = nullptr) {
  constexpr int ROWS = 64 * K;
  constexpr bool SCORE = MODE == GlMode::Score, DIRS = MODE == GlMode::Dirs;
  static_assert(!DIRS || ENDS == GL_BOTH, "the direction store is the anchored matrix's");
  constexpr bool QB = !SCORE || ENDS != GL_TARGET;  // the query's boundary column is penalised
  constexpr bool TB = !SCORE || ENDS != GL_QUERY;   // the target's boundary row is penalised
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nl = (m + K - 1) / K;  // lanes that hold rows
  const uint32_t steps = L ? L + nl - 1 : 0u;
  const uint32_t mycols = lane < nl ? L : 0u;
  const uint32_t lq = (m - 1) / K, rq = (m - 1) % K;  // where row m - 1 lives
  const int32_t oe = o - e;

  int32_t h[K], ho[K], eg[K];  // H, H + o (what opening a gap from it gives) and E at j - 1
#pragma unroll
  for (int r = 0; r < K; ++r) {
    h[r] = QB ? o + (int32_t)(lane * K + r) * e : 0;  // H(i,-1)
    ho[r] = h[r] + o;
    eg[r] = h[r] + oe;                                // E(i,-1), see above
  }
  // the row above this lane's first: H and F at this step's column (un, uf), H at the column
  // before it (ud).  Lane 0: the boundary row, H(-1,0), F(-1,0) and H(-1,-1) = 0
  int32_t bt = TB ? o : 0;  // H(-1,t) of the step, then of the next one
  int32_t un = lane ? (QB ? o + (int32_t)(lane * K - 1) * e : 0) : bt;
  int32_t uf = bt + oe, ud = 0, fbot = 0;
  int32_t bv = INT32_MIN;
  uint32_t bp = 0;
  if (ENDS == GL_QUERY || L == 0) {
    // H(m-1,-1).  (L == 0, TARGET: the maximum over i of H(i,-1) = 0 is H(-1,-1), as here)
    bv = QB ? o + (int32_t)(m - 1) * e : 0;
  } else if (ENDS == GL_TARGET) {
    bv = lane == 0 ? o + (int32_t)(L - 1) * e : INT32_MIN;  // H(-1,L-1)
  }
  uint32_t cw = 0;  // this lane's target code
  const int8_t* myprof = prof + lane * K;

  for (uint32_t t0 = 0; t0 < steps; t0 += 64) {
    const uint32_t jn = t0 + lane;
    const uint32_t nxt = jn < L ? code(jn) : 0u;
    const uint32_t cnt = min(64u, steps - t0);
    for (uint32_t s = 0; s < cnt; ++s) {
      cw = (uint32_t)gl_shr1(__builtin_amdgcn_readlane((int32_t)nxt, (int)s), (int32_t)cw);
      const uint32_t j = t0 + s - lane;
      if (j < mycols) {
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(myprof + cw * ROWS);
        uint32_t w[K / 4];
#pragma unroll
        for (int i = 0; i < K / 4; ++i) w[i] = pw[i];
        // seven VALU a cell: H + o is formed once and opens both the gap to the right (the next
        // step's E) and the gap below (the next row's F)
        int32_t no = un + o, f = uf, d = ud;
        uint32_t dw[K / 4];
        if constexpr (DIRS) {
#pragma unroll
          for (int i = 0; i < K / 4; ++i) dw[i] = 0;
        }
#pragma unroll
        for (int r = 0; r < K; ++r) {
          const int32_t sc = (int32_t)(int8_t)(w[r / 4] >> (8 * (r % 4)));
          const int32_t E = max(ho[r], eg[r] + e);
          const int32_t F = max(no, f + e);
          const int32_t H = max(max(sc + d, E), F);
          if constexpr (DIRS) {
            // the -infinity start of E and F (see above) is a tie of open and extend here, and a
            // tie opens: the first cell of a row or a column never extends into the boundary
            const uint32_t src = sc + d == H ? GL_SRC_M : E == H ? GL_SRC_E : GL_SRC_F;
            const uint32_t bits = src | (eg[r] + e > ho[r] ? GL_E_EXT : 0u) |
                                  (f + e > no ? GL_F_EXT : 0u);
            dw[r / 4] |= bits << (8 * (r % 4));
          }
          d = h[r];
          h[r] = H;
          ho[r] = no = H + o;
          eg[r] = E;
          f = F;
        }
        fbot = f;
        if constexpr (DIRS) {
          uint32_t* at = dirs + (size_t)(t0 + s) * (K / 4) * 64 + lane;
#pragma unroll
          for (int i = 0; i < K / 4; ++i) at[(size_t)i * 64] = dw[i];
        }
        if constexpr (ENDS == GL_QUERY) {
          int32_t hq = h[0];
#pragma unroll
          for (int r = 1; r < K; ++r) hq = rq == (uint32_t)r ? h[r] : hq;
          const bool up = lane == lq && hq > bv;
          bv = up ? hq : bv;
          bp = up ? j + 1 : bp;
        } else if (j == L - 1) {
#pragma unroll
          for (int r = 0; r < K; ++r) {
            const uint32_t i = lane * K + r;
            const bool up = (ENDS == GL_BOTH ? i == m - 1 : i < m) && h[r] > bv;
            bv = up ? h[r] : bv;
            bp = up ? i + 1 : bp;
          }
        }
      }
      // the bottom row goes one lane down; above lane 0 lies the boundary row
      bt = TB ? bt + e : 0;
      ud = un;
      un = gl_shr1(bt, h[K - 1]);
      uf = gl_shr1(bt + oe, fbot);
    }
  }
  if (ENDS == GL_BOTH && L == 0) bp = 0;
#pragma unroll
  for (int dd = 32; dd >= 1; dd >>= 1) {
    const int32_t v2 = __shfl_xor(bv, dd, 64);
    const uint32_t p2 = (uint32_t)__shfl_xor((int32_t)bp, dd, 64);
    const bool better = v2 > bv || (v2 == bv && p2 < bp);
    bv = better ? v2 : bv;
    bp = better ? p2 : bp;
  }
  return GlBest{bv, ENDS == GL_BOTH ? 0u : bp};
}
}  // namespace swk
