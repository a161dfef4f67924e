// swbank_kfswalk.h — the three-frame walk of the frameshift-tolerant translated search, shared by
// its score kernel (swbank_kfshift.hip) and by the kernels that align its hits
// (swbank_kfsalign.hip); include/swbank.h "frameshift-tolerant translated search", DESIGN.md §3.16.
//
// A wave walks one matrix: some rows of a query against the codons of some columns of a strand.
// Lane l owns the K rows [lK, lK + K) and walks anti-diagonals as the wave kernel of §3.2 does: at
// step t it is at codon index j = t - l and computes the three columns p = 3j, 3j + 1, 3j + 2
// (frames 0, 1, 2) of its rows, in that order.  In these terms the links of the recurrence read
// row i - 1 at
//     p - 3: the same frame at j - 1
//     p - 2: frame 1 at j - 1 (f = 0), frame 2 at j - 1 (f = 1), frame 0 at j (f = 2)
//     p - 4: frame 2 at j - 2 (f = 0), frame 0 at j - 1 (f = 1), frame 1 at j - 1 (f = 2)
// so a row keeps seven words between steps (H of the three frames at j - 1, H of frame 2 at
// j - 2, E of the three frames), F and the new H run down the rows of a step in registers, and
// the bottom row's new H and F (six words) move one lane down per step with DPP wave_shr:1; the
// receiving lane keeps the last two H triples and the frame-2 H before them.  The three amino
// acids of a codon index travel down the lanes the same way, packed in one word; every 64 steps
// the lanes translate the next 64 codon indices together and lane 0 takes them one per step.
//
// All arithmetic is int32: scores are exact with no width limit.  No masks are needed: rows past
// the matrix's, codon indices before its first column and past its last, and the frames of the
// last index that run past it all read the score FS_PAD (<= every matrix entry, < 0), under which
// H there is at most an H of a real cell (M = pad + max(0, H' ...) < max(0, H' ...), E and F are an
// H minus a penalty), and is 0 before the start, where every H is 0: E of such a cell is o, which
// is E of a real cell whose left neighbour lies outside the matrix.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swk {
constexpr int FS_AMINO = 24;       // the profile's real columns (SW_PROTEIN_ALPHA)
constexpr uint32_t FS_OFF = 24;    // the column of a codon outside the matrix
constexpr uint32_t FS_X = 22;      // a codon holding N (or any code past it)
constexpr int32_t FS_PAD = -128;   // rows past the matrix's, codons outside it
constexpr int32_t FS_NEG = -(1 << 29);
constexpr uint32_t FS_OFFW = FS_OFF | FS_OFF << 8 | FS_OFF << 16;

// Rows per lane for queries of at most qlen rows: 4, 8 or 16 (SW_FSHIFT_MAX_QUERY = 64 x 16).
__host__ __device__ inline int fs_rows(uint32_t qlen) {
  return qlen <= 256 ? 4 : qlen <= 512 ? 8 : 16;
}
// The penalties every entry takes: open + extend, extend, frameshift.
inline bool fs_penalties_ok(int32_t o, int32_t e, int32_t fs) {
  return o <= 0 && e <= 0 && fs <= 0 && o >= -65534 && e >= -32767 && fs >= -32767;
}
// 64 amino acids, c0 * 16 + c1 * 4 + c2, as little-endian words: byte i of the table is byte i of
// the words in LDS.
struct FsTable {
  uint32_t w[16];
};
inline FsTable fs_table(const uint8_t* table) {
  FsTable t;
  for (int i = 0; i < 16; ++i)
    t.w[i] = (uint32_t)table[4 * i] | (uint32_t)table[4 * i + 1] << 8 |
             (uint32_t)table[4 * i + 2] << 16 | (uint32_t)table[4 * i + 3] << 24;
  return t;
}

__device__ __forceinline__ int32_t fs_shr1(int32_t lane0_value, int32_t v) {  // wave_shr:1
  return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int32_t fs_max3(int32_t a, int32_t b, int32_t c) {
  return max(max(a, b), c);
}
// The amino acid of the codon c0 c1 c2 (codes of the strand read).
__device__ __forceinline__ uint32_t fs_codon(const uint8_t* tab, uint32_t c0, uint32_t c1,
                                             uint32_t c2) {
  const bool ok = (c0 | c1 | c2) < 4;  // all three are T, C, A or G
  return ok ? tab[c0 * 16 + c1 * 4 + c2] : FS_X;
}

// prof[c][row], row < 64K: the score of the matrix's row `row` (query code qp[row * qstep], row <
// rows) against amino acid c; FS_PAD past the rows and in column FS_OFF.  All `nthreads` threads
// of the workgroup call it; the caller synchronises.
template <int K>
__device__ __forceinline__ void fs_profile(const int8_t* mat, uint32_t alpha, int8_t* prof,
                                           const uint8_t* qp, int32_t qstep, uint32_t rows,
                                           uint32_t nthreads) {
  constexpr int ROWS = 64 * K;
  for (uint32_t row = threadIdx.x; row < (uint32_t)ROWS; row += nthreads) {
    const bool in_q = row < rows;
    const uint32_t q = in_q ? qp[(int64_t)row * qstep] : 0u;
    const int8_t* mr = mat + (q < alpha ? q : 0u) * alpha;
#pragma unroll
    for (int c = 0; c < FS_AMINO; ++c)
      prof[c * ROWS + row] = in_q && (uint32_t)c < alpha ? mr[c] : (int8_t)FS_PAD;
    prof[FS_OFF * ROWS + row] = (int8_t)FS_PAD;
  }
}

// Direction byte of a cell: bits 0-1 the source of H (0 M, 1 E, 2 F), bits 2-3 the link of M
// (0 the start, 1 p - 3, 2 p - 2, 3 p - 4), bit 4 E extends, bit 5 F extends.  Ties: M, then E,
// then F; p - 3, then p - 2, then p - 4; a gap opens rather than extends.

// One cell.  d3, bk, sk: H of the row above at p - 3, p - 2, p - 4; hl, el: H and E of this row at
// p - 3; nu, fu: H and F of the row above at p.  DIRS: the anchored matrix (no floor; `first`: the
// window's first cell, whose diagonal is 0) and the cell's direction byte.
template <bool DIRS>
__device__ __forceinline__ void fs_cell(int32_t s, int32_t d3, int32_t bk, int32_t sk, bool first,
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
    E = max(E, FS_NEG);
    F = max(F, FS_NEG);
    const int32_t M = s + (first ? 0 : max(d3, sh));
    H = fs_max3(M, E, F);
    const uint32_t link = first ? 0u : d3 >= sh ? 1u : bk >= sk ? 2u : 3u;
    const uint32_t src = H == M ? 0u : H == E ? 1u : 2u;
    dir = src | link << 2 | (ex > eo ? 16u : 0u) | (fx > fo ? 32u : 0u);
  } else {
    const int32_t M = s + fs_max3(0, d3, sh);
    H = max(fs_max3(0, M, E), F);
  }
}

// What a walk records, and returns.
//   Score  the local matrix; an int32_t, this lane's highest H.  (A plain value: out of a struct
//          the compiler cannot tell that it is no poison value, freezes it for the butterfly that
//          follows, drops the no-wrap flags of every add behind it, and the kernels take 4 to 11
//          VGPRs more.)
//   Best   the local matrix; an FsBest, the best cell: the highest H, then the smallest column,
//          then the smallest row; v = 0 when no cell is positive.  The same in every lane.
//   Dirs   the anchored matrix; per cell one direction byte, stored by walk step: at step t lane l
//          writes its 3K bytes (frame-major) as 3K/4 dwords at dirs[t][word][lane].  Nothing.
enum class FsMode { Score, Best, Dirs };
struct FsBest {
  int32_t v;
  uint32_t c, i;
};
__host__ __device__ inline uint64_t fs_dir_dwords(int K, uint32_t rows, uint32_t cols) {
  if (rows == 0 || cols == 0) return 0;
  const uint64_t J = ((uint64_t)cols + 2) / 3, nl = ((uint64_t)rows + K - 1) / K;
  return (J + nl - 1) * (uint64_t)(48 * K);
}

// The walk of one wave over `rows` rows (the profile's) and J codon indices; aminos(j), j < J,
// gives the amino acids of index j, frame f at bits 8f, FS_OFF for a frame past the last column.
template <int K, FsMode MODE, class Aminos>
__device__ __forceinline__ auto fs_walk(const int8_t* prof, const Aminos& aminos, uint32_t J,
                                        uint32_t rows, int32_t o, int32_t e, int32_t fs,
                                        uint32_t* dirs) {
  constexpr int ROWS = 64 * K;
  constexpr bool DIRS = MODE == FsMode::Dirs;
  constexpr int32_t OUT = DIRS ? FS_NEG : 0;  // H outside the matrix
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nl = (rows + K - 1) / K;     // lanes that hold rows
  const uint32_t steps = J && nl ? J + nl - 1 : 0u;

  int32_t h0[K], h1[K], h2[K], g2[K], e0[K], e1[K], e2[K];
#pragma unroll
  for (int r = 0; r < K; ++r) {
    h0[r] = h1[r] = h2[r] = g2[r] = OUT;
    e0[r] = e1[r] = e2[r] = FS_NEG;
  }
  // the row above this lane's first: H and F of the three frames at this step's codon index (un,
  // uf), H at the index before it (ud), H of frame 2 two indices back (udd2)
  int32_t un0 = OUT, un1 = OUT, un2 = OUT, uf0 = FS_NEG, uf1 = FS_NEG, uf2 = FS_NEG;
  int32_t ud0 = OUT, ud1 = OUT, ud2 = OUT, udd2 = OUT;
  // Score: best0 is the best H of all three frames.  Best: the best H per frame and its place,
  // step << 4 | row; within a frame the visiting order is column-major, so the first best is the
  // rule's
  int32_t best0 = 0;
  [[maybe_unused]] int32_t best1 = 0, best2 = 0;
  [[maybe_unused]] uint32_t pos0 = 0, pos1 = 0, pos2 = 0;
  uint32_t aw = FS_OFFW;  // this lane's three amino acids
  const int8_t* myprof = prof + lane * K;

  for (uint32_t t0 = 0; t0 < steps; t0 += 64) {
    const uint32_t jn = t0 + lane;
    const uint32_t nxt = jn < J ? aminos(jn) : FS_OFFW;
    const uint32_t cnt = min(64u, steps - t0);
    for (uint32_t s = 0; s < cnt; ++s) {
      aw = (uint32_t)fs_shr1(__builtin_amdgcn_readlane((int32_t)nxt, (int)s), (int32_t)aw);
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
      [[maybe_unused]] const uint32_t t = t0 + s;
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
        fs_cell<DIRS>(s0, d0, d1, dd2, r == 0 && start, h0[r], e0[r], n0, f0, o, e, fs, H0, E0, F0,
                      b0);
        // frame 1: p - 3 frame 1 at j - 1, p - 2 frame 2 at j - 1, p - 4 frame 0 at j - 1
        fs_cell<DIRS>(s1, d1, d2, d0, false, h1[r], e1[r], n1, f1, o, e, fs, H1, E1, F1, b1);
        // frame 2: p - 3 frame 2 at j - 1, p - 2 frame 0 at j (the row above, this step),
        // p - 4 frame 1 at j - 1
        fs_cell<DIRS>(s2, d2, n0, d1, false, h2[r], e2[r], n2, f2, o, e, fs, H2, E2, F2, b2);
        if constexpr (MODE == FsMode::Score) {
          best0 = max(fs_max3(best0, H0, H1), H2);
        } else if constexpr (MODE == FsMode::Best) {
          const uint32_t at = t << 4 | (uint32_t)r;
          pos0 = H0 > best0 ? at : pos0;
          best0 = max(best0, H0);
          pos1 = H1 > best1 ? at : pos1;
          best1 = max(best1, H1);
          pos2 = H2 > best2 ? at : pos2;
          best2 = max(best2, H2);
        } else {
          dw[r / 4] |= b0 << (8 * (r % 4));
          dw[K / 4 + r / 4] |= b1 << (8 * (r % 4));
          dw[2 * (K / 4) + r / 4] |= b2 << (8 * (r % 4));
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
      un0 = fs_shr1(OUT, n0);
      un1 = fs_shr1(OUT, n1);
      un2 = fs_shr1(OUT, n2);
      uf0 = fs_shr1(FS_NEG, f0);
      uf1 = fs_shr1(FS_NEG, f1);
      uf2 = fs_shr1(FS_NEG, f2);
    }
  }
  if constexpr (MODE == FsMode::Score) {
    return best0;
  } else if constexpr (MODE == FsMode::Best) {
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
    return FsBest{__builtin_amdgcn_readfirstlane(v), (uint32_t)__builtin_amdgcn_readfirstlane(c),
                  (uint32_t)__builtin_amdgcn_readfirstlane(i)};
  }
}
}  // namespace swk
