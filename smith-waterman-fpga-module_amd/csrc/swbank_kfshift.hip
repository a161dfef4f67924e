// swbank_kfshift.hip — the score kernel of the frameshift-tolerant translated search
// (include/swbank.h "frameshift-tolerant translated search").
//
// A workgroup is two waves and owns one (query, target) pair: wave 0 scores the forward strand,
// wave 1 the reverse strand, read from the target's far end and complemented; the two meet once,
// at the end, to merge their scores.  Nothing waits across workgroups, so the hardware deals
// targets of any mix of lengths over the chip (a 70,000-nt target holds one workgroup, the short
// ones pass it by).
//
// Inside a wave lane l owns the K query rows [lK, lK + K) and walks anti-diagonals as the wave
// kernel of §3.2 does: at step t it is at codon index j = t - l and computes the three columns
// p = 3j, 3j + 1, 3j + 2 (frames 0, 1, 2) of its rows, in that order.  In these terms the links
// of the recurrence read row i - 1 at
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
// the query, codon indices before the target's start and past its end, and the frames of the last
// index that run past the target all read the score FS_PAD (<= every matrix entry, < 0), under
// which H there is at most an H of a real cell (M = pad + max(0, H' ...) < max(0, H' ...), E and F
// are an H minus a penalty), and is 0 before the start, where every H is 0: E of such a cell is
// o, which is E of a real cell whose left neighbour lies outside the matrix.
#include "swbank.h"
#include "swbank_kcommon.h"

namespace swk {
struct FsTable {  // 64 amino acids, c0 * 16 + c1 * 4 + c2 (little-endian words)
  uint32_t w[16];
};
struct FsArgs {
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  size_t k0, n;        // targets [k0, k0 + gridDim.x) of n
  uint32_t max_len;    // codes of a target past it are not read
  const uint2* qtab;   // per query {offset into query, length}
  const int8_t* mat;   // alpha x alpha, mat[q * alpha + a]
  const uint8_t* query;
  uint32_t q0, alpha;  // queries q0 + blockIdx.y
  int32_t o, e, fs;    // open + extend, extend, frameshift (all <= 0)
  int32_t* scores;     // nq x n
  uint8_t* strands;    // nq x n or null
  FsTable table;
};

constexpr int FS_AMINO = 24;       // the profile's real columns (SW_PROTEIN_ALPHA)
constexpr int FS_OFF = 24;         // the column of a codon outside the target
constexpr uint32_t FS_X = 22;      // a codon holding N (or any code past it)
constexpr int32_t FS_PAD = -128;   // rows past the query, codons outside the target
constexpr int32_t FS_NEG = -(1 << 29);
constexpr uint32_t FS_OFFW = FS_OFF | FS_OFF << 8 | FS_OFF << 16;

__device__ __forceinline__ int32_t fs_shr1(int32_t lane0_value, int32_t v) {  // wave_shr:1
  return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int32_t fs_max3(int32_t a, int32_t b, int32_t c) {
  return max(max(a, b), c);
}
__device__ __forceinline__ uint32_t fs_comp(uint32_t c) { return c < 4 ? c ^ 2u : c; }

// The amino acids of codon index j of a strand of L codes, packed f at bits 8f: FS_OFF for a
// frame whose codon runs past the strand.
__device__ __forceinline__ uint32_t fs_aminos(const uint8_t* tab, const uint8_t* p, uint32_t L,
                                              uint32_t j, bool reverse) {
  const uint64_t s = 3ull * j;
  uint32_t c[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const bool in_t = s + i < L;
    const uint64_t at = reverse ? (uint64_t)L - 1 - (s + i) : s + i;
    const uint32_t v = in_t ? p[in_t ? at : 0] : 4u;
    c[i] = reverse ? fs_comp(v) : v;
  }
  uint32_t w = 0;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const bool ok = (c[f] | c[f + 1] | c[f + 2]) < 4;  // all three are T, C, A or G
    uint32_t a = tab[ok ? c[f] * 16 + c[f + 1] * 4 + c[f + 2] : 0];
    a = ok ? a : FS_X;
    a = s + f + 2 < L ? a : (uint32_t)FS_OFF;
    w |= a << (8 * f);
  }
  return w;
}

template <int K>
__global__ void __launch_bounds__(128) fshift_score(const FsArgs a) {
  constexpr int ROWS = 64 * K;
  // prof[c][row]: the score of query row `row` against amino acid c, FS_PAD past the query
  __shared__ __attribute__((aligned(16))) int8_t prof[(FS_AMINO + 1) * ROWS];
  __shared__ uint32_t tabw[16];
  __shared__ int32_t sbest[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const bool reverse = tid >= 64;
  const uint32_t qi = a.q0 + blockIdx.y;
  const uint2 qe = a.qtab[qi];
  const uint32_t m = __builtin_amdgcn_readfirstlane(min(qe.y, (uint32_t)ROWS));
  const uint8_t* qc = a.query + qe.x;
  if (tid < 16) tabw[tid] = a.table.w[tid];
  for (uint32_t row = tid; row < (uint32_t)ROWS; row += 128) {
    const bool in_q = row < m;
    const uint32_t q = in_q ? qc[row] : 0u;
    const int8_t* mr = a.mat + (q < a.alpha ? q : 0u) * a.alpha;
#pragma unroll
    for (int c = 0; c < FS_AMINO; ++c)
      prof[c * ROWS + row] = in_q && (uint32_t)c < a.alpha ? mr[c] : (int8_t)FS_PAD;
    prof[FS_OFF * ROWS + row] = (int8_t)FS_PAD;
  }
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);

  const size_t k = a.k0 + blockIdx.x;  // (< n: the grid's x extent is the slice)
  const uint32_t L = __builtin_amdgcn_readfirstlane(min(a.lens[k], a.max_len));
  const uint8_t* tp = a.res + (L ? a.offs[k] : 0);
  const uint32_t J = L / 3;                       // codon indices
  const uint32_t nl = (m + K - 1) / K;            // lanes that hold query rows
  const uint32_t steps = J && nl ? J + nl - 1 : 0u;
  const int32_t o = a.o, e = a.e, fs = a.fs;

  int32_t h0[K], h1[K], h2[K], g2[K], e0[K], e1[K], e2[K];
#pragma unroll
  for (int r = 0; r < K; ++r) {
    h0[r] = h1[r] = h2[r] = g2[r] = 0;
    e0[r] = e1[r] = e2[r] = FS_NEG;
  }
  // the row above this lane's first: H and F of the three frames at this step's codon index (un,
  // uf), H at the index before it (ud), H of frame 2 two indices back (udd2)
  int32_t un0 = 0, un1 = 0, un2 = 0, uf0 = FS_NEG, uf1 = FS_NEG, uf2 = FS_NEG;
  int32_t ud0 = 0, ud1 = 0, ud2 = 0, udd2 = 0;
  int32_t best = 0;
  uint32_t aw = FS_OFFW;  // this lane's three amino acids
  const int8_t* myprof = prof + lane * K;

  for (uint32_t t0 = 0; t0 < steps; t0 += 64) {
    const uint32_t jn = t0 + lane;
    const uint32_t nxt = jn < J ? fs_aminos(tab, tp, L, jn, reverse) : FS_OFFW;
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
      // running down the rows: the row above at this index (n, f) and its state before this
      // step (d: H at j - 1, dd2: H of frame 2 at j - 2)
      int32_t n0 = un0, n1 = un1, n2 = un2, f0 = uf0, f1 = uf1, f2 = uf2;
      int32_t d0 = ud0, d1 = ud1, d2 = ud2, dd2 = udd2;
#pragma unroll
      for (int r = 0; r < K; ++r) {
        const int32_t s0 = (int32_t)(int8_t)(w0[r / 4] >> (8 * (r % 4)));
        const int32_t s1 = (int32_t)(int8_t)(w1[r / 4] >> (8 * (r % 4)));
        const int32_t s2 = (int32_t)(int8_t)(w2[r / 4] >> (8 * (r % 4)));
        // frame 0: p - 3 frame 0 at j - 1, p - 2 frame 1 at j - 1, p - 4 frame 2 at j - 2
        const int32_t m0 = s0 + fs_max3(0, d0, max(d1, dd2) + fs);
        const int32_t E0 = max(h0[r] + o, e0[r] + e);
        const int32_t F0 = max(n0 + o, f0 + e);
        const int32_t H0 = max(fs_max3(0, m0, E0), F0);
        // frame 1: p - 3 frame 1 at j - 1, p - 2 frame 2 at j - 1, p - 4 frame 0 at j - 1
        const int32_t m1 = s1 + fs_max3(0, d1, max(d2, d0) + fs);
        const int32_t E1 = max(h1[r] + o, e1[r] + e);
        const int32_t F1 = max(n1 + o, f1 + e);
        const int32_t H1 = max(fs_max3(0, m1, E1), F1);
        // frame 2: p - 3 frame 2 at j - 1, p - 2 frame 0 at j (the row above, this step),
        // p - 4 frame 1 at j - 1
        const int32_t m2 = s2 + fs_max3(0, d2, max(n0, d1) + fs);
        const int32_t E2 = max(h2[r] + o, e2[r] + e);
        const int32_t F2 = max(n2 + o, f2 + e);
        const int32_t H2 = max(fs_max3(0, m2, E2), F2);
        best = max(fs_max3(best, H0, H1), H2);
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
      // the bottom row goes one lane down; above lane 0 lies the matrix's edge
      udd2 = ud2;
      ud0 = un0;
      ud1 = un1;
      ud2 = un2;
      un0 = fs_shr1(0, n0);
      un1 = fs_shr1(0, n1);
      un2 = fs_shr1(0, n2);
      uf0 = fs_shr1(FS_NEG, f0);
      uf1 = fs_shr1(FS_NEG, f1);
      uf2 = fs_shr1(FS_NEG, f2);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d, 64));
  if (lane == 0) sbest[reverse ? 1 : 0] = best;
  __syncthreads();
  if (tid == 0) {
    const size_t at = (size_t)qi * a.n + k;
    const int32_t fw = sbest[0], rv = sbest[1];
    a.scores[at] = max(fw, rv);
    if (a.strands) a.strands[at] = rv > fw ? 1 : 0;
  }
}

template <int K>
static hipError_t fs_launch(FsArgs a, size_t n, size_t nq, hipStream_t st) {
  const size_t XS = (size_t)1 << 24, YS = 65535;  // targets and queries of a launch
  for (size_t q0 = 0; q0 < nq; q0 += YS)
    for (size_t k0 = 0; k0 < n; k0 += XS) {
      a.k0 = k0;
      a.q0 = (uint32_t)q0;
      hipLaunchKernelGGL(fshift_score<K>,
                         dim3((unsigned)std::min(XS, n - k0), (unsigned)std::min(YS, nq - q0)),
                         dim3(128), 0, st, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}
}  // namespace swk

// Rows per lane for queries of at most qlen rows: 4, 8 or 16 (SW_FSHIFT_MAX_QUERY = 64 x 16).
extern "C" int swk_fshift_rows(uint32_t qlen) { return qlen <= 256 ? 4 : qlen <= 512 ? 8 : 16; }

// qtab / mat / query: the alignment unit's table (qtab::build_align) of nq queries of at most
// qlen <= 1024 rows each; table: 64 protein codes (host); o, e, fs <= 0.  scores / strands
// (optional): nq x n.
extern "C" hipError_t swk_fshift_score(const uint8_t* res, const uint64_t* offs,
                                       const uint32_t* lens, size_t n, uint32_t max_len,
                                       const uint2* qtab, const int8_t* mat, const uint8_t* query,
                                       size_t nq, uint32_t qlen, uint32_t alpha,
                                       const uint8_t* table, int32_t o, int32_t e, int32_t fs,
                                       int32_t* scores, uint8_t* strands, hipStream_t st) {
  using namespace swk;
  if (!res || !offs || !lens || !qtab || !mat || !query || !table || !scores || n == 0 ||
      nq == 0 || nq > 0xFFFFFFFFull || qlen == 0 || qlen > 1024 || alpha == 0 ||
      alpha > (uint32_t)FS_AMINO || o > 0 || e > 0 || fs > 0 || o < -65534 || e < -32767 ||
      fs < -32767)
    return hipErrorInvalidValue;
  FsArgs a{};
  a.res = res;
  a.offs = offs;
  a.lens = lens;
  a.n = n;
  a.max_len = max_len;
  a.qtab = qtab;
  a.mat = mat;
  a.query = query;
  a.alpha = alpha;
  a.o = o;
  a.e = e;
  a.fs = fs;
  a.scores = scores;
  a.strands = strands;
  for (int i = 0; i < 16; ++i)  // (little-endian words: byte i of the table is byte i of LDS)
    a.table.w[i] = (uint32_t)table[4 * i] | (uint32_t)table[4 * i + 1] << 8 |
                   (uint32_t)table[4 * i + 2] << 16 | (uint32_t)table[4 * i + 3] << 24;
  switch (swk_fshift_rows(qlen)) {
    case 4: return fs_launch<4>(a, n, nq, st);
    case 8: return fs_launch<8>(a, n, nq, st);
    default: return fs_launch<16>(a, n, nq, st);
  }
}
