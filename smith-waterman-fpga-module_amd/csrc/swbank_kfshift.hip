// swbank_kfshift.hip — the score kernel of the frameshift-tolerant translated search
// (include/swbank.h "frameshift-tolerant translated search").
//
// A workgroup is two waves and owns one (query, target) pair: wave 0 scores the forward strand,
// wave 1 the reverse strand, read from the target's far end and complemented; the two meet once,
// at the end, to merge their scores.  Nothing waits across workgroups, so the hardware deals
// targets of any mix of lengths over the chip (a 70,000-nt target holds one workgroup, the short
// ones pass it by).  Each wave walks all rows of the query over all codons of its strand with the
// walk of swbank_kfswalk.h and keeps only the highest H.
#include "swbank.h"
#include "swbank_kcommon.h"
#include "swbank_kfswalk.h"

namespace swk {
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
    const uint32_t a = fs_codon(tab, c[f], c[f + 1], c[f + 2]);
    w |= (s + f + 2 < L ? a : FS_OFF) << (8 * f);
  }
  return w;
}

template <int K>
__global__ void __launch_bounds__(128) fshift_score(const FsArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[(FS_AMINO + 1) * ROWS];
  __shared__ uint32_t tabw[16];
  __shared__ int32_t sbest[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const bool reverse = tid >= 64;
  const uint32_t qi = a.q0 + blockIdx.y;
  const uint2 qe = a.qtab[qi];
  const uint32_t m = __builtin_amdgcn_readfirstlane(min(qe.y, (uint32_t)ROWS));
  if (tid < 16) tabw[tid] = a.table.w[tid];
  fs_profile<K>(a.mat, a.alpha, prof, a.query + qe.x, 1, m, 128);
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);

  const size_t k = a.k0 + blockIdx.x;  // (< n: the grid's x extent is the slice)
  const uint32_t L = __builtin_amdgcn_readfirstlane(min(a.lens[k], a.max_len));
  const uint8_t* tp = a.res + (L ? a.offs[k] : 0);
  const auto aminos = [&](uint32_t j) { return fs_aminos(tab, tp, L, j, reverse); };
  int32_t best = fs_walk<K, FsMode::Score>(prof, aminos, L / 3, m, a.o, a.e, a.fs, nullptr);
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

extern "C" int swk_fshift_rows(uint32_t qlen) { return swk::fs_rows(qlen); }

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
      alpha > (uint32_t)FS_AMINO || !fs_penalties_ok(o, e, fs))
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
  a.table = fs_table(table);
  switch (fs_rows(qlen)) {
    case 4: return fs_launch<4>(a, n, nq, st);
    case 8: return fs_launch<8>(a, n, nq, st);
    default: return fs_launch<16>(a, n, nq, st);
  }
}
