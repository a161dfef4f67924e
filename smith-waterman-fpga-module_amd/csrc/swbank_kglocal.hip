// swbank_kglocal.hip — the score kernel of the global-local search (include/swbank.h
// "global-local search").
//
// A workgroup is two waves that share one query's profile in LDS.  With both_strands it owns one
// (query, target) pair, as the frameshift search's does: wave 0 scores the forward strand, wave 1
// the reverse strand, read from the target's far end and complemented; the two meet once, at the
// end, to merge their results.  Without both_strands wave 1 scores the forward strand of the
// NEXT target: the workgroup owns (query, targets 2b and 2b + 1), each wave stores its own
// result, and the profile (5 to 24 KiB of LDS stores for 1,024 rows) is built once for two pairs.
// An idle wave 1 would leave a SIMD with at most 1.5 walking waves at 16 rows per lane, where LDS
// admits six workgroups per CU.  Nothing waits across workgroups.  Every result is an ordinary
// vector store by a wave's first lane.
#include "swbank.h"
#include "swbank_kcommon.h"
#include "swbank_kglwalk.h"

namespace swk {
struct GlArgs {
  const uint8_t* res;
  const uint64_t* offs;
  const uint32_t* lens;
  size_t k0, k1, n;    // targets [k0, k1) of n: one per workgroup, or two without `both`
  uint32_t max_len;    // codes of a target past it are not read
  const uint2* qtab;   // per query {offset into query, length}
  const int8_t* mat;   // alpha x alpha, mat[q * alpha + t]
  const uint8_t* query;
  uint32_t q0, alpha;  // queries q0 + blockIdx.y
  int32_t o, e;        // open + extend, extend (both <= 0)
  uint32_t both;       // wave 1 walks the reverse strand (DNA codes)
  int32_t* scores;     // nq x n
  uint32_t* ends;      // nq x n or null
  uint8_t* strands;    // nq x n or null
};

template <int K, int ENDS>
__global__ void __launch_bounds__(128) glocal_score(const GlArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[GL_MAX_ALPHA * ROWS];
  __shared__ int32_t sbest[2];
  __shared__ uint32_t spos[2];
  const uint32_t tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool reverse = a.both && wave;
  const uint32_t qi = a.q0 + blockIdx.y;
  const uint2 qe = a.qtab[qi];
  const uint32_t m = __builtin_amdgcn_readfirstlane(min(qe.y, (uint32_t)ROWS));
  gl_profile<K>(a.mat, a.alpha, prof, a.query + qe.x, m, 128);
  __syncthreads();

  // (k < k1 <= n for wave 0: the grid's x extent is the slice's workgroups)
  const size_t k = a.both ? a.k0 + blockIdx.x : a.k0 + 2 * (size_t)blockIdx.x + wave;
  const bool have = m && k < a.k1;
  const uint32_t L = have ? __builtin_amdgcn_readfirstlane(min(a.lens[k], a.max_len)) : 0u;
  const uint8_t* tp = a.res + (L ? a.offs[k] : 0);
  const uint32_t last = a.alpha - 1;  // a code past the alphabet reads as its last code
  const size_t at = (size_t)qi * a.n + k;
  if (have) {
    const auto code = [&](uint32_t j) {
      uint32_t c = tp[reverse ? L - 1 - j : j];
      c = reverse && c < 4 ? c ^ 2u : c;
      return min(c, last);
    };
    const GlBest b = gl_walk<K, ENDS>(prof, code, L, m, a.o, a.e);
    if ((tid & 63) == 0) {
      if (a.both) {
        sbest[wave] = b.v;
        spos[wave] = b.pos;
      } else {
        a.scores[at] = b.v;
        if (a.ends) a.ends[at] = b.pos - 1;  // (index + 1; 0 - 1 = SW_END_NONE)
        if (a.strands) a.strands[at] = 0;
      }
    }
  }
  __syncthreads();
  if (tid == 0 && have && a.both) {
    const bool rv = sbest[1] > sbest[0];
    uint32_t pos = spos[rv ? 1 : 0];  // index + 1; 0: the boundary
    if (ENDS == GL_QUERY && rv && pos) pos = L + 1 - pos;  // on the forward target: L - 1 - j
    a.scores[at] = sbest[rv ? 1 : 0];
    if (a.ends) a.ends[at] = pos - 1;  // (0 - 1 = SW_END_NONE)
    if (a.strands) a.strands[at] = rv ? 1 : 0;
  }
}

template <int K, int ENDS>
static hipError_t gl_launch(GlArgs a, size_t n, size_t nq, hipStream_t st) {
  const size_t XS = (size_t)1 << 24, YS = 65535;  // targets and queries of a launch
  for (size_t q0 = 0; q0 < nq; q0 += YS)
    for (size_t k0 = 0; k0 < n; k0 += XS) {
      const size_t cnt = std::min(XS, n - k0);
      a.k0 = k0;
      a.k1 = k0 + cnt;
      a.q0 = (uint32_t)q0;
      hipLaunchKernelGGL((glocal_score<K, ENDS>),
                         dim3((unsigned)(a.both ? cnt : (cnt + 1) / 2),
                              (unsigned)std::min(YS, nq - q0)),
                         dim3(128), 0, st, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

template <int ENDS>
static hipError_t gl_rows_launch(const GlArgs& a, uint32_t qlen, size_t n, size_t nq,
                                 hipStream_t st) {
  switch (gl_rows(qlen)) {
    case 4: return gl_launch<4, ENDS>(a, n, nq, st);
    case 8: return gl_launch<8, ENDS>(a, n, nq, st);
    default: return gl_launch<16, ENDS>(a, n, nq, st);
  }
}
}  // namespace swk

extern "C" int swk_glocal_rows(uint32_t qlen) { return swk::gl_rows(qlen); }

// qtab / mat / query: the alignment unit's table (qtab::build_align) of nq queries of 1 to
// qlen <= 1024 rows each; o, e <= 0, inside the entry's range rule for max_len; ends: SW_ENDS_*;
// both: DNA codes only.  scores, ends_out / strands (optional): nq x n.
extern "C" hipError_t swk_glocal_score(const uint8_t* res, const uint64_t* offs,
                                       const uint32_t* lens, size_t n, uint32_t max_len,
                                       const uint2* qtab, const int8_t* mat, const uint8_t* query,
                                       size_t nq, uint32_t qlen, uint32_t alpha, int32_t o,
                                       int32_t e, int32_t ends, int32_t both, int32_t* scores,
                                       uint32_t* ends_out, uint8_t* strands, hipStream_t st) {
  using namespace swk;
  if (!res || !offs || !lens || !qtab || !mat || !query || !scores || n == 0 || nq == 0 ||
      nq > 0xFFFFFFFFull || qlen == 0 || qlen > 1024 || alpha == 0 ||
      alpha > (uint32_t)GL_MAX_ALPHA || o > 0 || e > 0 || o < -65534 || e < -32767 ||
      ends < GL_QUERY || ends > GL_BOTH)
    return hipErrorInvalidValue;
  GlArgs a{};
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
  a.both = both ? 1u : 0u;
  a.scores = scores;
  a.ends = ends_out;
  a.strands = strands;
  switch (ends) {
    case GL_QUERY: return gl_rows_launch<GL_QUERY>(a, qlen, n, nq, st);
    case GL_TARGET: return gl_rows_launch<GL_TARGET>(a, qlen, n, nq, st);
    default: return gl_rows_launch<GL_BOTH>(a, qlen, n, nq, st);
  }
}
