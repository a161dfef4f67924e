// swbank_kframe.hip — the kernels of the translated search (include/swbank.h "translated
// search"): the six-frame translation of a ragged DNA batch, the merge of the
// six frames' score rows, and, for the alignment of chosen hits, the translation of each hit's
// frame and the rewrite of its record into nucleotide coordinates.  All are small beside the
// scoring pass they surround and are kept plain; inside a launch no workgroup waits for another.
#include "swbank.h"
#include "swbank_kcommon.h"

namespace swk {
// The 64 amino acids of a genetic code, indexed c0 * 16 + c1 * 4 + c2, as kernel arguments; a
// workgroup copies them to LDS once.
struct CodonTable {
  uint32_t w[16];
};
constexpr uint8_t FR_X = 22;  // a codon holding N (or any code past it)

__device__ __forceinline__ void fr_table_to_lds(uint32_t* tabw, const CodonTable& t) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) tabw[i] = t.w[i];
  }
  __syncthreads();
}

__device__ __forceinline__ uint8_t fr_comp(uint8_t c) { return c < 4 ? (uint8_t)(c ^ 2) : c; }

__device__ __forceinline__ uint8_t fr_amino(const uint8_t* tab, uint32_t c0, uint32_t c1,
                                            uint32_t c2) {
  const bool ok = (c0 | c1 | c2) < 4;  // all three are T, C, A or G
  const uint8_t a = tab[ok ? c0 * 16 + c1 * 4 + c2 : 0];
  return ok ? a : FR_X;
}

// Codons of frame f % 3 = o of a target of len codes, at most cap.
__device__ __forceinline__ uint32_t fr_codons(uint32_t len, uint32_t o, uint32_t cap) {
  return len >= o + 3 ? min((len - o) / 3, cap) : 0u;
}

__device__ __forceinline__ uint32_t fr_lane_u32(uint32_t v, int t) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, t);
}
__device__ __forceinline__ unsigned long long fr_lane_u64(unsigned long long v, int t) {
  return ((unsigned long long)fr_lane_u32((uint32_t)(v >> 32), t) << 32) |
         fr_lane_u32((uint32_t)v, t);
}

// ---- the translation of a batch ----------------------------------------------------------------
// A workgroup is one wave and owns 64 adjacent targets (revcomp_batch's shape, swbank_kstrand.hip):
// the lanes read the 64 offsets and lengths together and write the 6 x 64 offsets and lengths of
// the translations, then the wave walks the targets, lane l on codon c + l of one target.  Codon j
// of the three forward frames lies in codes 3j .. 3j + 4, and of the three reverse frames in the
// same five codes counted from the far end, complemented: ten loads give six amino acids, a
// group's loads before its stores.  One path serves every length: the wave runs until its longest
// target is done.  blockIdx.y deals the 64-codon steps of those targets over gridDim.y waves (long
// targets in a small batch would otherwise leave most of the chip idle: 12,500 targets are 196
// waves); the wave of blockIdx.y == 0 writes the offsets and lengths.  Translated target
// f * n + k goes to out + (f * n + k) * stride; cap bounds a translation's length (the host's
// max_len / 3, so a length past max_len cannot leave its slot).
constexpr int FR_GROUP = 4;  // targets whose loads are in flight together

__global__ void __launch_bounds__(64) translate_batch(const uint8_t* __restrict__ in,
                                                      const uint64_t* __restrict__ offs,
                                                      const uint32_t* __restrict__ lens, size_t n,
                                                      const CodonTable table,
                                                      uint8_t* __restrict__ out, size_t stride,
                                                      uint32_t cap, uint64_t* __restrict__ out_offs,
                                                      uint32_t* __restrict__ out_lens) {
  __shared__ uint32_t tabw[16];
  fr_table_to_lds(tabw, table);
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  const int lane = threadIdx.x;
  const size_t kbase = (size_t)blockIdx.x * 64, k = kbase + lane;
  const bool have = k < n;
  const unsigned long long off = have ? offs[k] : 0ull;
  const uint32_t len = have ? lens[k] : 0u;
  if (have && blockIdx.y == 0) {
#pragma unroll
    for (int f = 0; f < SW_FRAME_COUNT; ++f) {
      const size_t slot = (size_t)f * n + k;
      out_offs[slot] = (uint64_t)slot * stride;
      out_lens[slot] = fr_codons(len, f % 3, cap);
    }
  }
  const uint32_t step = 64u * gridDim.y;
  for (uint32_t c = 64u * blockIdx.y;; c += step) {
    // (frame 0 has the most codons)
    const unsigned long long live = __ballot(fr_codons(len, 0, cap) > c);
    if (!live) break;
    const uint32_t j = c + lane;
    const unsigned long long s = 3ull * j;  // the codon's first code in frame 0
    for (int t0 = 0; t0 < 64; t0 += FR_GROUP) {
      if (!((live >> t0) & ((1ull << FR_GROUP) - 1))) continue;
      uint8_t v[FR_GROUP][SW_FRAME_COUNT];
#pragma unroll
      for (int u = 0; u < FR_GROUP; ++u) {
        const uint32_t tl = fr_lane_u32(len, t0 + u);
        const uint8_t* p = in + fr_lane_u64(off, t0 + u);
        uint32_t fw[5], rv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const bool in_t = s + i < tl;
          fw[i] = in_t ? p[s + i] : 4u;
          rv[i] = in_t ? fr_comp(p[tl - 1 - (s + i)]) : 4u;
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) {
          v[u][o] = fr_amino(tab, fw[o], fw[o + 1], fw[o + 2]);
          v[u][3 + o] = fr_amino(tab, rv[o], rv[o + 1], rv[o + 2]);
        }
      }
#pragma unroll
      for (int u = 0; u < FR_GROUP; ++u) {
        const uint32_t tl = fr_lane_u32(len, t0 + u);  // (0 for a target past n)
        const size_t kk = kbase + t0 + u;
#pragma unroll
        for (int o = 0; o < 3; ++o) {
          if (j < fr_codons(tl, o, cap)) {
            out[((size_t)o * n + kk) * stride + j] = v[u][o];
            out[((size_t)(3 + o) * n + kk) * stride + j] = v[u][3 + o];
          }
        }
      }
    }
    if (c > 0xFFFFFFFFu - step) break;
  }
}

// ---- the frame merge -----------------------------------------------------------------------------
// sl: nq rows of 6 * nk scores, frame-major, the slice [k0, k0 + nk) of the targets; out / frames:
// nq rows of n.  blockIdx.y is the row.  A tie is the lowest frame.
constexpr int FR_MERGE_BLOCK = 256;

__global__ void __launch_bounds__(FR_MERGE_BLOCK) frame_merge(int32_t* __restrict__ out,
                                                              const int32_t* __restrict__ sl,
                                                              uint8_t* __restrict__ frames, size_t n,
                                                              size_t k0, size_t nk, size_t row0) {
  const size_t k = (size_t)blockIdx.x * FR_MERGE_BLOCK + threadIdx.x;
  if (k >= nk) return;
  const size_t row = row0 + blockIdx.y, at = row * n + k0 + k;
  const int32_t* s = sl + row * SW_FRAME_COUNT * nk + k;
  int32_t best = s[0];
  uint8_t bf = 0;
#pragma unroll
  for (int f = 1; f < SW_FRAME_COUNT; ++f) {
    const int32_t x = s[(size_t)f * nk];
    if (x > best) {
      best = x;
      bf = (uint8_t)f;
    }
  }
  out[at] = best;
  if (frames) frames[at] = bf;
}

// ---- the hits of an alignment call ----------------------------------------------------------------
// The pair list of sw_align_set_hits (swbank_align.h): hit h is query hit_queries[h], or
// h / hits_per_query, against target hits[h], or h; a query >= nq or a target >= n names no pair.
struct FramePairs {
  const uint32_t* hit_queries;
  uint32_t hits_per_query;
  const uint64_t* hits;
  size_t n_hits;
  const uint8_t* frames;  // nq x n
  size_t n;
  uint32_t nq;
};

__device__ __forceinline__ bool fr_pair(const FramePairs& a, size_t h, uint32_t& q, uint64_t& t,
                                        uint32_t& f) {
  q = a.hit_queries ? a.hit_queries[h] : (uint32_t)(h / a.hits_per_query);
  t = a.hits ? a.hits[h] : (uint64_t)h;
  if (q >= a.nq || t >= a.n) return false;
  f = a.frames[(size_t)q * a.n + t];
  return true;
}

// One workgroup (a wave) per hit: the translation of the hit's frame to out + h * stride, that
// offset, its length and the hit's query to out_offs / out_lens / out_q [h].  A slot that names
// no pair gets length 0 and the query SW_QUERY_NONE; a frame above 5 length 0.
__global__ void __launch_bounds__(64) translate_hits(const uint8_t* __restrict__ in,
                                                     const uint64_t* __restrict__ offs,
                                                     const uint32_t* __restrict__ lens,
                                                     const FramePairs a, const CodonTable table,
                                                     uint8_t* __restrict__ out, size_t stride,
                                                     uint32_t cap, uint64_t* __restrict__ out_offs,
                                                     uint32_t* __restrict__ out_lens,
                                                     uint32_t* __restrict__ out_q) {
  __shared__ uint32_t tabw[16];
  fr_table_to_lds(tabw, table);
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  const size_t h = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  uint32_t q = 0, f = 0;
  uint64_t t = 0;
  const bool pair = fr_pair(a, h, q, t, f);
  const uint32_t L = pair && f < SW_FRAME_COUNT ? lens[t] : 0u, o = f % 3;
  const uint32_t nc = fr_codons(L, o, cap);
  if (lane == 0) {
    out_offs[h] = (uint64_t)h * stride;
    out_lens[h] = nc;
    out_q[h] = pair ? q : SW_QUERY_NONE;
  }
  if (nc == 0) return;
  const uint8_t* p = in + offs[t];
  uint8_t* dst = out + h * stride;
  for (uint32_t j = lane; j < nc; j += 64) {
    const uint32_t s = o + 3 * j;  // (s + 2 < L)
    dst[j] = f < 3 ? fr_amino(tab, p[s], p[s + 1], p[s + 2])
                   : fr_amino(tab, fr_comp(p[L - 1 - s]), fr_comp(p[L - 2 - s]),
                              fr_comp(p[L - 3 - s]));
  }
}

// After the alignment of the translated hits (target h of that call is hit h): the records name
// the DNA target, carry the frame in their flags and give nucleotide coordinates on the forward
// target.
__global__ void __launch_bounds__(256) frame_fixup(sw_alignment* __restrict__ out,
                                                   const uint32_t* __restrict__ lens,
                                                   const uint64_t* __restrict__ ids,
                                                   const FramePairs a) {
  const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= a.n_hits) return;
  sw_alignment& r = out[h];
  if (r.flags & (uint32_t)SW_ALIGN_NO_HIT) return;
  uint32_t q = 0, f = 0;
  uint64_t t = 0;
  if (!fr_pair(a, h, q, t, f)) return;
  r.index = t;
  r.id = ids ? ids[t] : t;
  if (f >= SW_FRAME_COUNT) return;  // (an empty pair without a frame)
  const uint32_t o = f % 3;
  r.flags |= (o << SW_ALIGN_FRAME_SHIFT) | (f >= 3 ? (uint32_t)SW_ALIGN_REVERSE : 0u);
  if (r.score <= 0) return;
  const uint32_t L = lens[t], fs = o + 3 * r.t_start, fe = o + 3 * r.t_end + 2;
  r.t_start = f < 3 ? fs : L - 1 - fe;
  r.t_end = f < 3 ? fe : L - 1 - fs;
}

static CodonTable codon_table(const uint8_t* table) {
  CodonTable t;
  for (int i = 0; i < 16; ++i)  // (little-endian words: byte i of the table is byte i of LDS)
    t.w[i] = (uint32_t)table[4 * i] | (uint32_t)table[4 * i + 1] << 8 |
             (uint32_t)table[4 * i + 2] << 16 | (uint32_t)table[4 * i + 3] << 24;
  return t;
}
static FramePairs frame_pairs(const uint8_t* frames, const uint32_t* hit_queries,
                              size_t hits_per_query, const uint64_t* hits, size_t n_hits, size_t n,
                              size_t nq) {
  return FramePairs{hit_queries, (uint32_t)hits_per_query, hits, n_hits, frames, n, (uint32_t)nq};
}
static bool frame_pairs_ok(const uint8_t* frames, const uint32_t* hit_queries,
                           size_t hits_per_query, size_t n_hits, size_t n, size_t nq) {
  return frames && n_hits && n_hits <= 0xFFFFFFFFull && n && nq && nq <= 0xFFFFFFFFull &&
         (hit_queries != nullptr) != (hits_per_query != 0) && hits_per_query <= 0xFFFFFFFFull;
}
}  // namespace swk

// table: 64 protein codes (host).  6n < 2^32; cap <= stride.
extern "C" hipError_t swk_translate_batch(const uint8_t* in, const uint64_t* offs,
                                          const uint32_t* lens, size_t n, const uint8_t* table,
                                          uint8_t* out, size_t stride, uint32_t cap,
                                          uint64_t* out_offs, uint32_t* out_lens, hipStream_t st) {
  if (!in || !offs || !lens || !table || !out || !out_offs || !out_lens || n == 0 ||
      n >= 0x100000000ull / SW_FRAME_COUNT || cap > stride)
    return hipErrorInvalidValue;
  // (cap says how many 64-codon steps the longest target can have)
  const unsigned ysteps =
      (unsigned)std::min<uint64_t>(std::max<uint64_t>(((uint64_t)cap + 63) / 64, 1), 64);
  hipLaunchKernelGGL(swk::translate_batch, dim3((unsigned)((n + 63) / 64), ysteps), dim3(64), 0, st,
                     in, offs, lens, n, swk::codon_table(table), out, stride, cap, out_offs, out_lens);
  return hipGetLastError();
}

extern "C" hipError_t swk_frame_merge(int32_t* out, const int32_t* slice, uint8_t* frames, size_t n,
                                      size_t k0, size_t nk, size_t nq, hipStream_t st) {
  using namespace swk;
  if (!out || !slice || nk == 0 || nq == 0 || k0 > n || nk > n - k0 || n > 0x100000000ull)
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((nk + FR_MERGE_BLOCK - 1) / FR_MERGE_BLOCK);
  const size_t ROWS = 65535;  // rows of a launch (the grid's y extent)
  for (size_t r0 = 0; r0 < nq; r0 += ROWS) {
    hipLaunchKernelGGL(frame_merge, dim3(blocks, (unsigned)std::min(ROWS, nq - r0)),
                       dim3(FR_MERGE_BLOCK), 0, st, out, slice, frames, n, k0, nk, r0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" hipError_t swk_translate_hits(const uint8_t* in, const uint64_t* offs,
                                         const uint32_t* lens, size_t n, size_t nq,
                                         const uint8_t* frames, const uint32_t* hit_queries,
                                         size_t hits_per_query, const uint64_t* hits,
                                         size_t n_hits, const uint8_t* table, uint8_t* out,
                                         size_t stride, uint32_t cap, uint64_t* out_offs,
                                         uint32_t* out_lens, uint32_t* out_q, hipStream_t st) {
  if (!in || !offs || !lens || !table || !out || !out_offs || !out_lens || !out_q ||
      cap > stride || !swk::frame_pairs_ok(frames, hit_queries, hits_per_query, n_hits, n, nq))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(swk::translate_hits, dim3((unsigned)n_hits), dim3(64), 0, st, in, offs, lens,
                     swk::frame_pairs(frames, hit_queries, hits_per_query, hits, n_hits, n, nq),
                     swk::codon_table(table), out, stride, cap, out_offs, out_lens, out_q);
  return hipGetLastError();
}

extern "C" hipError_t swk_frame_fixup(sw_alignment* out, const uint32_t* lens, const uint64_t* ids,
                                      size_t n, size_t nq, const uint8_t* frames,
                                      const uint32_t* hit_queries, size_t hits_per_query,
                                      const uint64_t* hits, size_t n_hits, hipStream_t st) {
  if (!out || !lens || !swk::frame_pairs_ok(frames, hit_queries, hits_per_query, n_hits, n, nq))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(swk::frame_fixup, dim3((unsigned)((n_hits + 255) / 256)), dim3(256), 0, st,
                     out, lens, ids,
                     swk::frame_pairs(frames, hit_queries, hits_per_query, hits, n_hits, n, nq));
  return hipGetLastError();
}
