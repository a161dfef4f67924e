// swbank_kstat.hip — the kernels of the hit statistics (include/swbank.h "hit significance",
// DESIGN.md §3.12): the seeded shuffle of a batch, the score / length histogram of a score
// matrix, and bits and E-values of a hit list.  All three are small beside the scoring pass they
// surround and are kept plain; inside a launch no workgroup waits for another.
#include "swbank.h"
#include "swbank_kcommon.h"

namespace swk {
// ---- the shuffle ----------------------------------------------------------------------------
// The Fisher-Yates chain of a target is sequential (step j swaps with a position drawn from
// [0, j]), the draws are counter-based.  Targets go three ways by their length:
//   lane tier   shuffle_batch: a workgroup is one wave and owns 64 adjacent targets.  A target of
//               at most `row` bytes (max_len, at most SHUF_LANE) is shuffled by its own lane in
//               that lane's LDS row (an odd number of dwords apart, so the lanes' bytes of one
//               index sit on different banks); the wave stages the rows and writes them out
//               together, 64 adjacent bytes of one target per access.
//   classes     shuffle_long: a workgroup (one wave) owns ONE longer target, staged whole in
//               dynamic LDS sized by the launch's class (SHUF_CLASS, not by max_len: a contig does
//               not set the occupancy of the reads beside it).  The 64 lanes compute 64 draws at a
//               time; what stays sequential is the swaps, two byte reads and two byte writes of
//               LDS per step, the index handed over by readlane.  One launch per class that
//               max_len reaches, a workgroup per target, those outside the class return at once.
//   global tier past the largest class that was launched, shuffle_batch's wave copies the target
//               to its place in `out` and lane 0 walks the chain there (one thread's loads and
//               stores of an address stay in order).
constexpr int SHUF_LANE = 260;
constexpr unsigned long long STAT_G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long stat_mix(unsigned long long z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// The chain of one target of len codes at p (LDS or global), by one thread.
__device__ __forceinline__ void shuffle_chain(uint8_t* p, uint32_t len, unsigned long long key) {
  unsigned long long c = key + STAT_G * len;  // key + G (j + 1) at j = len - 1
  for (uint32_t j = len - 1; j >= 1; --j, c -= STAT_G) {
    const uint32_t r = __umulhi((uint32_t)(stat_mix(c) >> 32), j + 1);
    const uint8_t a = p[j], b = p[r];
    p[j] = b;
    p[r] = a;
  }
}

// Lane t's value in every lane (t is wave-uniform).
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int t) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, t);
}
__device__ __forceinline__ unsigned long long lane_u64(unsigned long long v, int t) {
  return ((unsigned long long)lane_u32((uint32_t)(v >> 32), t) << 32) | lane_u32((uint32_t)v, t);
}

// Targets [0, n) of (in, offs, lens), keyed by their batch positions k0 + k.  out_offs == nullptr:
// target k goes to out + offs[k] (the caller's layout); else to out + k * stride, and that offset
// to out_offs[k] (the estimate's scratch, whose size the host knows without reading offsets).
// row: bytes of a lane's LDS row (a multiple of 4, <= SHUF_LANE; the launch gives 64 rows of
// dynamic LDS): the lane tier's limit.  The host sizes it from max_len, so a batch of short targets
// keeps more waves on a CU.  top: targets of more than row and at most top bytes are left to
// shuffle_long's launches (top == row: there are none), the longer ones walked in `out`.
constexpr int SHUF_GROUP = 8;  // targets whose loads are in flight together while staging

__global__ void __launch_bounds__(64) shuffle_batch(const uint8_t* __restrict__ in,
                                                    const uint64_t* __restrict__ offs,
                                                    const uint32_t* __restrict__ lens, size_t n,
                                                    uint64_t k0, uint64_t seed,
                                                    uint8_t* __restrict__ out, uint64_t* out_offs,
                                                    uint32_t stride, uint32_t row, uint32_t top) {
  extern __shared__ uint8_t lds[];  // 64 x row bytes
  const int lane = threadIdx.x;
  const size_t k = (size_t)blockIdx.x * 64 + lane;
  const bool have = k < n;
  const unsigned long long off = have ? offs[k] : 0ull;
  const uint32_t len = have ? lens[k] : 0u;
  const unsigned long long to = out_offs ? (unsigned long long)k * stride : off;
  if (have && out_offs) out_offs[k] = to;
  const unsigned long long key = stat_mix(seed + STAT_G * (k0 + k + 1));
  const uint32_t mine = len <= row ? len : 0u;  // codes in this lane's row
  // stage the rows: 64 adjacent bytes of one target per access, a group's loads before its stores
  for (uint32_t c = 0; c < row; c += 64) {
    if (!__ballot(mine > c)) break;
    const uint32_t i = c + lane;
    for (int t0 = 0; t0 < 64; t0 += SHUF_GROUP) {
      uint8_t v[SHUF_GROUP];
#pragma unroll
      for (int u = 0; u < SHUF_GROUP; ++u)
        v[u] = i < lane_u32(mine, t0 + u) ? in[lane_u64(off, t0 + u) + i] : (uint8_t)0;
#pragma unroll
      for (int u = 0; u < SHUF_GROUP; ++u)
        if (i < lane_u32(mine, t0 + u)) lds[(t0 + u) * row + i] = v[u];
    }
  }
  __syncthreads();
  if (mine > 1) shuffle_chain(lds + lane * row, mine, key);
  __syncthreads();
  for (uint32_t c = 0; c < row; c += 64) {
    if (!__ballot(mine > c)) break;
    const uint32_t i = c + lane;
    for (int t0 = 0; t0 < 64; t0 += SHUF_GROUP) {
      uint8_t v[SHUF_GROUP];
#pragma unroll
      for (int u = 0; u < SHUF_GROUP; ++u)
        v[u] = i < lane_u32(mine, t0 + u) ? lds[(t0 + u) * row + i] : (uint8_t)0;
#pragma unroll
      for (int u = 0; u < SHUF_GROUP; ++u)
        if (i < lane_u32(mine, t0 + u)) out[lane_u64(to, t0 + u) + i] = v[u];
    }
  }
  if (!__ballot(len > top)) return;
  for (int t = 0; t < 64; ++t) {  // (wave-uniform: every lane sees target t's length)
    const uint32_t tl = lane_u32(len, t);
    if (tl <= top) continue;
    const uint8_t* src = in + lane_u64(off, t);
    uint8_t* dst = out + lane_u64(to, t);
    const unsigned long long tkey = lane_u64(key, t);
    for (uint32_t i = lane; i < tl; i += 64) dst[i] = src[i];
    __threadfence();  // the wave's copy is visible to lane 0's loads
    __syncthreads();
    if (lane == 0) shuffle_chain(dst, tl, tkey);
  }
}

// The classes: a target of more than SHUF_CLASS[c - 1] (class 0: the lane tier's row) and at
// most SHUF_CLASS[c] bytes is shuffled in SHUF_CLASS[c] bytes of dynamic LDS.  4 KiB keeps a CU's
// 32 waves resident, 40 KiB four workgroups, the last class takes the CU's whole LDS.
constexpr int SHUF_CLASSES = 3;
constexpr uint32_t SHUF_CLASS[SHUF_CLASSES] = {4u << 10, 40u << 10, 160u << 10};
constexpr int SHUF_STAGE = 8;  // loads of a lane in flight together while staging

// Target kb + blockIdx.x of the slice, when lo < its length <= hi (the launch's dynamic LDS);
// k0, seed, out and stride (0: the caller's layout) as for shuffle_batch, which writes out_offs.
// One wave: the barriers only order its LDS accesses.
__global__ void __launch_bounds__(64) shuffle_long(const uint8_t* __restrict__ in,
                                                   const uint64_t* __restrict__ offs,
                                                   const uint32_t* __restrict__ lens, size_t kb,
                                                   uint64_t k0, uint64_t seed,
                                                   uint8_t* __restrict__ out, uint32_t stride,
                                                   uint32_t lo, uint32_t hi) {
  extern __shared__ uint8_t lds[];  // hi bytes
  const uint32_t lane = threadIdx.x;
  const size_t k = kb + blockIdx.x;
  const uint32_t len = __builtin_amdgcn_readfirstlane(lens[k]);
  if (len <= lo || len > hi) return;
  const unsigned long long off = offs[k];
  const uint8_t* src = in + off;
  uint8_t* dst = out + (stride ? (unsigned long long)k * stride : off);
  const unsigned long long key = stat_mix(seed + STAT_G * (k0 + k + 1));
  for (uint32_t c = 0; c < len; c += 64 * SHUF_STAGE) {
    uint8_t v[SHUF_STAGE];
#pragma unroll
    for (int u = 0; u < SHUF_STAGE; ++u) {
      const uint32_t i = c + u * 64 + lane;
      v[u] = i < len ? src[i] : (uint8_t)0;
    }
#pragma unroll
    for (int u = 0; u < SHUF_STAGE; ++u) {
      const uint32_t i = c + u * 64 + lane;
      if (i < len) lds[i] = v[u];
    }
  }
  __syncthreads();
  // steps j0, j0 - 1, ... down to 1, 64 at a time: lane t draws step j0 - t's position, then
  // the swaps run in order at wave-uniform addresses, stored by lane 0
  for (uint32_t j0 = len - 1; j0 >= 1; j0 = j0 > 64 ? j0 - 64 : 0) {
    const uint32_t j = j0 - lane;  // (steps below 1 are drawn and not taken)
    const unsigned long long h = stat_mix(key + STAT_G * ((unsigned long long)j + 1));
    const uint32_t r = __umulhi((uint32_t)(h >> 32), j + 1);
    const auto step = [&](int t) {  // (t is wave-uniform)
      const uint32_t jt = j0 - t, rt = lane_u32(r, t);
      const uint8_t a = lds[jt], b = lds[rt];
      if (lane == 0) {
        lds[jt] = b;
        lds[rt] = a;
      }
    };
    if (j0 >= 64) {
#pragma unroll
      for (int t = 0; t < 64; ++t) step(t);
    } else {
#pragma nounroll
      for (int t = 0; t < (int)j0; ++t) step(t);
    }
  }
  __syncthreads();
  for (uint32_t c = 0; c < len; c += 64 * SHUF_STAGE) {
    uint8_t v[SHUF_STAGE];
#pragma unroll
    for (int u = 0; u < SHUF_STAGE; ++u) {
      const uint32_t i = c + u * 64 + lane;
      v[u] = i < len ? lds[i] : (uint8_t)0;
    }
#pragma unroll
    for (int u = 0; u < SHUF_STAGE; ++u) {
      const uint32_t i = c + u * 64 + lane;
      if (i < len) dst[i] = v[u];
    }
  }
}

// ---- the score / length histogram ---------------------------------------------------------------
// top_hist's pattern (swbank_ktop.hip): a workgroup's histogram in LDS, then one global atomic
// per non-empty bin; blockIdx.y is the row.  A workgroup visits HIST_BLOCK * HIST_ITEMS = 4096
// targets, so its counts fit 32 bits; its length sums (4096 lengths below 2^32) do not and are
// 64-bit LDS atomics.
constexpr int HIST_BLOCK = 256, HIST_ITEMS = 16, HIST_BINS = SW_STAT_BINS;

__global__ void __launch_bounds__(HIST_BLOCK) stat_hist(const int32_t* scores,
                                                        const uint32_t* lens, size_t n,
                                                        size_t row0, unsigned long long* counts,
                                                        unsigned long long* len_sums,
                                                        unsigned long long* clamped) {
  __shared__ uint32_t hc[HIST_BINS];
  __shared__ unsigned long long hl[HIST_BINS];
  __shared__ uint32_t hclamp;
  const size_t row = row0 + blockIdx.y;
  const bool sums = lens && len_sums;
  for (uint32_t i = threadIdx.x; i < HIST_BINS; i += HIST_BLOCK) {
    hc[i] = 0;
    hl[i] = 0;
  }
  if (threadIdx.x == 0) hclamp = 0;
  __syncthreads();
  const int32_t* r = scores + row * n;
  uint32_t nc = 0;
#pragma unroll 4
  for (int it = 0; it < HIST_ITEMS; ++it) {
    const size_t i = ((size_t)blockIdx.x * HIST_ITEMS + it) * HIST_BLOCK + threadIdx.x;
    if (i >= n) break;
    const uint32_t len = lens ? lens[i] : 1u;
    if (len == 0) continue;
    const int32_t s = r[i];
    const int32_t b = s < 0 ? 0 : s > HIST_BINS - 1 ? HIST_BINS - 1 : s;
    nc += b != s;
    atomicAdd(&hc[b], 1u);
    if (sums) atomicAdd(&hl[b], (unsigned long long)len);
  }
  if (nc) atomicAdd(&hclamp, nc);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < HIST_BINS; i += HIST_BLOCK) {
    if (!hc[i]) continue;
    atomicAdd(&counts[row * HIST_BINS + i], (unsigned long long)hc[i]);
    if (sums) atomicAdd(&len_sums[row * HIST_BINS + i], hl[i]);
  }
  if (clamped && threadIdx.x == 0 && hclamp) atomicAdd(&clamped[row], (unsigned long long)hclamp);
}

// ---- bits and E-values of a hit list ----------------------------------------------------------
// par: per row lambda, K, the query length and ln K, as doubles.
constexpr int SIG_BLOCK = 256, SIG_PAR = 4;

__global__ void __launch_bounds__(SIG_BLOCK) stat_signif(const double* par, const int32_t* hit_scores,
                                                         const uint64_t* hits, const uint32_t* lens,
                                                         size_t k, size_t total, double db_size,
                                                         double* bits, double* evalues) {
  const size_t idx = (size_t)blockIdx.x * SIG_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const uint64_t h = hits[idx];
  if (h == UINT64_MAX) {
    if (bits) bits[idx] = -__builtin_inf();
    if (evalues) evalues[idx] = __builtin_inf();
    return;
  }
  const double* p = par + idx / k * SIG_PAR;
  const double ls = p[0] * (double)hit_scores[idx];
  if (bits) bits[idx] = (ls - p[3]) / 0.693147180559945309417232121458;
  if (evalues) evalues[idx] = db_size * p[1] * p[2] * (double)lens[h] * exp(-ls);
}
}  // namespace swk

extern "C" size_t swk_stat_par_doubles(void) { return swk::SIG_PAR; }

// stride == 0: the caller's layout (out_offs unused); see shuffle_batch.  n < 2^32; max_len
// sizes the lanes' LDS rows and chooses the classes that are launched (a longer target than it
// says is still shuffled, in `out`).
extern "C" hipError_t swk_shuffle_batch(const uint8_t* in, const uint64_t* offs,
                                        const uint32_t* lens, size_t n, uint32_t max_len,
                                        uint64_t k0, uint64_t seed, uint8_t* out,
                                        uint64_t* out_offs, uint32_t stride, hipStream_t st) {
  if (!in || !offs || !lens || !out || n == 0 || n >= 0x100000000ull ||
      ((out_offs != nullptr) != (stride != 0)))
    return hipErrorInvalidValue;
  // an odd number of dwords, so the lanes' bytes of one index sit on different banks
  using namespace swk;
  uint32_t row = (std::min<uint32_t>(std::max<uint32_t>(max_len, 4), SHUF_LANE) + 3) / 4;
  row = (row | 1u) * 4;
  // the classes max_len reaches; what lies past the last of them is walked in `out`
  int classes = 0;
  while (classes < SHUF_CLASSES && max_len > (classes ? SHUF_CLASS[classes - 1] : row)) ++classes;
  const uint32_t top = classes ? SHUF_CLASS[classes - 1] : row;
  hipLaunchKernelGGL(shuffle_batch, dim3((unsigned)((n + 63) / 64)), dim3(64), 64 * row, st, in,
                     offs, lens, n, k0, seed, out, out_offs, stride, row, top);
  hipError_t e = hipGetLastError();
  const size_t XS = (size_t)1 << 24;  // targets of a launch
  for (int c = 0; c < classes && e == hipSuccess; ++c) {
    const uint32_t lo = c ? SHUF_CLASS[c - 1] : row, hi = SHUF_CLASS[c];
    if (hi > (64u << 10)) {  // (past 64 KiB a launch has to ask; the attribute is per device)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(shuffle_long),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)hi);
    }
    for (size_t kb = 0; kb < n && e == hipSuccess; kb += XS) {
      hipLaunchKernelGGL(shuffle_long, dim3((unsigned)std::min(XS, n - kb)), dim3(64), hi, st, in,
                         offs, lens, kb, k0, seed, out, stride, lo, hi);
      e = hipGetLastError();
    }
  }
  return e;
}

// The lane tier's row (i < 0) and the classes' limits in bytes (0 past the last), for the tests.
extern "C" uint32_t swk_shuffle_class_limit(int i) {
  return i < 0 ? (uint32_t)swk::SHUF_LANE : i < swk::SHUF_CLASSES ? swk::SHUF_CLASS[i] : 0u;
}

extern "C" hipError_t swk_stat_hist(const int32_t* scores, const uint32_t* lens, size_t n,
                                    size_t nq, unsigned long long* counts,
                                    unsigned long long* len_sums, unsigned long long* clamped,
                                    hipStream_t st) {
  using namespace swk;
  if (!scores || !counts || n == 0 || nq == 0 || n > 0x100000000ull) return hipErrorInvalidValue;
  const size_t per = (size_t)HIST_BLOCK * HIST_ITEMS;
  const unsigned blocks = (unsigned)((n + per - 1) / per);
  const size_t ROWS = 65535;  // rows of a launch (the grid's y extent)
  for (size_t r0 = 0; r0 < nq; r0 += ROWS) {
    hipLaunchKernelGGL(stat_hist, dim3(blocks, (unsigned)std::min(ROWS, nq - r0)),
                       dim3(HIST_BLOCK), 0, st, scores, lens, n, r0, counts, len_sums, clamped);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" hipError_t swk_stat_signif(const double* par, const int32_t* hit_scores,
                                      const uint64_t* hits, const uint32_t* lens, size_t k,
                                      size_t nq, double db_size, double* bits, double* evalues,
                                      hipStream_t st) {
  using namespace swk;
  if (!par || !hit_scores || !hits || !lens || k == 0 || nq == 0 || (!bits && !evalues))
    return hipErrorInvalidValue;
  const size_t total = nq * k, blocks = (total + SIG_BLOCK - 1) / SIG_BLOCK;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stat_signif, dim3((unsigned)blocks), dim3(SIG_BLOCK), 0, st, par, hit_scores,
                     hits, lens, k, total, db_size, bits, evalues);
  return hipGetLastError();
}
