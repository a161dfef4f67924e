// swbank_ktop.hip — the k best hits of every row of a score matrix (sw_top_hits_device,
// DESIGN.md §3.10): an exact radix select of the k-th largest key, a compaction of the keys at
// or above it, and the final order in one workgroup per row.
//
// key = (score ^ 0x80000000) << 32 | (2^32 - 1 - position), best_kernel's (swbank_kaux.hip):
// the order "higher score first, then lower position" is the descending order of the keys, and
// the keys of a row are distinct.  So the k-th largest key K* is unique and key >= K* selects
// exactly the k wanted targets, however many share the k-th score: the digits of the cut that
// lie in the position half of the key are found like the others.
//
// The kernels are ordered by launches only; inside a launch no workgroup waits for another
// (the last workgroup of a row to finish a histogram pass scans it: sort_hist_scan's pattern).
#include "swbank_kcommon.h"

namespace swk {
constexpr int TOP_BLOCK = 1024;   // threads of a workgroup
#ifndef SWK_TOP_GROUPS
#define SWK_TOP_GROUPS 2  // 16-byte groups of 4 scores a thread of the select's kernels visits
#endif
constexpr int TOP_GROUPS = SWK_TOP_GROUPS;
constexpr int TOP_BINS = 2048;    // bins of a pass (digits of at most 11 bits)
constexpr int TOP_PASSES = 6;     // 5 digits of 11 bits and one of 9, from the top
// Per-row state, 64-bit words: the pass's histogram, then the digits found so far (right
// aligned), the rank wanted among the keys that share them, the pass's finished-workgroup
// count and the compaction's key count (the low 32 bits of a word each).  All zero between
// passes: the last workgroup of a pass clears what it read.
constexpr int TOP_PREFIX = TOP_BINS, TOP_RANK = TOP_BINS + 1, TOP_DONE = TOP_BINS + 2,
              TOP_COUNT = TOP_BINS + 3, TOP_STATE = TOP_BINS + 4;

__device__ __forceinline__ unsigned long long top_key(int32_t score, uint32_t pos) {
  return ((unsigned long long)((uint32_t)score ^ 0x80000000u) << 32) | (0xFFFFFFFFu - pos);
}

// Calls f(key, valid) for the TOP_GROUPS * 4 scores of the row that this thread visits, in the
// same order in every thread (f may use wave-wide operations).  A row starts at any multiple of
// 4 bytes (the stride n may be odd), so the groups are laid over the 16-byte lines the row
// touches: a group wholly inside the row is one 16-byte load, the row's first and last group are
// read score by score, and nothing outside the row is read.
template <class F>
__device__ __forceinline__ void top_visit(const int32_t* row, size_t n, F&& f) {
  const uintptr_t addr = reinterpret_cast<uintptr_t>(row);
  const uint32_t mis = (uint32_t)(addr >> 2) & 3u;  // scores between the line's start and the row's
  const int32_t* base = reinterpret_cast<const int32_t*>(addr - 4 * (uintptr_t)mis);
  const uint64_t end = (uint64_t)mis + n;  // the row is base[mis .. end)
#pragma unroll
  for (int it = 0; it < TOP_GROUPS; ++it) {
    const uint64_t v =
        (((uint64_t)blockIdx.x * TOP_GROUPS + it) * TOP_BLOCK + threadIdx.x) * 4;
    int32_t s[4] = {0, 0, 0, 0};
    if (v >= mis && v + 4 <= end) {
      const int4 q = *reinterpret_cast<const int4*>(base + v);
      s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (v + j >= mis && v + j < end) s[j] = base[v + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = v + j >= mis && v + j < end;
      f(top_key(s[j], (uint32_t)(v + j - mis)), valid);
    }
  }
}

// Workgroups a row of n scores needs, wherever it starts.
inline unsigned top_blocks(size_t n) {
  const uint64_t groups = ((uint64_t)n + 3 + 3) / 4;
  return (unsigned)((groups + TOP_BLOCK * TOP_GROUPS - 1) / (TOP_BLOCK * TOP_GROUPS));
}

// h[bin] += 1 for the active lanes: once per wave when its active lanes share one bin (the score
// digits of a batch whose scores lie in a narrow band), else one LDS atomic per lane.
__device__ __forceinline__ void top_bin_add(uint32_t* h, uint32_t bin, bool active) {
  const uint64_t act = __ballot(active);
  if (!act) return;
  const int leader = __builtin_ctzll(act);
  const uint32_t lb = __builtin_amdgcn_readlane(bin, leader);
  const uint64_t same = __ballot(active && bin == lb);
  if (same == act) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[lb], (uint32_t)__builtin_popcountll(act));
  } else if (active) {
    atomicAdd(&h[bin], 1u);
  }
}

// One pass of the radix select over key bits [lo, hi): the histogram of that digit over the keys
// whose bits [hi, 64) are the digits found so far (every key when hi == 64), per workgroup in LDS
// and one atomic per non-empty bin into the row's; the last workgroup of the row to finish then
// finds, from the top bin down, the bin that holds the rank-th largest of those keys, appends it
// to the digits, lowers the rank by the keys in the bins above it, and clears the histogram.
__global__ void __launch_bounds__(TOP_BLOCK) top_hist(const int32_t* scores, size_t n, size_t row0,
                                                      unsigned long long* state, uint32_t hi,
                                                      uint32_t lo, unsigned long long rank0) {
  __shared__ uint32_t h[TOP_BINS];
  __shared__ unsigned long long part[TOP_BLOCK / 64];  // the waves' sums of the scan
  __shared__ int last;
  const size_t row = row0 + blockIdx.y;
  unsigned long long* st = state + row * TOP_STATE;
  const uint32_t bits = hi - lo, nb = 1u << bits;
  const unsigned long long prefix = hi < 64 ? st[TOP_PREFIX] : 0ull;
  const unsigned long long rank = hi < 64 ? st[TOP_RANK] : rank0;
  for (uint32_t i = threadIdx.x; i < TOP_BINS; i += TOP_BLOCK) h[i] = 0;
  __syncthreads();
  top_visit(scores + row * n, n, [&](unsigned long long key, bool valid) {
    const bool match = valid && (hi == 64 || (key >> hi) == prefix);
    top_bin_add(h, (uint32_t)(key >> lo) & (nb - 1), match);
  });
  __syncthreads();
  // hand-off as in sort_hist_scan (swbank_kaux.hip): the bins are written by device-scope
  // atomics, each wave waits for its own, and the last workgroup (told by the counter's returned
  // value) reads them with agent-scope loads
  for (uint32_t i = threadIdx.x; i < nb; i += TOP_BLOCK)
    if (h[i]) atomicAdd(&st[i], (unsigned long long)h[i]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t* done = reinterpret_cast<uint32_t*>(&st[TOP_DONE]);
  if (threadIdx.x == 0) last = atomicAdd(done, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  // thread t owns the bins nb - 1 - 2t and nb - 2 - 2t: a scan from the top bin down
  const uint32_t r0 = threadIdx.x * 2;
  const bool own0 = r0 < nb, own1 = r0 + 1 < nb;
  const uint32_t b0 = own0 ? nb - 1 - r0 : 0u, b1 = own1 ? nb - 2 - r0 : 0u;
  const unsigned long long a =
      own0 ? __hip_atomic_load(&st[b0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  const unsigned long long c =
      own1 ? __hip_atomic_load(&st[b1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  // inclusive scan of a + c over the workgroup: by shuffles inside a wave, then the sums of the
  // waves before this one
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = a + c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += part[w];
  const unsigned long long above = incl - (a + c);  // keys in the bins above b0
  // rank <= the keys counted (min(k, n) at first, a bin's count after that), so one bin has it
  if (above < rank && rank <= above + a) {
    st[TOP_PREFIX] = (prefix << bits) | b0;
    st[TOP_RANK] = rank - above;
  } else if (above + a < rank && rank <= above + a + c) {
    st[TOP_PREFIX] = (prefix << bits) | b1;
    st[TOP_RANK] = rank - above - a;
  }
  if (own0) st[b0] = 0;
  if (own1) st[b1] = 0;
  if (threadIdx.x == 0) *done = 0;
}

// After the last pass the digits are K*.  Every key >= max(K*, floor) (floor: the lowest key of
// the score min_score) goes into the row's k slots, in any order.  At most min(k, n) <= 4096 keys
// are >= K*, so a workgroup stages its own in LDS (one LDS atomic per wave that has any), takes
// its range of the slots with one global atomic, and copies them there: with one global atomic
// per wave, the 4,096 waves that each hold one of the best of a million queued on one address.
__global__ void __launch_bounds__(TOP_BLOCK) top_select(const int32_t* scores, size_t n,
                                                        size_t row0, unsigned long long* state,
                                                        unsigned long long* keys, size_t k,
                                                        unsigned long long floor) {
  __shared__ unsigned long long mine[4096];
  __shared__ uint32_t held, base;
  const size_t row = row0 + blockIdx.y;
  unsigned long long* st = state + row * TOP_STATE;
  const unsigned long long kth = st[TOP_PREFIX], cut = kth > floor ? kth : floor;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) held = 0;
  __syncthreads();
  top_visit(scores + row * n, n, [&](unsigned long long key, bool valid) {
    const bool take = valid && key >= cut;
    const uint64_t m = __ballot(take);
    if (!m) return;
    const int leader = __builtin_ctzll(m);
    uint32_t slot = 0;
    if (lane == leader) slot = atomicAdd(&held, (uint32_t)__builtin_popcountll(m));
    slot = __builtin_amdgcn_readlane(slot, leader) +
           (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1));
    if (take && slot < 4096) mine[slot] = key;
  });
  __syncthreads();
  const uint32_t have = held < 4096 ? held : 4096;
  if (have == 0) return;
  if (threadIdx.x == 0)
    base = atomicAdd(reinterpret_cast<uint32_t*>(&st[TOP_COUNT]), have);
  __syncthreads();
  unsigned long long* out = keys + row * k;
  for (uint32_t i = threadIdx.x; i < have; i += TOP_BLOCK)
    if ((size_t)base + i < k) out[base + i] = mine[i];
}

// One compare-exchange of the bitonic network on slot i, whose partner slot i ^ stride holds y:
// in the phase of run length `size`, runs whose `size` bit is clear end up descending, and the
// lower slot of a pair in such a run keeps the larger key.
__device__ __forceinline__ unsigned long long top_cmpx(unsigned long long x, unsigned long long y,
                                                       uint32_t i, uint32_t size,
                                                       uint32_t stride) {
  const bool keep_max = ((i & stride) == 0) == ((i & size) == 0);
  return (x > y) == keep_max ? x : y;
}

// One workgroup per row: the row's keys (at most k <= 4096) into descending order by a bitonic
// sort over P >= k slots (P a power of two; the slots past the count hold key 0, the lowest),
// then position, score and id of every key, and the sentinels past the count.  A thread holds
// the 4 slots wave * 256 + e * 64 + lane in registers, so only the strides of 256 and more (10
// of the 78 steps at P = 4096) go through LDS and barriers: strides 64 and 128 are between a
// thread's own registers, the strides below 64 are wave shuffles.
__global__ void __launch_bounds__(TOP_BLOCK) top_order(const unsigned long long* state,
                                                       const unsigned long long* keys,
                                                       const uint64_t* ids, size_t k, uint32_t P,
                                                       size_t row0, uint64_t* hits,
                                                       int32_t* hit_scores, uint64_t* hit_ids,
                                                       uint32_t* counts) {
  __shared__ unsigned long long s[4096];
  const size_t row = row0 + blockIdx.x;
  const unsigned long long* st = state + row * TOP_STATE;
  const uint32_t have = *reinterpret_cast<const uint32_t*>(&st[TOP_COUNT]);
  const uint32_t cnt = have < k ? have : (uint32_t)k;
  const uint32_t slot0 = (threadIdx.x >> 6) * 256 + (threadIdx.x & 63);  // slot of e: + 64 e
  unsigned long long v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = slot0 + 64 * e < cnt ? keys[row * k + slot0 + 64 * e] : 0ull;
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride >= 256; stride >>= 1) {  // across waves
      __syncthreads();  // (the reads of the step before are done)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[slot0 + 64 * e] = v[e];
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = top_cmpx(v[e], s[(slot0 + 64 * e) ^ stride], slot0 + 64 * e, size, stride);
    }
    if (size >= 256) {  // stride 128: registers 0 | 2 and 1 | 3
      const unsigned long long a = v[0], b = v[1], c = v[2], d = v[3];
      v[0] = top_cmpx(a, c, slot0, size, 128), v[2] = top_cmpx(c, a, slot0 + 128, size, 128);
      v[1] = top_cmpx(b, d, slot0 + 64, size, 128), v[3] = top_cmpx(d, b, slot0 + 192, size, 128);
    }
    if (size >= 128) {  // stride 64: registers 0 | 1 and 2 | 3
      const unsigned long long a = v[0], b = v[1], c = v[2], d = v[3];
      v[0] = top_cmpx(a, b, slot0, size, 64), v[1] = top_cmpx(b, a, slot0 + 64, size, 64);
      v[2] = top_cmpx(c, d, slot0 + 128, size, 64), v[3] = top_cmpx(d, c, slot0 + 192, size, 64);
    }
    for (uint32_t stride = size >> 1 < 32 ? size >> 1 : 32; stride > 0; stride >>= 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = top_cmpx(v[e], __shfl_xor(v[e], (int)stride), slot0 + 64 * e, size, stride);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t j = slot0 + 64 * e;
    if (j >= k) continue;
    const bool hit = j < cnt;
    const unsigned long long key = v[e];
    const uint64_t pos = 0xFFFFFFFFull - (key & 0xFFFFFFFFull);
    hits[row * k + j] = hit ? pos : UINT64_MAX;
    if (hit_scores)
      hit_scores[row * k + j] = hit ? (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u) : INT32_MIN;
    if (hit_ids) hit_ids[row * k + j] = !hit ? UINT64_MAX : ids ? ids[pos] : pos;
  }
  if (counts && threadIdx.x == 0) counts[row] = cnt;
}
}  // namespace swk

extern "C" size_t swk_top_state_words(void) { return swk::TOP_STATE; }

// The k best of each of the nq rows of n scores (1 <= k <= 4096, n <= 2^32): see
// sw_top_hits_device.  state: nq * swk_top_state_words() 64-bit words, keys: nq * k, both
// scratch that the call initialises itself.
extern "C" hipError_t swk_top_hits(const int32_t* scores, const uint64_t* ids, size_t n, size_t nq,
                                   size_t k, int32_t min_score, unsigned long long* state,
                                   unsigned long long* keys, uint64_t* hits, int32_t* hit_scores,
                                   uint64_t* hit_ids, uint32_t* counts, hipStream_t st) {
  using namespace swk;
  hipError_t e = hipMemsetAsync(state, 0, nq * TOP_STATE * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const unsigned blocks = top_blocks(n);
  const unsigned long long rank0 = std::min(k, n);
  const unsigned long long floor = (unsigned long long)((uint32_t)min_score ^ 0x80000000u) << 32;
  uint32_t P = 1;
  while (P < k) P <<= 1;
  const size_t ROWS = 65535;  // rows of a launch (the grid's y extent)
  for (int p = 0; p < TOP_PASSES; ++p) {  // bits [53, 64), [42, 53), ..., [9, 20), [0, 9)
    const uint32_t hi = 64 - 11 * p, lo = p + 1 < TOP_PASSES ? hi - 11 : 0;
    for (size_t r0 = 0; r0 < nq; r0 += ROWS) {
      const dim3 grid(blocks, (unsigned)std::min(ROWS, nq - r0));
      hipLaunchKernelGGL(top_hist, grid, dim3(TOP_BLOCK), 0, st, scores, n, r0, state, hi, lo,
                         rank0);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  for (size_t r0 = 0; r0 < nq; r0 += ROWS) {
    const dim3 grid(blocks, (unsigned)std::min(ROWS, nq - r0));
    hipLaunchKernelGGL(top_select, grid, dim3(TOP_BLOCK), 0, st, scores, n, r0, state, keys, k,
                       floor);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const size_t ORD = 0x7FFFFFFF;
  for (size_t r0 = 0; r0 < nq; r0 += ORD) {
    hipLaunchKernelGGL(top_order, dim3((unsigned)std::min(ORD, nq - r0)), dim3(TOP_BLOCK), 0, st,
                       state, keys, ids, k, P, r0, hits, hit_scores, hit_ids, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}
