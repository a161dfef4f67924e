// swbank_kstrand.hip — the kernels of the both-strand search (include/swbank.h "both DNA
// strands"): the reverse complement of a batch and the merge of the forward
// and reverse-strand score matrices.  Both are small beside the two scoring passes they
// surround and are kept plain; inside a launch no workgroup waits for another.
#include "swbank.h"
#include "swbank_kcommon.h"

namespace swk {
// T <-> A (0 <-> 2), C <-> G (1 <-> 3); N and anything past it stays.
__device__ __forceinline__ uint8_t rc_code(uint8_t c) { return c < 4 ? (uint8_t)(c ^ 2) : c; }

__device__ __forceinline__ uint32_t rc_lane_u32(uint32_t v, int t) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, t);
}
__device__ __forceinline__ unsigned long long rc_lane_u64(unsigned long long v, int t) {
  return ((unsigned long long)rc_lane_u32((uint32_t)(v >> 32), t) << 32) |
         rc_lane_u32((uint32_t)v, t);
}

// ---- the reverse complement -----------------------------------------------------------------
// A workgroup is one wave and owns 64 adjacent targets (the shuffle's shape, swbank_kstat.hip):
// the lanes read the 64 offsets and lengths together, then the wave walks the targets, 64
// adjacent bytes of one target per access, a group's loads before its stores.  One path serves
// every length: the wave runs until its longest target is done.
// out_offs == nullptr: target k goes to out + offs[k] (the caller's layout); else to
// out + k * stride, and that offset to out_offs[k] (the bank's scratch, whose size the host knows
// without reading offsets).
constexpr int RC_GROUP = 8;  // targets whose loads are in flight together

__global__ void __launch_bounds__(64) revcomp_batch(const uint8_t* __restrict__ in,
                                                    const uint64_t* __restrict__ offs,
                                                    const uint32_t* __restrict__ lens, size_t n,
                                                    uint8_t* __restrict__ out, uint64_t* out_offs,
                                                    uint32_t stride) {
  const int lane = threadIdx.x;
  const size_t k = (size_t)blockIdx.x * 64 + lane;
  const bool have = k < n;
  const unsigned long long off = have ? offs[k] : 0ull;
  const uint32_t len = have ? lens[k] : 0u;
  const unsigned long long to = out_offs ? (unsigned long long)k * stride : off;
  if (have && out_offs) out_offs[k] = to;
  for (uint32_t c = 0;; c += 64) {
    const unsigned long long live = __ballot(len > c);  // targets with codes at or past c
    if (!live) break;
    const uint32_t i = c + lane;
    for (int t0 = 0; t0 < 64; t0 += RC_GROUP) {
      if (!((live >> t0) & ((1ull << RC_GROUP) - 1))) continue;
      uint8_t v[RC_GROUP];
#pragma unroll
      for (int u = 0; u < RC_GROUP; ++u) {
        const uint32_t tl = rc_lane_u32(len, t0 + u);
        v[u] = i < tl ? in[rc_lane_u64(off, t0 + u) + (tl - 1 - i)] : (uint8_t)0;
      }
#pragma unroll
      for (int u = 0; u < RC_GROUP; ++u)
        if (i < rc_lane_u32(len, t0 + u)) out[rc_lane_u64(to, t0 + u) + i] = rc_code(v[u]);
    }
    if (c > 0xFFFFFFFFu - 64) break;
  }
}

// ---- the strand merge ---------------------------------------------------------------------------
// fwd: nq rows of n scores; rev: nq rows of nk scores, the slice [k0, k0 + nk) of the targets.
// blockIdx.y is the row.  A tie is the forward strand.
constexpr int MERGE_BLOCK = 256;

__global__ void __launch_bounds__(MERGE_BLOCK) strand_merge(int32_t* __restrict__ fwd,
                                                            const int32_t* __restrict__ rev,
                                                            uint8_t* __restrict__ strands, size_t n,
                                                            size_t k0, size_t nk, size_t row0) {
  const size_t k = (size_t)blockIdx.x * MERGE_BLOCK + threadIdx.x;
  if (k >= nk) return;
  const size_t row = row0 + blockIdx.y, at = row * n + k0 + k;
  const int32_t f = fwd[at], r = rev[row * nk + k];
  if (r > f) fwd[at] = r;
  if (strands) strands[at] = r > f ? 1 : 0;
}
}  // namespace swk

// stride == 0: the caller's layout (out_offs unused); see revcomp_batch.  n < 2^32.
extern "C" hipError_t swk_revcomp_batch(const uint8_t* in, const uint64_t* offs,
                                        const uint32_t* lens, size_t n, uint8_t* out,
                                        uint64_t* out_offs, uint32_t stride, hipStream_t st) {
  if (!in || !offs || !lens || !out || n == 0 || n >= 0x100000000ull ||
      ((out_offs != nullptr) != (stride != 0)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(swk::revcomp_batch, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, in, offs,
                     lens, n, out, out_offs, stride);
  return hipGetLastError();
}

extern "C" hipError_t swk_strand_merge(int32_t* fwd, const int32_t* rev, uint8_t* strands, size_t n,
                                       size_t k0, size_t nk, size_t nq, hipStream_t st) {
  using namespace swk;
  if (!fwd || !rev || nk == 0 || nq == 0 || k0 > n || nk > n - k0 || n > 0x100000000ull)
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((nk + MERGE_BLOCK - 1) / MERGE_BLOCK);
  const size_t ROWS = 65535;  // rows of a launch (the grid's y extent)
  for (size_t r0 = 0; r0 < nq; r0 += ROWS) {
    hipLaunchKernelGGL(strand_merge, dim3(blocks, (unsigned)std::min(ROWS, nq - r0)),
                       dim3(MERGE_BLOCK), 0, st, fwd, rev, strands, n, k0, nk, r0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
