// swbank_kbestq.hip — the best query of every target: the maximum down each column of an
// nq x n score matrix (include/swbank.h "the best query per target").
//
// Memory-bound: one read of nq x n x 4 bytes.  A workgroup of 256 threads covers W adjacent
// columns (W = 256, or the power of two >= n below that) and 256 / W row phases: thread
// (tx, ty) walks rows ty, ty + 256 / W, ... of the workgroup's row range down column tx, so a
// wave's loads are dword loads along n (rows start at any multiple of 4 bytes; nothing outside
// the matrix is read).  The candidates are best_kernel's 64-bit keys (swbank_kaux.hip),
//   key = (score ^ 0x80000000) << 32 | (2^32 - 1 - query),
// one 64-bit max picks the highest score and among equals the lowest query.  The row phases
// meet in LDS.  When the columns alone give too few workgroups the query axis is split over
// blockIdx.y and the parts meet by atomicMax on n keys of bank scratch (zeroed before; every
// real key is > 0), a second launch writes the outputs: no workgroup waits for another, and the
// keys of a column being distinct the result does not depend on the order of arrival.
#include "swbank.h"
#include "swbank_kcommon.h"

namespace swk {
constexpr unsigned BQ_THREADS = 256;
constexpr unsigned BQ_BLOCKS = 512;  // workgroups the split form aims at (2 per CU)
constexpr unsigned BQ_MIN_ROWS = 4;  // rows per thread below which the query axis is not split

__device__ __forceinline__ void bq_write(unsigned long long key, size_t k, int32_t min_score,
                                         uint32_t* best_query, int32_t* best_score) {
  int32_t s = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
  uint32_t q = 0xFFFFFFFFu - (uint32_t)key;
  if (s < min_score) {
    s = INT32_MIN;
    q = SW_QUERY_NONE;
  }
  if (best_query) best_query[k] = q;
  if (best_score) best_score[k] = s;
}

// keys == nullptr: gridDim.y == 1 and the outputs are written here.
__global__ void __launch_bounds__(BQ_THREADS) best_queries(const int32_t* scores, size_t n,
                                                           uint32_t nq, uint32_t wshift,
                                                           uint32_t rows, int32_t min_score,
                                                           unsigned long long* keys,
                                                           uint32_t* best_query,
                                                           int32_t* best_score) {
  __shared__ unsigned long long red[BQ_THREADS];
  const uint32_t W = 1u << wshift, R = BQ_THREADS >> wshift;
  const uint32_t tx = threadIdx.x & (W - 1), ty = threadIdx.x >> wshift;
  const size_t k = (size_t)blockIdx.x * W + tx;
  const uint32_t r0 = blockIdx.y * rows, r1 = min(nq, r0 + rows);
  unsigned long long m = 0;
  if (k < n) {
    const int32_t* col = scores + k;
#pragma unroll 4
    for (uint32_t i = r0 + ty; i < r1; i += R) {
      const unsigned long long v =
          ((unsigned long long)((uint32_t)col[(size_t)i * n] ^ 0x80000000u) << 32) |
          (0xFFFFFFFFull - i);
      m = v > m ? v : m;
    }
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (uint32_t w = BQ_THREADS / 2; w >= W; w >>= 1) {  // (thread t and t + w share a column)
    if (threadIdx.x < w && red[threadIdx.x + w] > red[threadIdx.x])
      red[threadIdx.x] = red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < W && k < n) {
    if (keys) atomicMax(&keys[k], red[threadIdx.x]);
    else bq_write(red[threadIdx.x], k, min_score, best_query, best_score);
  }
}

__global__ void __launch_bounds__(BQ_THREADS) best_queries_out(const unsigned long long* keys,
                                                               size_t n, int32_t min_score,
                                                               uint32_t* best_query,
                                                               int32_t* best_score) {
  const size_t k = (size_t)blockIdx.x * BQ_THREADS + threadIdx.x;
  if (k < n) bq_write(keys[k], k, min_score, best_query, best_score);
}

// The launch shape of an nq x n matrix: log2 of the columns per workgroup, the rows per
// workgroup and the workgroups along the query axis.
static void bq_shape(size_t n, size_t nq, unsigned& wshift, unsigned& rows, unsigned& gy) {
  wshift = 8;
  while (wshift > 0 && ((size_t)1 << (wshift - 1)) >= n) --wshift;
  const size_t gx = (n + ((size_t)1 << wshift) - 1) >> wshift;
  const size_t R = BQ_THREADS >> wshift;
  const size_t most = std::max<size_t>(1, nq / (BQ_MIN_ROWS * R));
  const size_t want = std::min<size_t>(most, (BQ_BLOCKS + gx - 1) / gx);
  rows = (unsigned)((nq + want - 1) / want);
  gy = (unsigned)((nq + rows - 1) / rows);
}
}  // namespace swk

extern "C" size_t swk_best_queries_keys(size_t n, size_t nq) {
  unsigned wshift, rows, gy;
  swk::bq_shape(n, nq, wshift, rows, gy);
  return gy > 1 ? n : 0;
}

// best_query[k] / best_score[k] (either may be null) of every column k < n of scores[nq x n];
// keys: swk_best_queries_keys(n, nq) words of scratch.  1 <= nq <= 65536, 1 <= n <= 2^32.
extern "C" hipError_t swk_best_queries(const int32_t* scores, size_t n, size_t nq,
                                       int32_t min_score, unsigned long long* keys,
                                       uint32_t* best_query, int32_t* best_score,
                                       hipStream_t st) {
  if (!scores || n == 0 || nq == 0 || nq > 65536 || n > 0x100000000ull ||
      (!best_query && !best_score))
    return hipErrorInvalidValue;
  unsigned wshift, rows, gy;
  swk::bq_shape(n, nq, wshift, rows, gy);
  const size_t gx = (n + ((size_t)1 << wshift) - 1) >> wshift;
  if (gy > 1) {
    if (!keys) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(keys, 0, n * sizeof(*keys), st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(swk::best_queries, dim3((unsigned)gx, gy), dim3(swk::BQ_THREADS), 0, st,
                     scores, n, (uint32_t)nq, wshift, rows, min_score, gy > 1 ? keys : nullptr,
                     best_query, best_score);
  if (gy > 1)
    hipLaunchKernelGGL(swk::best_queries_out,
                       dim3((unsigned)((n + swk::BQ_THREADS - 1) / swk::BQ_THREADS)),
                       dim3(swk::BQ_THREADS), 0, st, keys, n, min_score, best_query, best_score);
  return hipGetLastError();
}
