// swbank_klalign.hip — the kernel behind the non-intersecting local alignments of a pair
// (include/swbank.h "non-intersecting local alignments").
//
// One wave per hit and one launch per round.  Round r of a hit
//   walks the whole matrix (la_walk, swbank_klawalk.h): the local Gotoh recurrence in which the
//     cells of the paths of rounds 0 .. r-1 hold H = 0 and E = F = -infinity; one direction byte
//     per cell, bit 7 carried over from the previous round's byte; the best cell under the end
//     rule of sw_align_hits;
//   then lane 0 follows the bytes from that cell in state H until a cell with H = 0 or the edge
//     of the matrix, as pass D of swbank_kglalign.hip does: it re-scores what it walks, sets bit 7
//     on every cell it visits, emits the ops backwards and reverses them in place.
// The record of (hit h, round r) is out[h * rounds + r].  A round whose score is below min_score
// leaves an empty record, and so does every later round of that hit, at once.  Nothing waits
// inside the kernel or across workgroups; every store is an ordinary vector store; the rounds of
// a hit are ordered by the stream.
#include "swbank.h"
#include "swbank_align.h"
#include "swbank_kcommon.h"
#include "swbank_klawalk.h"

namespace swk {
struct LaArgs {
  SwkLaAlign p;
  size_t h0;
  uint32_t round;
};

// The target as it lies; a code past the alphabet reads as its last code.
struct LaTarget {
  const uint8_t* tp;
  uint32_t last;
  __device__ __forceinline__ uint32_t operator()(uint32_t x) const { return min(tp[x], last); }
};

template <int K, bool FIRST>
__global__ void __launch_bounds__(64) lalign_round(const LaArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[GL_MAX_ALPHA * ROWS];
  const SwkLaAlign& p = a.p;
  const uint32_t tid = threadIdx.x;
  const size_t k = blockIdx.x;  // (< count)
  const size_t h = a.h0 + k;
  const size_t x = h * p.rounds + a.round;
  sw_alignment* out = static_cast<sw_alignment*>(p.out);
  sw_alignment r;
  r.score = 0;
  r.q_start = r.q_end = r.t_start = r.t_end = 0u;
  r.n_columns = r.n_identities = 0;
  r.cigar_offset = p.cigar && p.cigar_stride && !p.plan ? (uint32_t)(x * p.cigar_stride) : 0u;
  r.cigar_len = 0;
  // hit h's pair
  const uint64_t t = p.hits ? p.hits[h] : (uint64_t)h;
  const uint32_t qi = p.hit_queries ? p.hit_queries[h] : (uint32_t)(h / p.hits_per_query);
  if (qi >= p.nq || t >= p.n) {
    r.index = r.id = SW_HIT_NONE;
    r.flags = (uint32_t)SW_ALIGN_EMPTY | (uint32_t)SW_ALIGN_NO_HIT;
    if (tid == 0) out[x] = r;
    return;
  }
  r.index = t;
  r.id = p.ids ? p.ids[t] : t;
  r.flags = (uint32_t)SW_ALIGN_EMPTY;
  const uint2 qe = p.qtab[qi];
  const uint8_t* qp = p.query + qe.x;
  const uint32_t m = __builtin_amdgcn_readfirstlane(min(qe.y, (uint32_t)ROWS));
  const uint32_t L = __builtin_amdgcn_readfirstlane(min(p.lens[t], p.max_len));
  uint64_t dir_off = (uint64_t)k * p.slot, dir_cap = p.slot, cig_off = x * (uint64_t)p.cigar_stride;
  uint32_t cig_cap = p.cigar ? p.cigar_stride : 0u;
  if (p.plan) {
    dir_off = p.plan[h].dir_off;
    dir_cap = p.plan[h].dir_cap;
    cig_cap = p.cigar ? p.plan[h].cig_cap : 0u;
    cig_off = p.plan[h].cig_off + (uint64_t)a.round * cig_cap;
  }
  bool over = m == 0 || L == 0 || gl_dir_dwords(K, m, L) > dir_cap;  // (the host sized the store)
  if constexpr (!FIRST) over = over || (out[x - 1].flags & (uint32_t)SW_ALIGN_EMPTY) != 0;
  if (over) {
    if (tid == 0) out[x] = r;
    return;
  }
  gl_profile<K>(p.mat, p.alpha, prof, qp, m, 64);
  __syncthreads();
  const LaTarget code{p.res + p.offs[t], p.alpha - 1};
  uint32_t* dirs = p.dirs + dir_off;
  const LaBest b = la_walk<K, FIRST>(prof, code, L, m, p.o, p.e, dirs);
  __threadfence();  // lane 0 reads what the other lanes stored
  __syncthreads();
  if (tid != 0) return;
  if (b.v < p.min_score) {
    out[x] = r;
    return;
  }

  // the path
  uint8_t* db = reinterpret_cast<uint8_t*>(dirs);
  uint32_t* cig = p.cigar + cig_off;  // (written only below cig_cap)
  int64_t i = b.i, c = b.j;
  uint32_t qs = b.i, ts = b.j;
  uint32_t nops = 0, cur = 0, run = 0, cols = 0, idn = 0;
  int32_t acc = 0;  // what the walked path scores
  int state = 3;    // 0 M, 1 E, 2 F, 3 H (the end cell is walked in state H)
  bool done = false;
  const auto flush = [&] {
    if (run) {
      if (nops < cig_cap) cig[nops] = run << 4 | cur;
      ++nops;
    }
    run = 0;
  };
  const auto emit = [&](uint32_t op) {
    if (run && op == cur) {
      ++run;
    } else {
      flush();
      cur = op;
      run = 1;
    }
    ++cols;
  };
  for (uint64_t it = 0, lim = (uint64_t)m + L + 2; it < lim; ++it) {
    if (i < 0 || c < 0) {  // the edge of the matrix: a path ends there after an M only
      done = state == 3;
      break;
    }
    const uint32_t ln = (uint32_t)i / K, rr = (uint32_t)i % K;
    const uint64_t st = (uint64_t)c + ln;
    uint8_t* cell = db + ((st * (K / 4) + rr / 4) * 64 + ln) * 4 + rr % 4;
    const uint32_t bits = *cell;
    if (state == 3) {
      state = (int)(bits & 3u);
      if (state == (int)LA_SRC_ZERO) {  // H = 0: not part of the path
        done = true;
        break;
      }
    }
    *cell = (uint8_t)(bits | LA_USED);
    qs = (uint32_t)i;
    ts = (uint32_t)c;
    if (state == 0) {
      const uint32_t tc = code((uint32_t)c);
      emit(SW_CIGAR_M);
      idn += qp[i] == tc;
      acc += prof[tc * ROWS + i];
      --i;
      --c;
      state = 3;
    } else if (state == 1) {
      emit(SW_CIGAR_D);
      acc += (bits & GL_E_EXT) ? p.e : p.o;
      state = (bits & GL_E_EXT) ? 1 : 3;
      --c;
    } else {
      emit(SW_CIGAR_I);
      acc += (bits & GL_F_EXT) ? p.e : p.o;
      state = (bits & GL_F_EXT) ? 2 : 3;
      --i;
    }
  }
  flush();
  r.score = b.v;
  r.q_start = qs;
  r.q_end = b.i;
  r.t_start = ts;
  r.t_end = b.j;
  r.flags = (uint32_t)SW_ALIGN_NO_PATH;
  if (done && acc == b.v && nops <= cig_cap && nops) {
    for (uint32_t y = 0; y < nops / 2; ++y) {
      const uint32_t v = cig[y];
      cig[y] = cig[nops - 1 - y];
      cig[nops - 1 - y] = v;
    }
    r.flags = 0;
    r.n_columns = cols;
    r.n_identities = idn;
    r.cigar_len = nops;
  }
  out[x] = r;
}

static bool la_args_ok(const SwkLaAlign* p) {
  return p && p->res && p->offs && p->lens && p->qtab && p->mat && p->query && p->out && p->dirs &&
         p->n && p->nq && p->qlen && p->qlen <= 1024 && p->alpha &&
         p->alpha <= (uint32_t)GL_MAX_ALPHA &&
         (p->hit_queries != nullptr) != (p->hits_per_query != 0) && p->rounds >= 1 &&
         p->rounds <= 64 && p->min_score >= 1 && p->n_hits <= 0xFFFFFFFFull && p->o <= 0 &&
         p->e <= 0 && p->o >= -65534 && p->e >= -32767;
}

template <int K>
static void la_launch(const LaArgs& a, dim3 grid, hipStream_t st) {
  if (a.round == 0)
    hipLaunchKernelGGL((lalign_round<K, true>), grid, dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((lalign_round<K, false>), grid, dim3(64), 0, st, a);
}
}  // namespace swk

extern "C" uint64_t swk_lalign_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t cols) {
  return swk::gl_dir_dwords(swk::gl_rows(qlen), rows, cols);
}

extern "C" hipError_t swk_launch_lalign_round(const SwkLaAlign* p, size_t h0, size_t count,
                                              uint32_t round, hipStream_t st) {
  using namespace swk;
  if (!p || count == 0) return hipSuccess;
  if (!la_args_ok(p) || round >= p->rounds || h0 + count > p->n_hits ||
      count > ((size_t)1 << 30))
    return hipErrorInvalidValue;
  const LaArgs a{*p, h0, round};
  const dim3 grid((unsigned)count);
  switch (gl_rows(p->qlen)) {
    case 4: la_launch<4>(a, grid, st); break;
    case 8: la_launch<8>(a, grid, st); break;
    default: la_launch<16>(a, grid, st); break;
  }
  return hipGetLastError();
}
