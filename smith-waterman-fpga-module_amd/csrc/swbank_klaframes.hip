// swbank_klaframes.hip — the kernels behind the non-intersecting alignments over the six reading
// frames of a hit (include/swbank.h "non-intersecting alignments over reading frames", DESIGN.md
// §3.20).
//
// The six frames of a DNA target are six unrelated matrices of one protein query, each with its
// own direction store and its own used cells.  A hit keeps one pending candidate per frame, the
// best remaining cell of that frame's matrix, in a small state; a round reports the best of the
// six (the largest score, then the lowest frame), follows its path as lalign_round does
// (swbank_klalign.hip) and marks its cells, which changes the matrix of that frame alone.
//   Round 0: one workgroup of six waves per hit.  The waves share the query's profile in LDS; wave
//     f walks frame f (la_walk, swbank_klawalk.h, FIRST) into its part of the hit's store, reading
//     the amino acid of a column from three DNA codes and the codon table as it goes -- frames
//     3..5 from the far end, complemented; nothing is translated into memory.
//   Round r > 0: one wave per hit walks the frame the previous record came from again, with that
//     frame's used cells, and refreshes its candidate; the other five are still exact.
// Then one thread picks the winner and follows its path.  The record of (hit h, round r) is
// out[h * rounds + r] with the frame in its flags and nucleotide coordinates; a winner below
// min_score leaves an empty record, and so does every later round of that hit, at once.  Nothing
// waits across workgroups; every store is an ordinary vector store; the rounds of a hit are
// ordered by the stream.  The number of planes and how a plane reads its columns are a template
// parameter (FramePlanes); the kernels know neither.
#include "swbank.h"
#include "swbank_align.h"
#include "swbank_kcommon.h"
#include "swbank_klawalk.h"

namespace swk {
struct LfTable {  // byte i of the table is byte i of the words in LDS
  uint32_t w[16];
};
struct LfArgs {
  SwkLaAlign p;
  LfTable table;
  int32_t* state;
  size_t h0;
  uint32_t round;
};

// Column j of one reading frame of a target of L codes: the amino acid of its codon, X when a
// code is no nucleotide; a code past the alphabet reads as its last code.
struct FrameCode {
  const uint8_t* tp;
  const uint8_t* tab;
  uint32_t L, o, rev, last;
  __device__ __forceinline__ uint32_t operator()(uint32_t j) const {
    const uint32_t s = o + 3 * j;  // (s + 2 < L)
    const uint32_t c0 = rev ? tp[L - 1 - s] : tp[s];
    const uint32_t c1 = rev ? tp[L - 2 - s] : tp[s + 1];
    const uint32_t c2 = rev ? tp[L - 3 - s] : tp[s + 2];
    const uint32_t flip = rev ? 0x2Au : 0u;  // T <-> A, C <-> G: code ^ 2
    const uint32_t aa = (c0 | c1 | c2) < 4 ? tab[(c0 * 16 + c1 * 4 + c2) ^ flip] : 22u;  // X
    return min(aa, last);
  }
};

// The six reading frames as the planes of a hit: frame f < 3 starts at code f of the target,
// frame f >= 3 at code f - 3 of its reverse complement.
struct FramePlanes {
  static constexpr int N = SW_FRAME_COUNT;
  using Code = FrameCode;
  __device__ static __forceinline__ uint32_t cols(uint32_t L, uint32_t f) {
    const uint32_t o = f % 3;
    return L >= o + 3 ? (L - o) / 3 : 0u;
  }
  __device__ static __forceinline__ Code code(const uint8_t* tp, const uint8_t* tab, uint32_t L,
                                              uint32_t f, uint32_t last) {
    return Code{tp, tab, L, f % 3, f >= 3 ? 1u : 0u, last};
  }
  // the plane's flags, and a plane's columns [ts, te] on the forward target
  __device__ static __forceinline__ void place(sw_alignment& r, uint32_t f, uint32_t L) {
    const uint32_t o = f % 3;
    r.flags |= (o << SW_ALIGN_FRAME_SHIFT) | (f >= 3 ? (uint32_t)SW_ALIGN_REVERSE : 0u);
    const uint32_t fs = o + 3 * r.t_start, fe = o + 3 * r.t_end + 2;
    r.t_start = f < 3 ? fs : L - 1 - fe;
    r.t_end = f < 3 ? fe : L - 1 - fs;
  }
};

// What both kernels know of their hit before they walk.
struct LfHit {
  sw_alignment r;  // the empty record of the slot
  const uint8_t* qp;
  const uint8_t* tp;
  uint32_t m, L, cig_cap;
  uint32_t* dirs;  // the hit's store, the planes back to back
  uint32_t* cig;   // (written only below cig_cap)
  int32_t* state;
  bool pair, over;
};

template <int K, class PL>
__device__ __forceinline__ LfHit lf_hit(const LfArgs& a) {
  constexpr int ROWS = 64 * K;
  const SwkLaAlign& p = a.p;
  const size_t k = blockIdx.x;  // (< count)
  const size_t h = a.h0 + k;
  const size_t x = h * p.rounds + a.round;
  LfHit w;
  sw_alignment& r = w.r;
  r.score = 0;
  r.q_start = r.q_end = r.t_start = r.t_end = 0u;
  r.n_columns = r.n_identities = 0;
  r.cigar_offset = p.cigar && p.cigar_stride && !p.plan ? (uint32_t)(x * p.cigar_stride) : 0u;
  r.cigar_len = 0;
  const uint64_t t = p.hits ? p.hits[h] : (uint64_t)h;
  const uint32_t qi = p.hit_queries ? p.hit_queries[h] : (uint32_t)(h / p.hits_per_query);
  w.pair = qi < p.nq && t < p.n;
  w.over = true;
  w.state = a.state + k * SWK_LAFRAMES_STATE;
  if (!w.pair) {
    r.index = r.id = SW_HIT_NONE;
    r.flags = (uint32_t)SW_ALIGN_EMPTY | (uint32_t)SW_ALIGN_NO_HIT;
    return w;
  }
  r.index = t;
  r.id = p.ids ? p.ids[t] : t;
  r.flags = (uint32_t)SW_ALIGN_EMPTY;
  const uint2 qe = p.qtab[qi];
  w.qp = p.query + qe.x;
  w.tp = p.res + p.offs[t];
  w.m = __builtin_amdgcn_readfirstlane(min(qe.y, (uint32_t)ROWS));
  w.L = __builtin_amdgcn_readfirstlane(min(p.lens[t], p.max_len));
  uint64_t dir_off = (uint64_t)k * p.slot, dir_cap = p.slot, cig_off = x * (uint64_t)p.cigar_stride;
  w.cig_cap = p.cigar ? p.cigar_stride : 0u;
  if (p.plan) {
    dir_off = p.plan[h].dir_off;
    dir_cap = p.plan[h].dir_cap;
    w.cig_cap = p.cigar ? p.plan[h].cig_cap : 0u;
    cig_off = p.plan[h].cig_off + (uint64_t)a.round * w.cig_cap;
  }
  uint64_t need = 0;
  for (uint32_t f = 0; f < (uint32_t)PL::N; ++f) need += gl_dir_dwords(K, w.m, PL::cols(w.L, f));
  w.over = w.m == 0 || need > dir_cap;  // (the host sized the store)
  w.dirs = p.dirs + dir_off;
  w.cig = p.cigar + cig_off;
  return w;
}

// Where plane f's store begins in the hit's.
template <int K, class PL>
__device__ __forceinline__ uint64_t lf_plane_off(uint32_t m, uint32_t L, uint32_t f) {
  uint64_t off = 0;
  for (uint32_t g = 0; g < f; ++g) off += gl_dir_dwords(K, m, PL::cols(L, g));
  return off;
}

// One thread: the winner of the candidates in w.state, its path in its plane's store as
// lalign_round follows it, the record.  The winner's plane is kept in the state.
template <int K, class PL>
__device__ __forceinline__ void lf_record(const SwkLaAlign& p, const LfHit& w, const int8_t* prof,
                                          const uint8_t* tab, sw_alignment* out) {
  constexpr int ROWS = 64 * K;
  sw_alignment r = w.r;
  LaBest b{0, 0u, 0u};
  uint32_t win = 0;
  for (uint32_t f = 0; f < (uint32_t)PL::N; ++f) {  // the largest score, then the lowest plane
    const int32_t v = w.state[3 * f];
    if (v > b.v) {
      b = LaBest{v, (uint32_t)w.state[3 * f + 1], (uint32_t)w.state[3 * f + 2]};
      win = f;
    }
  }
  w.state[3 * PL::N] = (int32_t)win;
  if (b.v < p.min_score) {
    *out = r;
    return;
  }
  const typename PL::Code code = PL::code(w.tp, tab, w.L, win, p.alpha - 1);
  uint8_t* db = reinterpret_cast<uint8_t*>(w.dirs + lf_plane_off<K, PL>(w.m, w.L, win));
  uint32_t* cig = w.cig;
  const uint32_t cig_cap = w.cig_cap;
  const uint32_t ncols = PL::cols(w.L, win);
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
  for (uint64_t it = 0, lim = (uint64_t)w.m + ncols + 2; it < lim; ++it) {
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
      idn += w.qp[i] == tc;
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
  PL::place(r, win, w.L);
  *out = r;
}

// Round 0: wave f of the workgroup walks plane f.
template <int K, class PL>
__global__ void __launch_bounds__(64 * PL::N) laframes_first(const LfArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[GL_MAX_ALPHA * ROWS];
  __shared__ uint32_t tabw[16];
  __shared__ int32_t cand[3 * PL::N];
  const SwkLaAlign& p = a.p;
  const uint32_t tid = threadIdx.x;
  const LfHit w = lf_hit<K, PL>(a);
  sw_alignment* out = static_cast<sw_alignment*>(p.out) + (a.h0 + blockIdx.x) * p.rounds;
  if (!w.pair || w.over) {  // (the same in every thread of the workgroup)
    if (tid == 0) *out = w.r;
    return;
  }
  gl_profile<K>(p.mat, p.alpha, prof, w.qp, w.m, 64 * PL::N);
  if (tid < 16) tabw[tid] = a.table.w[tid];
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  const uint32_t f = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t n = PL::cols(w.L, f);
  LaBest b{0, 0u, 0u};  // a plane without columns
  if (n) {
    const typename PL::Code code = PL::code(w.tp, tab, w.L, f, p.alpha - 1);
    b = la_walk<K, true>(prof, code, n, w.m, p.o, p.e,
                         w.dirs + lf_plane_off<K, PL>(w.m, w.L, f));
  }
  if ((tid & 63) == 0) {
    cand[3 * f] = b.v;
    cand[3 * f + 1] = (int32_t)b.j;
    cand[3 * f + 2] = (int32_t)b.i;
  }
  __threadfence();  // thread 0 reads what the other threads stored
  __syncthreads();
  if (tid != 0) return;
  for (int y = 0; y < 3 * PL::N; ++y) w.state[y] = cand[y];
  lf_record<K, PL>(p, w, prof, tab, out);
}

// Round r > 0: one wave walks the previous record's plane again.
template <int K, class PL>
__global__ void __launch_bounds__(64) laframes_next(const LfArgs a) {
  constexpr int ROWS = 64 * K;
  __shared__ __attribute__((aligned(16))) int8_t prof[GL_MAX_ALPHA * ROWS];
  __shared__ uint32_t tabw[16];
  const SwkLaAlign& p = a.p;
  const uint32_t tid = threadIdx.x;
  const LfHit w = lf_hit<K, PL>(a);
  sw_alignment* out =
      static_cast<sw_alignment*>(p.out) + (a.h0 + blockIdx.x) * p.rounds + a.round;
  // (a hit whose store was too small has an empty record 0)
  if (!w.pair || w.over || (out[-1].flags & (uint32_t)SW_ALIGN_EMPTY) != 0) {
    if (tid == 0) *out = w.r;
    return;
  }
  gl_profile<K>(p.mat, p.alpha, prof, w.qp, w.m, 64);
  if (tid < 16) tabw[tid] = a.table.w[tid];
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tabw);
  // (the previous record is not empty: its plane has columns)
  const uint32_t f =
      __builtin_amdgcn_readfirstlane(min((uint32_t)w.state[3 * PL::N], (uint32_t)PL::N - 1));
  const uint32_t n = PL::cols(w.L, f);
  LaBest b{0, 0u, 0u};
  if (n) {
    const typename PL::Code code = PL::code(w.tp, tab, w.L, f, p.alpha - 1);
    b = la_walk<K, false>(prof, code, n, w.m, p.o, p.e,
                          w.dirs + lf_plane_off<K, PL>(w.m, w.L, f));
  }
  __threadfence();  // lane 0 reads what the other lanes stored
  __syncthreads();
  if (tid != 0) return;
  w.state[3 * f] = b.v;
  w.state[3 * f + 1] = (int32_t)b.j;
  w.state[3 * f + 2] = (int32_t)b.i;
  lf_record<K, PL>(p, w, prof, tab, out);
}

static bool lf_args_ok(const SwkLaFrames* f) {
  const SwkLaAlign* p = f ? &f->a : nullptr;
  return p && f->state && p->res && p->offs && p->lens && p->qtab && p->mat && p->query &&
         p->out && p->dirs && p->n && p->nq && p->qlen && p->qlen <= 1024 && p->alpha &&
         p->alpha <= (uint32_t)GL_MAX_ALPHA &&
         (p->hit_queries != nullptr) != (p->hits_per_query != 0) && p->rounds >= 1 &&
         p->rounds <= 64 && p->min_score >= 1 && p->n_hits <= 0xFFFFFFFFull && p->o <= 0 &&
         p->e <= 0 && p->o >= -65534 && p->e >= -32767;
}

template <int K>
static void lf_launch(const LfArgs& a, dim3 grid, hipStream_t st) {
  if (a.round == 0)
    hipLaunchKernelGGL((laframes_first<K, FramePlanes>), grid, dim3(64 * FramePlanes::N), 0, st,
                       a);
  else
    hipLaunchKernelGGL((laframes_next<K, FramePlanes>), grid, dim3(64), 0, st, a);
}
}  // namespace swk

extern "C" uint64_t swk_laframes_dir_dwords(uint32_t qlen, uint32_t rows, uint32_t len) {
  uint64_t need = 0;
  for (uint32_t o = 0; o < 3; ++o)  // (frames f and f + 3 hold the same number of codons)
    need += 2 * swk::gl_dir_dwords(swk::gl_rows(qlen), rows, len >= o + 3 ? (len - o) / 3 : 0u);
  return need;
}

extern "C" hipError_t swk_launch_laframes_round(const SwkLaFrames* p, size_t h0, size_t count,
                                                uint32_t round, hipStream_t st) {
  using namespace swk;
  if (!p || count == 0) return hipSuccess;
  if (!lf_args_ok(p) || round >= p->a.rounds || h0 + count > p->a.n_hits ||
      count > ((size_t)1 << 30))
    return hipErrorInvalidValue;
  LfArgs a{p->a, LfTable{}, p->state, h0, round};
  for (int i = 0; i < 16; ++i)
    a.table.w[i] = (uint32_t)p->table[4 * i] | (uint32_t)p->table[4 * i + 1] << 8 |
                   (uint32_t)p->table[4 * i + 2] << 16 | (uint32_t)p->table[4 * i + 3] << 24;
  const dim3 grid((unsigned)count);
  switch (gl_rows(p->a.qlen)) {
    case 4: lf_launch<4>(a, grid, st); break;
    case 8: lf_launch<8>(a, grid, st); break;
    default: lf_launch<16>(a, grid, st); break;
  }
  return hipGetLastError();
}
