// swbank_qtab.h — the query tables, built on the host (internal, header-inline, no HIP): what
// prepare(), prepare_multi(), prepare_i32() and prepare_align() (swbank_bank.hip,
// swbank_align.hip) upload.  Plain C++17 for a compiler with _Float16 (the ROCm host clang), so
// tests/c/qtab_check.cc compiles the code libswbank.so runs.  DESIGN.md §4.1 lists every table's
// layout and padding in one place.
//
//   analyse()       scoring scheme + query length + options -> Plan (every derived scalar) or a
//                   refusal (status and text)
//   build_query()   Plan + query -> QueryTables (tile segments, pair / skewed tables, wave tables)
//   build_set()     Plan + segments + query set -> SetTables
//   build_i32(), build_align()   the int32 strip profile, the alignment unit's table
#ifndef SWBANK_QTAB_H
#define SWBANK_QTAB_H

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "swbank.h"

namespace qtab {

// Scores in the f16 kernels are f16 multiples of 2^-11 (x as x/2048, swbank_kcommon.h), so
// the packed add's [0, 1] clamp is max(0, x); -2048 (padding rows / letters) is 0xBC00.
inline uint16_t f16_score_bits(int v) {
  return __builtin_bit_cast(uint16_t, (_Float16)((float)v * (1.0f / 2048.0f)));
}

// How a table stores the score s: S - s as a byte (rows past the query and the padding letter
// 0xFF), the high byte of its f16 bits (0xBC: -2048; exact only for scores whose low byte is 0),
// or the f16 bits as two bytes (0xBC00).
enum class Entry { U8, F16Hi, F16 };
inline size_t entry_bytes(Entry k) { return k == Entry::F16 ? 2 : 1; }
inline uint32_t entry_pad(Entry k) { return k == Entry::U8 ? 0xFFu : k == Entry::F16Hi ? 0xBCu : 0xBC00u; }
inline uint32_t entry_of(Entry k, int S, int s) {
  return k == Entry::U8 ? (uint32_t)(uint8_t)(S - s)
                        : k == Entry::F16Hi ? (uint32_t)(f16_score_bits(s) >> 8) : f16_score_bits(s);
}

// The tuning knobs (the SWBANK_* environment variables of the same names, read by the callers in
// swbank_bank.hip only); 0 in R, RB, seg: the rule's own value.
struct Options {
  int profile = 0, R = 0, RB = 0, seg = 0, f16 = 1, mq_pair = 1, mq_pair_rows = 128;
};

struct Seg { int W; size_t off, off16; };  // rows = W*R (last may be shorter); word offsets
                                            // in qtab and qtab16

// What analyse() derives from (matrix, gap model, penalties, query length, options).
struct Plan {
  sw_status status = SW_OK;
  char msg[160] = {0};  // the refusal's text
  int A = 0, qlen = 0, o = 0, e = 0;
  bool gotoh = false;
  int S = 0, smin = 0, smax = 0, sN = 0;
  bool lut = false, f16 = false, f16_range = false, u16_only = false;
  int prof = 0, col0 = 0, R = 32, RB = 4, seg_rows = 0, Wseg = 1;
  uint32_t PS = 0, PS16 = 0, pad = 4, nv = 0, nv16 = 0;
  int32_t f16_neg = 0;
  int wK = 0, wsegs = 1, sK[3] = {0, 0, 0};  // wave kernel: rows per lane, segments, split tail
};

// Profile row stride for `bytes` of rows: a multiple of 16 B that is 16 mod 256, so the 16-B
// reads of lanes holding different letters fall in different LDS banks (a stride of 0 mod 256
// puts every letter row on the same 4 banks).
inline uint32_t stride16mod256(uint32_t bytes) {
  const uint32_t s = (bytes + 15) / 16 * 16;
  return s + (16u + 256u - s % 256u) % 256u;
}

template <class... T>
inline Plan& refuse(Plan& p, sw_status st, const char* fmt, T... a) {
  p.status = st;
  snprintf(p.msg, sizeof(p.msg), fmt, a...);
  return p;
}

// has_variant(p, f16): whether the tile kernel exists for (p.R, p.RB, p.col0, p.prof, p.gotoh) in
// u16 (0) or f16 (1) -- swk_has_variant, which lives in a kernel unit.
template <class HasVariant>
inline Plan analyse(const int8_t* m, int A, bool gotoh, int gap_open, int gap_extend, int qlen,
                    const Options& opt, HasVariant&& has_variant) {
  Plan p;
  p.A = A;
  p.qlen = qlen;
  p.gotoh = gotoh;
  p.smax = -128;
  p.smin = 127;
  for (int i = 0; i < A * A; ++i) {
    p.smax = std::max<int>(p.smax, m[i]);
    p.smin = std::min<int>(p.smin, m[i]);
  }
  const int S = p.S = std::max(0, p.smax);
  if (S - p.smin > 254)
    return refuse(p, SW_ERR_RANGE, "substitution range [%d, %d] exceeds 254", p.smin, p.smax);
  const int o = p.o = -gap_open, e = p.e = -gap_extend;
  if (gotoh && o + e + S > 65535) return refuse(p, SW_ERR_RANGE, "%s", "gap penalties too large");

  // LUT mode needs a DNA matrix whose N column (codes 4..7 share one word) is uniform and <= 0
  p.lut = A == SW_DNA_ALPHA;
  const int sN = p.sN = m[4];
  for (int i = 0; p.lut && i < A; ++i) p.lut = m[i * A + 4] == sN;
  p.lut = p.lut && sN <= 0;
  // The f16 LUT holds one byte per entry (the f16 high byte): only scores whose f16 low byte
  // is 0 (|s| <= 8, or coarser even values) qualify.  Other DNA matrices run in profile mode
  // (2-byte f16 entries) when f16 applies at all: faster than the u16 LUT kernel.
  bool lut_f16 = true;
  for (int i = 0; i < A * A; ++i) lut_f16 = lut_f16 && (f16_score_bits(m[i]) & 0xFFu) == 0;
  p.f16_range = -(o + 2 * e + (S - p.smin)) >= -2048;
  p.prof = (opt.profile || !p.lut || (!lut_f16 && p.f16_range)) ? 1 : 0;

  // the HDL column-0 rule differs from the plain recurrence only if a match pays for a gap
  p.col0 = (!gotoh && p.smax > o + e) ? 1 : 0;
  // Rows per wave: 32 for the DNA LUT kernels (merged and Gotoh: the Gotoh f16 column with
  // the letter-pair table runs 8.3-8.6 TCUPS at R = 32 against 7.8-8.2 at R = 16, and a
  // 512-row query fits one workgroup); 16 for tiny queries and for the profile / column-0
  // variants, whose 32-row columns do not fit 128 VGPRs (the occupancy-4 budget) without
  // spilling.  Queries longer than one workgroup (16 waves) run
  // as segments of opt.seg rows (default: a full 16-wave workgroup, 16·R rows), each
  // segment's bottom row handed to the next through HBM.  opt.R / RB / seg override (tuning only).
  // u16 Gotoh keeps R = 16 when no f16 pass can run (its 32-row column spills past 128 VGPRs);
  // u16 passes that follow an f16 pass (optimistic re-scores) are rare and use the f16 layout
  p.u16_only = gotoh && (!p.f16_range || opt.f16 == 0);
  const int R = p.R = opt.R ? opt.R : (qlen <= 16 || p.prof || p.col0 || p.u16_only) ? 16 : 32;
  p.RB = opt.RB ? opt.RB : 4;
  const int max_rows = (R >= 64 ? 8 : 16) * R;
  p.seg_rows = qlen > max_rows ? (opt.seg ? opt.seg : max_rows) : std::max(qlen, 1);
  if (p.seg_rows % R != 0 && p.seg_rows < qlen)
    return refuse(p, SW_ERR_ARG, "segment rows %d not a multiple of R=%d", p.seg_rows, R);
  if (!has_variant(p, 0))
    return refuse(p, SW_ERR_UNSUPPORTED, "no kernel variant R=%d RB=%d col0=%d prof=%d gotoh=%d",
                  R, p.RB, p.col0, p.prof, (int)gotoh);
  p.Wseg = std::max(1, (p.seg_rows + R - 1) / R);
  if (p.Wseg * 64 > (R >= 64 ? 512 : 1024))
    return refuse(p, SW_ERR_UNSUPPORTED, "segment of %d rows too tall for one workgroup",
                  p.seg_rows);

  p.PS = p.prof ? stride16mod256((uint32_t)(p.Wseg * R)) : 0;
  p.pad = p.prof ? (uint32_t)A : 4u;  // profile letter A = padding row (all 0xFF)
  p.nv = p.prof ? 0u : entry_of(Entry::U8, S, sN) * 0x01010101u;
  // f16 variant of the LUT: each substitution score must be an f16 whose low byte is 0
  // (|s| <= 8 or a coarser even value), so the byte perm yields the exact f16 bits.
  // LUT mode: one byte per entry (the f16 high byte); profile mode: two bytes (any |s| <= 127
  // is an exact f16), row stride PS16 = 2 x rows, 16 mod 256 like PS
  auto hi_exact = [](int v) {
    const uint16_t bits = f16_score_bits(v);
    return (bits & 0xFFu) == 0 &&
           (int)((float)__builtin_bit_cast(_Float16, bits) * 2048.0f) == v;
  };
  p.f16 = has_variant(p, 1);
  if (p.f16 && !p.prof) {
    p.nv16 = entry_of(Entry::F16Hi, S, sN) * 0x01010101u;
    for (int i = 0; p.f16 && i < A * A; ++i) p.f16 = hi_exact(m[i]);
  }
  if (p.f16 && p.prof) p.PS16 = stride16mod256((uint32_t)(2 * p.Wseg * R));
  p.f16_neg = -(o + 2 * e + (S - p.smin));  // most negative intermediate
  // wave kernel: rows padded to 64K; queries past 1024 rows run as 1024-row segments (K = 16);
  // its split tail (one segment, K >= 8): the query as P = 2, 4 and 8 segments of K/P rows a lane
  p.wK = qlen <= 256 ? 4 : qlen <= 512 ? 8 : 16;
  p.wsegs = std::max(1, (qlen + 64 * p.wK - 1) / (64 * p.wK));
  for (int i = 0; i < 3; ++i) p.sK[i] = (p.wsegs == 1 && p.wK >= 8) ? p.wK / (2 << i) : 0;
  return p;
}

// Row words of query rows [r0, r0 + nrows): word i = the entries of letters 0..3 of row r0 + i,
// letter c in byte c; rows past the query hold the padding entry in every byte.
inline void row_words(Entry k, const uint8_t* q, int qlen, int r0, int nrows, const int8_t* m,
                      int A, int S, uint32_t* out) {
  for (int i = 0; i < nrows; ++i) {
    uint32_t w = entry_pad(k) * 0x01010101u;
    if (r0 + i < qlen) {
      w = 0;
      for (int c = 0; c < 4; ++c) w |= entry_of(k, S, m[q[r0 + i] * A + c]) << (8 * c);
    }
    out[i] = w;
  }
}

// Query profile of rows [r0, r0 + nrows): A + 1 letter rows of `stride` entries, entry i of
// letter c = row r0 + i against c; rows past the query and the whole letter A hold the padding.
template <class T>  // T: the entry's bytes, uint8_t or uint16_t
inline void profile_as(Entry k, const uint8_t* q, int qlen, int r0, int nrows, const int8_t* m,
                       int A, int S, size_t stride, uint32_t* out) {
  std::vector<T> qp((size_t)(A + 1) * stride, (T)entry_pad(k));
  for (int c = 0; c < A; ++c)
    for (int i = 0; i < nrows && r0 + i < qlen; ++i)
      qp[(size_t)c * stride + i] = (T)entry_of(k, S, m[q[r0 + i] * A + c]);
  std::memcpy(out, qp.data(), qp.size() * sizeof(T));
}
inline void profile(Entry k, const uint8_t* q, int qlen, int r0, int nrows, const int8_t* m, int A,
                    int S, size_t stride, uint32_t* out) {
  if (k == Entry::F16)
    profile_as<uint16_t>(k, q, qlen, r0, nrows, m, A, S, stride, out);
  else
    profile_as<uint8_t>(k, q, qlen, r0, nrows, m, A, S, stride, out);
}

// Appends the table of rows [r0, r0 + nrows) to `t` in the plan's mode: nrows row words (LUT) or
// a profile of `stride` entries per letter; returns the word offset it starts at.
inline size_t append_rows(const Plan& p, Entry k, const uint8_t* q, int qlen, int r0, int nrows,
                          size_t stride, const int8_t* m, std::vector<uint32_t>& t) {
  const size_t base = t.size();
  t.resize(base + (p.prof ? (size_t)(p.A + 1) * stride * entry_bytes(k) / 4 : (size_t)nrows));
  if (p.prof)
    profile(k, q, qlen, r0, nrows, m, p.A, p.S, stride, t.data() + base);
  else
    row_words(k, q, qlen, r0, nrows, m, p.A, p.S, t.data() + base);
  return base;
}

// Letter-pair table layout for NR rows: slot (a, b) at 16 + a*pS1 + b*pS2 (bytes), pS2/16 = 1 and
// pS1/16 = 4 (mod 16) so the 16 A/C/G/T slots sit on 16 different 4-bank LDS groups.
inline void pair_strides(uint32_t NR, uint32_t& pS1, uint32_t& pS2) {
  const uint32_t B = 4 * NR;
  pS2 = (B + 15) / 16 * 16;
  while ((pS2 / 16) % 16 != 1) pS2 += 16;
  pS1 = (4 * pS2 + B + 15) / 16 * 16;
  while ((pS1 / 16) % 16 != 4) pS1 += 16;
}

// The letter-pair table of query rows [r0, r0 + NR) (the PAIR tile kernel, DNA merged f16):
// slot (a, b) holds word k = {s(q_{r0+k+1}, a), s(q_{r0+k+1}, b)} (f16 halves; rows past the
// query -2048) and the row-r0 word 4 bytes before it.
// add / pad: the skewed rows' table holds s + add (add = 2e) and pad + add in rows past the query
// (the unskewed kernel's: s, -2048); add0: what the first row of every 8-row block holds on top
// (the skewed rows' -8e: the row above it sits 7 frames on), pad rows too.
inline std::vector<uint32_t> pair_table(const uint8_t* q, int qlen, int r0, uint32_t NR,
                                        const int8_t* m, int A, uint32_t pS1, uint32_t pS2,
                                        int add = 0, int pad = -2048, int add0 = 0) {
  const uint32_t bytes = 16 + 4 * pS1 + 4 * pS2 + 4 * NR;
  const uint32_t padw = (uint32_t)f16_score_bits(pad + add) * 0x10001u;
  std::vector<uint32_t> t(bytes / 4, padw);
  auto word = [&](int r, int x, int y) -> uint32_t {  // row r of the segment, letters x, y
    const int ad = add + (r % 8 == 0 ? add0 : 0);
    if (r0 + r >= qlen) return (uint32_t)f16_score_bits(pad + ad) * 0x10001u;
    const int c = q[r0 + r];
    return (uint32_t)f16_score_bits(m[c * A + x] + ad) |
           (uint32_t)f16_score_bits(m[c * A + y] + ad) << 16;
  };
  for (int x = 0; x < A; ++x)
    for (int y = 0; y < A; ++y) {
      const uint32_t base = (16 + x * pS1 + y * pS2) / 4;
      for (uint32_t k = 0; k + 1 < NR; ++k) t[base + k] = word((int)k + 1, x, y);
    }
  for (int x = 0; x < A; ++x)  // row-0 words last: they may reuse word NR-1 of a slot
    for (int y = 0; y < A; ++y) t[(16 + x * pS1 + y * pS2) / 4 - 1] = word(0, x, y);
  return t;
}

// The tables of one query, in the order prepare() uploads them: wt16, wt, (st16[i], st[i]) x 3,
// tab, tab16, tpair, tskew, tfloor.
struct QueryTables {
  std::vector<Seg> segs;
  std::vector<uint32_t> tab, tab16;  // tile segments: u16 (S - s bytes), f16
  // Letter-pair table for the PAIR tile kernel: DNA merged gaps, the f16 LUT kernel's R = 32, one
  // segment of at most 4 waves (the table's 25 slots then fit beside the ring at 4 workgroups per
  // CU); DNA Gotoh (R = 16 or 32): one table per query segment, each of the tallest segment's
  // rows (the Gotoh column is 7.5 VALU per 2 cells from the table against 8.5 with the row LUT).
  std::vector<uint32_t> tpair;
  uint32_t pS1 = 0, pS2 = 0, pair_words = 0;  // pair_words: one segment's table
  // The skewed rows of the merged pair kernel: the same table with s + 2e (the
  // first row of every 8-row block s + 2e - 8e), rows past the query with a score no H can lift
  // above 0 (H <= max(s) x rows; the same score in every row, so that skew_neg, and with it
  // launch()'s choice, is what it was before the frames restarted every 8 rows), and the floors
  // c_k = e (k - 1) of the frames k = (row mod 8) + column, word k + 2.  launch() takes them when
  // a batch's values fit f16 with the offsets.
  std::vector<uint32_t> tskew, tfloor;
  int32_t skew_neg = 0;
  // wave kernel: a table per 64K-row segment, concatenated; split tail [i]: P = 2 << i segments
  std::vector<uint32_t> wt, wt16, st[3], st16[3];
};

inline QueryTables build_query(const Plan& p, const int8_t* m, const uint8_t* q) {
  QueryTables t;
  const int A = p.A, R = p.R, qlen = p.qlen;
  const Entry k16 = p.prof ? Entry::F16 : Entry::F16Hi;
  // per segment: LUT words (W*R) or a query profile ((A+1) x PS bytes), concatenated
  for (int r0 = 0; r0 < std::max(qlen, 1); r0 += p.seg_rows) {
    const int rows = std::min(p.seg_rows, std::max(qlen, 1) - r0);
    const int W = std::max(1, (rows + R - 1) / R);
    Seg sg{W, 0, 0};
    sg.off = append_rows(p, Entry::U8, q, qlen, r0, W * R, p.PS, m, t.tab);
    if (p.f16) sg.off16 = append_rows(p, k16, q, qlen, r0, W * R, p.PS16 / 2, m, t.tab16);
    t.segs.push_back(sg);
  }
  if (p.f16 && !p.prof && !p.col0 && A == SW_DNA_ALPHA &&
      (p.gotoh ? R == 16 || R == 32 : R == 32 && t.segs.size() == 1 && t.segs[0].W <= 4)) {
    const uint32_t NR = (uint32_t)t.segs[0].W * R;
    pair_strides(NR, t.pS1, t.pS2);
    for (size_t sg = 0; sg < t.segs.size(); ++sg) {
      const std::vector<uint32_t> one =
          pair_table(q, qlen, (int)sg * p.seg_rows, NR, m, A, t.pS1, t.pS2);
      t.pair_words = (uint32_t)one.size();
      t.tpair.insert(t.tpair.end(), one.begin(), one.end());
    }
  }
  if (!t.tpair.empty() && !p.gotoh && 2 * p.e <= 2048) {
    const int e = p.e, spad = -std::min(2048 - 2 * e, p.S * std::max(qlen, 1));
    t.tskew = pair_table(q, qlen, 0, (uint32_t)t.segs[0].W * R, m, A, t.pS1, t.pS2, 2 * e, spad,
                         -8 * e);
    t.tfloor.resize(2048 + 32);
    for (size_t k = 0; k < t.tfloor.size(); ++k)
      t.tfloor[k] = (uint32_t)f16_score_bits(std::min(2048, e * ((int)k - 3))) * 0x10001u;
    // the most negative value that has to be exact: A - o of a block's first row in frame 0,
    // A = c_6 + min(s, pad) + 2e - 8e.  (The T~ of the row above, shifted into that frame, can
    // lie e lower; it is far below every floor and only ever enters a max)
    t.skew_neg = 5 * e + std::min(p.smin, spad) + 2 * e - 8 * e - p.o;
  }
  auto wave_tables = [&](int wrows, int nsegs, std::vector<uint32_t>& wt,
                         std::vector<uint32_t>& wt16) {
    for (int sg = 0; sg < nsegs; ++sg) {
      append_rows(p, Entry::U8, q, qlen, sg * wrows, wrows, wrows, m, wt);
      if (p.f16) append_rows(p, k16, q, qlen, sg * wrows, wrows, wrows, m, wt16);
    }
  };
  wave_tables(64 * p.wK, p.wsegs, t.wt, t.wt16);
  for (int i = 0; i < 3; ++i)
    if (p.sK[i]) wave_tables(64 * p.sK[i], 2 << i, t.st[i], t.st16[i]);
  return t;
}

// Row-LUT tables of every query of a set in the segment layout of the longest one: query i's
// words at i * words, rows past its end padding.  LUT mode only (DNA matrices without the
// column-0 rule).  Upload order: t8, t16, tp.
struct SetTables {
  size_t words = 0;  // per query
  std::vector<uint32_t> t8, t16;
  // letter-pair tables (DNA merged f16 without the column-0 rule), one per (segment, query):
  // 128-row segments (4 waves of 32 rows, 4-column chunks, 4 workgroups per CU whose wave
  // priorities rotate: a 1-kbp query is 8 segments, 7 bottom-row hand-offs through HBM; +11 %
  // against 512-row segments, one workgroup per CU) unless mq_pair_rows = 256
  // (8 waves, 2 workgroups per CU) or 512 (16 waves)
  std::vector<uint32_t> tp;
  size_t pair_words = 0;
  int pair_segs = 0, pair_rows = 0;
  uint32_t pS1 = 0, pS2 = 0;
};

inline SetTables build_set(const Plan& p, const std::vector<Seg>& segs, const int8_t* m,
                           const std::vector<std::vector<uint8_t>>& qset, const Options& opt) {
  SetTables t;
  const int R = p.R, seg_rows = segs[0].W * R;
  t.words = segs.back().off + (size_t)segs.back().W * R;
  t.t8.resize(qset.size() * t.words);
  if (p.f16) t.t16.resize(qset.size() * t.words);
  for (size_t i = 0; i < qset.size(); ++i)
    for (size_t sg = 0; sg < segs.size(); ++sg) {
      const size_t base = i * t.words + segs[sg].off;
      const int r0 = (int)sg * seg_rows, nr = segs[sg].W * R, ql = (int)qset[i].size();
      row_words(Entry::U8, qset[i].data(), ql, r0, nr, m, p.A, p.S, t.t8.data() + base);
      if (p.f16)
        row_words(Entry::F16Hi, qset[i].data(), ql, r0, nr, m, p.A, p.S, t.t16.data() + base);
    }
  if (p.f16 && !p.prof && !p.gotoh && !p.col0 && p.A == SW_DNA_ALPHA && opt.mq_pair != 0) {
    const uint32_t NR = opt.mq_pair_rows == 128 ? 128 : opt.mq_pair_rows == 256 ? 256 : 512;
    t.pair_rows = (int)NR;
    pair_strides(NR, t.pS1, t.pS2);
    t.pair_segs = std::max(1, (p.qlen + (int)NR - 1) / (int)NR);
    for (int sg = 0; sg < t.pair_segs; ++sg)
      for (const std::vector<uint8_t>& qi : qset) {
        const std::vector<uint32_t> one =
            pair_table(qi.data(), (int)qi.size(), sg * (int)NR, NR, m, p.A, t.pS1, t.pS2);
        t.pair_words = one.size();
        t.tp.insert(t.tp.end(), one.begin(), one.end());
      }
  }
  return t;
}

// The int32 re-score kernel's per-strip profile: [strip][letter 0..pad][lane] 4 x int16: rows
// 4l..4l+3 of a 256-row strip; letter = min(code, pad) as in the 16-bit kernels, the padding
// letter scoring S - 255 like their padding row; rows past the query 0.
inline std::vector<int16_t> build_i32(const int8_t* m, int A, int S, uint32_t pad, const uint8_t* q,
                                      uint32_t qlen, uint32_t& strips) {
  strips = std::max(1u, (qlen + 255) / 256);
  std::vector<int16_t> h((size_t)strips * (pad + 1) * 64 * 4, 0);
  for (uint32_t s = 0; s < strips; ++s)
    for (uint32_t c = 0; c <= pad; ++c)
      for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t k = 0; k < 4; ++k) {
          const uint32_t r = s * 256 + 4 * l + k;
          int v = 0;
          if (r < qlen) v = c < (uint32_t)A ? m[q[r] * A + c] : S - 255;
          h[(((size_t)s * (pad + 1) + c) * 64 + l) * 4 + k] = (int16_t)v;
        }
  return h;
}

// The alignment unit's table: an {offset, length} entry (2 x uint32) per query, the alpha x alpha
// matrix, then the codes of every query back to back (the offsets count from the first code).
inline std::vector<uint8_t> build_align(const std::vector<int8_t>& matrix,
                                        const std::vector<uint8_t>* queries, size_t nq) {
  size_t ql = 0;
  for (size_t i = 0; i < nq; ++i) ql += queries[i].size();
  std::vector<uint8_t> t(nq * 8 + matrix.size() + ql);
  uint8_t* codes = t.data() + nq * 8 + matrix.size();
  size_t at = 0;
  for (size_t i = 0; i < nq; ++i) {
    const uint32_t e[2] = {(uint32_t)at, (uint32_t)queries[i].size()};
    std::memcpy(t.data() + i * 8, e, 8);
    if (!queries[i].empty()) std::memcpy(codes + at, queries[i].data(), queries[i].size());
    at += queries[i].size();
  }
  if (!matrix.empty()) std::memcpy(t.data() + nq * 8, matrix.data(), matrix.size());
  return t;
}

}  // namespace qtab

#endif  // SWBANK_QTAB_H
