// Query-table check (swbank_qtab.h, the code prepare*() run), two ways per case of qtab_cases.h:
//  a. read-back: every table is decoded by the layouts DESIGN.md §4.1 states (the decoder below
//     calls no builder) and every entry compared with m[q[row] * A + letter] as that table stores
//     it; rows past the query and the padding letter must hold the padding; the pair-table
//     strides must spread the slots over the LDS bank groups and no two slots may overlap;
//  b. byte equality: FNV-1a 64 of the tables in upload order (the staging buffer's content), the
//     byte count, the scalars the bank stores and every refusal's status and text against
//     tests/golden/qtab_digests.tsv, recorded from the library before the builders moved here.
//     The file also records the two swk_has_variant answers, which the analysis is fed.
// usage: qtab_check tests/golden/qtab_digests.tsv
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>

#include "qtab_cases.h"

using qtab::f16_score_bits;
typedef std::vector<uint32_t> Words;

static int g_bad = 0;
static std::string g_case;
#define EXPECT(cond, ...)                                \
  do {                                                   \
    if (!(cond)) {                                       \
      if (++g_bad <= 20) {                               \
        fprintf(stderr, "%s: ", g_case.c_str());         \
        fprintf(stderr, __VA_ARGS__);                    \
        fprintf(stderr, "\n");                           \
      }                                                  \
    }                                                    \
  } while (0)

struct Golden {
  int status, hu, hf;
  size_t nbytes;
  std::string digest, text;
};

static std::string fmt(const char* f, ...) {
  char t[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(t, sizeof(t), f, ap);
  va_end(ap);
  return t;
}

static void fnv(uint64_t& h, const void* p, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    h ^= static_cast<const uint8_t*>(p)[i];
    h *= 0x100000001b3ull;
  }
}
template <class T>
static void fnv(uint64_t& h, size_t& bytes, const std::vector<T>& v) {
  fnv(h, v.data(), v.size() * sizeof(T));
  bytes += v.size() * sizeof(T);
}

static void compare(const std::map<std::string, Golden>& gold, const std::string& fn, int status,
                    size_t nbytes, uint64_t h, const std::string& text) {
  const auto it = gold.find(g_case + "\t" + fn);
  EXPECT(it != gold.end(), "%s: no golden line", fn.c_str());
  if (it == gold.end()) return;
  const Golden& g = it->second;
  EXPECT(g.status == status, "%s: status %d, golden %d", fn.c_str(), status, g.status);
  EXPECT(g.text == text, "%s: '%s', golden '%s'", fn.c_str(), text.c_str(), g.text.c_str());
  if (status != SW_OK) return;
  EXPECT(g.nbytes == nbytes, "%s: %zu bytes, golden %zu", fn.c_str(), nbytes, g.nbytes);
  const std::string d = fmt("%016llx", (unsigned long long)h);
  EXPECT(g.digest == d, "%s: digest %s, golden %s", fn.c_str(), d.c_str(), g.digest.c_str());
}

// ---- the decoder: the expected entry of (row, letter) as each table stores it -----------------
struct Ctx {
  const int8_t* m;
  int A, S;
};
static int score(const Ctx& c, const std::vector<uint8_t>& q, int row, int letter) {
  return c.m[q[(size_t)row] * c.A + letter];
}
static uint8_t byte_at(const Words& t, size_t byte) { return (uint8_t)(t[byte / 4] >> (8 * (byte % 4))); }
static uint16_t half_at(const Words& t, size_t byte) {
  return (uint16_t)(byte_at(t, byte) | byte_at(t, byte + 1) << 8);
}

// kind 0: S - s as a byte (pad 0xFF); 1: f16 high byte (pad 0xBC); 2: f16 bits (pad 0xBC00)
static uint32_t stored(const Ctx& c, int kind, int s) {
  return kind == 0 ? (uint32_t)(uint8_t)(c.S - s)
                   : kind == 1 ? (uint32_t)(f16_score_bits(s) >> 8) : (uint32_t)f16_score_bits(s);
}
static uint32_t padding(int kind) { return kind == 0 ? 0xFFu : kind == 1 ? 0xBCu : 0xBC00u; }

// One table of rows [r0, r0 + nrows) at word `off`: row words (LUT) or a profile of `stride`
// entries per letter; rows at or past `limit` rows of the table, or past the query, are padding.
static void check_rows(const char* what, const Ctx& c, bool prof, int kind, const Words& t,
                       size_t off, const std::vector<uint8_t>& q, int r0, int nrows, size_t stride) {
  const int qlen = (int)q.size();
  if (!prof) {
    EXPECT(off + (size_t)nrows <= t.size(), "%s: table too short", what);
    for (int i = 0; i < nrows; ++i)
      for (int l = 0; l < 4; ++l) {
        const uint32_t want = r0 + i < qlen ? stored(c, kind, score(c, q, r0 + i, l)) : padding(kind);
        const uint32_t got = byte_at(t, (off + i) * 4 + l);
        EXPECT(got == want, "%s: row %d letter %d holds %02x, want %02x", what, r0 + i, l, got, want);
      }
    return;
  }
  const size_t eb = kind == 2 ? 2 : 1;
  EXPECT(off * 4 + (size_t)(c.A + 1) * stride * eb <= t.size() * 4, "%s: table too short", what);
  for (int l = 0; l <= c.A; ++l)
    for (size_t i = 0; i < stride; ++i) {
      const bool real = l < c.A && (int)i < nrows && r0 + (int)i < qlen;
      const uint32_t want = real ? stored(c, kind, score(c, q, r0 + (int)i, l)) : padding(kind);
      const size_t at = off * 4 + ((size_t)l * stride + i) * eb;
      const uint32_t got = eb == 2 ? half_at(t, at) : byte_at(t, at);
      EXPECT(got == want, "%s: row %d letter %d holds %04x, want %04x", what, r0 + (int)i, l, got, want);
    }
}

// A letter-pair table of rows [r0, r0 + NR) at word `off`: slot (x, y) at byte 16 + x pS1 + y pS2,
// word k = rows r0 + k + 1 of letters {x, y} (f16 halves), the row-r0 word 4 bytes before the slot.
// A row holds s + add, and add0 on top when it is the first of an 8-row block; rows past the
// query `pad` in place of s.
static void check_pair(const char* what, const Ctx& c, const Words& t, size_t off, size_t words,
                       const std::vector<uint8_t>& q, int r0, uint32_t NR, uint32_t pS1,
                       uint32_t pS2, int add, int pad, int add0) {
  EXPECT((pS2 / 16) % 16 == 1 && pS2 % 16 == 0, "%s: pS2 %u", what, pS2);
  EXPECT((pS1 / 16) % 16 == 4 && pS1 % 16 == 0, "%s: pS1 %u", what, pS1);
  std::vector<std::pair<size_t, size_t>> spans;  // [first, last) byte of every slot
  for (int x = 0; x < c.A; ++x)
    for (int y = 0; y < c.A; ++y) {
      const size_t slot = 16 + (size_t)x * pS1 + (size_t)y * pS2;
      spans.push_back({slot - 4, slot + 4 * ((size_t)NR - 1)});
      EXPECT(spans.back().second <= words * 4, "%s: slot (%d, %d) ends past the table", what, x, y);
      if (spans.back().second > words * 4) return;
      for (uint32_t r = 0; r < NR; ++r) {
        const size_t at = off * 4 + slot + 4 * (size_t)r - 4;  // row r0 + r
        const int ad = add + (r % 8 == 0 ? add0 : 0);
        const bool real = r0 + (int)r < (int)q.size();
        const uint16_t lo = f16_score_bits((real ? score(c, q, r0 + (int)r, x) : pad) + ad);
        const uint16_t hi = f16_score_bits((real ? score(c, q, r0 + (int)r, y) : pad) + ad);
        EXPECT(half_at(t, at) == lo && half_at(t, at + 2) == hi,
               "%s: row %d letters (%d, %d) hold %04x %04x, want %04x %04x", what, r0 + (int)r, x, y,
               half_at(t, at), half_at(t, at + 2), lo, hi);
      }
    }
  for (size_t i = 0; i < spans.size(); ++i)
    for (size_t j = 0; j < i; ++j)
      EXPECT(spans[i].second <= spans[j].first || spans[j].second <= spans[i].first,
             "%s: slots %zu and %zu overlap", what, i, j);
}

static void check_query_tables(const Ctx& c, const qtab::Plan& p, const qtab::QueryTables& t,
                               const std::vector<uint8_t>& q) {
  const int k16 = p.prof ? 2 : 1;
  for (size_t g = 0; g < t.segs.size(); ++g) {
    const int r0 = (int)g * p.seg_rows, nrows = t.segs[g].W * p.R;
    check_rows("tab", c, p.prof, 0, t.tab, t.segs[g].off, q, r0, nrows, p.PS);
    if (p.f16) check_rows("tab16", c, p.prof, k16, t.tab16, t.segs[g].off16, q, r0, nrows, p.PS16 / 2);
  }
  EXPECT(p.f16 || t.tab16.empty(), "tab16 without f16");
  if (p.prof) {
    EXPECT(p.PS % 256 == 16 && (int)p.PS >= p.Wseg * p.R, "PS %u", p.PS);
    EXPECT(!p.f16 || (p.PS16 % 256 == 16 && (int)p.PS16 >= 2 * p.Wseg * p.R), "PS16 %u", p.PS16);
    EXPECT(p.pad == (uint32_t)c.A, "pad %u", p.pad);
  } else {  // the N word: letters 4..7 share one entry
    EXPECT(p.pad == 4 && p.nv == stored(c, 0, c.m[4]) * 0x01010101u, "nv %08x", p.nv);
    EXPECT(!p.f16 || p.nv16 == stored(c, 1, c.m[4]) * 0x01010101u, "nv16 %08x", p.nv16);
  }
  const uint32_t NR = (uint32_t)t.segs[0].W * p.R;
  if (!t.tpair.empty()) {
    EXPECT(t.tpair.size() == t.pair_words * t.segs.size(), "tpair size");
    for (size_t g = 0; g < t.segs.size(); ++g)
      check_pair("tpair", c, t.tpair, g * t.pair_words, t.pair_words, q, (int)g * p.seg_rows, NR,
                 t.pS1, t.pS2, 0, -2048, 0);
  }
  if (!t.tskew.empty()) {
    const int spad = -std::min(2048 - 2 * p.e, c.S * std::max((int)q.size(), 1));
    check_pair("tskew", c, t.tskew, 0, t.tskew.size(), q, 0, NR, t.pS1, t.pS2, 2 * p.e, spad,
               -8 * p.e);
    EXPECT(t.tfloor.size() == 2048 + 32, "tfloor size");
    for (size_t k = 0; k < t.tfloor.size(); ++k)
      EXPECT(t.tfloor[k] == f16_score_bits(std::min(2048, p.e * ((int)k - 3))) * 0x10001u,
             "tfloor[%zu]", k);
  }
  // wave tables: 64 K rows per segment; the split tails: P = 2 << i segments of 64 sK rows
  struct Wave { const char* name; const Words *t8, *t16; int rows, nsegs; };
  const Wave waves[4] = {{"wt", &t.wt, &t.wt16, 64 * p.wK, p.wsegs},
                         {"st0", &t.st[0], &t.st16[0], 64 * p.sK[0], 2},
                         {"st1", &t.st[1], &t.st16[1], 64 * p.sK[1], 4},
                         {"st2", &t.st[2], &t.st16[2], 64 * p.sK[2], 8}};
  for (const Wave& w : waves) {
    if (w.rows == 0) {
      EXPECT(w.t8->empty() && w.t16->empty(), "%s: tables without a split", w.name);
      continue;
    }
    EXPECT(w.rows * w.nsegs >= (int)q.size(), "%s: %d x %d rows", w.name, w.nsegs, w.rows);
    EXPECT(w.t8->size() % w.nsegs == 0 && (p.f16 ? w.t16->size() % w.nsegs == 0 : w.t16->empty()),
           "%s: sizes", w.name);
    for (int g = 0; g < w.nsegs; ++g) {
      check_rows(w.name, c, p.prof, 0, *w.t8, g * (w.t8->size() / w.nsegs), q, g * w.rows, w.rows,
                 w.rows);
      if (p.f16)
        check_rows(w.name, c, p.prof, k16, *w.t16, g * (w.t16->size() / w.nsegs), q, g * w.rows,
                   w.rows, w.rows);
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::map<std::string, Golden> gold;
  {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty() || line[0] == '#') continue;
      std::vector<std::string> f;
      std::stringstream ss(line);
      for (std::string x; std::getline(ss, x, '\t');) f.push_back(x);
      if (f.size() < 7) {
        fprintf(stderr, "bad golden line: %s\n", line.c_str());
        return 2;
      }
      gold[f[0] + "\t" + f[1]] = {atoi(f[2].c_str()), atoi(f[3].c_str()), atoi(f[4].c_str()),
                                  (size_t)atoll(f[5].c_str()), f[6], f.size() > 7 ? f[7] : ""};
    }
  }
  size_t lines = 0, ncases = 0;
  for (const qcase::Case& cs : qcase::cases()) {
    g_case = cs.name;
    ++ncases;
    const std::vector<int8_t> m = qcase::matrix(cs);
    std::vector<std::vector<uint8_t>> qset;
    for (size_t i = 0; i < cs.qlens.size(); ++i) qset.push_back(qcase::query(cs, i));
    size_t longest = 0;
    for (size_t i = 0; i < qset.size(); ++i)
      if (qset[i].size() > qset[longest].size()) longest = i;
    const std::vector<uint8_t>& q = qset[longest];
    const auto g0 = gold.find(g_case + "\tprepare");
    EXPECT(g0 != gold.end(), "no golden prepare line");
    if (g0 == gold.end()) continue;
    const int A = cs.protein ? SW_PROTEIN_ALPHA : SW_DNA_ALPHA;
    const qtab::Plan p = qtab::analyse(
        m.data(), A, cs.gotoh, cs.open, cs.extend, (int)q.size(), cs.opt,
        [&](const qtab::Plan&, int f16) { return (f16 ? g0->second.hf : g0->second.hu) != 0; });
    ++lines;
    if (p.status != SW_OK) {
      compare(gold, "prepare", p.status, 0, 0, p.msg);
      continue;
    }
    const qtab::QueryTables t = qtab::build_query(p, m.data(), q.data());
    const Ctx c{m.data(), A, p.S};
    check_query_tables(c, p, t, q);
    {
      uint64_t h = 0xcbf29ce484222325ull;
      size_t nb = 0;
      fnv(h, nb, t.wt16);
      fnv(h, nb, t.wt);
      for (int i = 0; i < 3; ++i) {
        fnv(h, nb, t.st16[i]);
        fnv(h, nb, t.st[i]);
      }
      fnv(h, nb, t.tab);
      fnv(h, nb, t.tab16);
      fnv(h, nb, t.tpair);
      fnv(h, nb, t.tskew);
      fnv(h, nb, t.tfloor);
      std::string s = fmt(
          "R=%d RB=%d W=%d col0=%d prof=%d S=%u O=%u E=%u nv=%08x PS=%u pad=%u smax=%d f16=%d "
          "nv16=%08x PS16=%u f16_neg=%d pair_bytes=%u pS1=%u pS2=%u skew_entries=%u skew_neg=%d "
          "wK=%d wsegs=%d wseg_words=%zu/%zu wPS=%u/%u",
          p.R, p.RB, t.segs[0].W, p.col0, p.prof, (uint32_t)p.S, (uint32_t)p.o, (uint32_t)p.e, p.nv,
          p.PS, p.pad, p.smax, (int)p.f16, p.nv16, p.PS16, p.f16_neg, t.pair_words * 4, t.pS1,
          t.pS2, (uint32_t)t.tfloor.size(), t.skew_neg, p.wK, p.wsegs, t.wt.size() / p.wsegs,
          t.wt16.size() / p.wsegs, p.prof ? 64u * p.wK : 0u, p.prof ? 128u * p.wK : 0u);
      for (int i = 0; i < 3; ++i)
        s += fmt(" s%d=%d,%zu,%zu,%u,%u", i, p.sK[i], t.st[i].size() / (2 << i),
                 t.st16[i].size() / (2 << i), p.prof ? 64u * p.sK[i] : 0u,
                 p.prof ? 128u * p.sK[i] : 0u);
      s += " segs=";
      for (const qtab::Seg& sg : t.segs) s += fmt("%d:%zu:%zu;", sg.W, sg.off, sg.off16);
      compare(gold, "prepare", SW_OK, nb, h, s);
    }
    if (qset.size() > 1) {  // the set's tables: query i at i * words in the longest one's layout
      const qtab::SetTables st = qtab::build_set(p, t.segs, m.data(), qset, cs.opt);
      EXPECT(st.words == t.tab.size(), "set words %zu", st.words);
      for (size_t i = 0; i < qset.size(); ++i)
        for (size_t g = 0; g < t.segs.size(); ++g) {
          const int r0 = (int)g * p.seg_rows, nrows = t.segs[g].W * p.R;
          check_rows("t8", c, false, 0, st.t8, i * st.words + t.segs[g].off, qset[i], r0, nrows, 0);
          if (p.f16)
            check_rows("t16", c, false, 1, st.t16, i * st.words + t.segs[g].off, qset[i], r0, nrows, 0);
        }
      EXPECT(st.tp.size() == st.pair_words * st.pair_segs * qset.size(), "set pair tables' size");
      EXPECT((st.pair_segs != 0) == (cs.opt.mq_pair != 0), "set pair tables: %d segments", st.pair_segs);
      for (int g = 0; g < st.pair_segs; ++g)  // [segment][query]
        for (size_t i = 0; i < qset.size(); ++i)
          check_pair("tp", c, st.tp, (g * qset.size() + i) * st.pair_words, st.pair_words, qset[i],
                     g * st.pair_rows, (uint32_t)st.pair_rows, st.pS1, st.pS2, 0, -2048, 0);
      uint64_t h = 0xcbf29ce484222325ull;
      size_t nb = 0;
      fnv(h, nb, st.t8);
      fnv(h, nb, st.t16);
      fnv(h, nb, st.tp);
      std::string s = fmt("mq_words=%zu pair_segs=%d", st.words, st.pair_segs);
      if (st.pair_segs > 0)
        s += fmt(" pair_words=%zu pair_rows=%d pS1=%u pS2=%u", st.pair_words, st.pair_rows, st.pS1,
                 st.pS2);
      compare(gold, "prepare_multi", SW_OK, nb, h, s);
      ++lines;
    }
    {  // int32 strips: [strip][letter 0..pad][lane][k] int16, row = 256 strip + 4 lane + k
      uint32_t strips = 0;
      const std::vector<int16_t> h16 =
          qtab::build_i32(m.data(), A, p.S, p.pad, q.data(), (uint32_t)q.size(), strips);
      EXPECT(strips == std::max<size_t>(1, (q.size() + 255) / 256), "strips %u", strips);
      EXPECT(h16.size() == (size_t)strips * (p.pad + 1) * 256, "i32 size");
      for (size_t x = 0; x < h16.size(); ++x) {
        const size_t k = x % 4, lane = x / 4 % 64, letter = x / 256 % (p.pad + 1);
        const size_t row = x / 256 / (p.pad + 1) * 256 + 4 * lane + k;
        const int want = row >= q.size() ? 0 : (int)letter < A ? score(c, q, (int)row, (int)letter)
                                                                : p.S - 255;
        EXPECT(h16[x] == want, "i32 row %zu letter %zu holds %d, want %d", row, letter, h16[x], want);
      }
      uint64_t h = 0xcbf29ce484222325ull;
      size_t nb = 0;
      fnv(h, nb, h16);
      compare(gold, "prepare_i32", SW_OK, nb, h, fmt("strips=%u", strips));
      ++lines;
    }
    {  // alignment table: {offset, length} per query, the matrix, the codes back to back
      const std::vector<uint8_t> at = qtab::build_align(m, qset.data(), qset.size());
      size_t off = 0;
      const size_t nq = qset.size(), codes = nq * 8 + m.size();
      for (size_t i = 0; i < nq; ++i) {
        uint32_t e[2];
        memcpy(e, at.data() + 8 * i, 8);
        EXPECT(e[0] == off && e[1] == qset[i].size(), "align entry %zu: {%u, %u}", i, e[0], e[1]);
        EXPECT(codes + off + qset[i].size() <= at.size() &&
                   memcmp(at.data() + codes + off, qset[i].data(), qset[i].size()) == 0,
               "align codes of query %zu", i);
        off += qset[i].size();
      }
      EXPECT(at.size() == codes + off && memcmp(at.data() + nq * 8, m.data(), m.size()) == 0,
             "align matrix / size");
      uint64_t h = 0xcbf29ce484222325ull;
      size_t nb = 0;
      fnv(h, nb, at);
      compare(gold, "prepare_align", SW_OK, nb, h, fmt("nq=%zu", nq));
      ++lines;
    }
  }
  EXPECT(lines == gold.size(), "%zu lines checked, the golden file holds %zu", lines, gold.size());
  if (g_bad) {
    fprintf(stderr, "%d mismatches\n", g_bad);
    return 1;
  }
  printf("qtab ok (%zu cases, %zu digests)\n", ncases, lines);
  return 0;
}
