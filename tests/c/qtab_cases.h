// The cases of the query-table check (qtab_check.cc; tests/golden/qtab_digests.tsv holds one line
// per case and prepare function): the smallest queries at which each branch of the table
// construction is taken, and every refusal.  Queries come from a fixed generator, so the file
// that recorded the digests and the harness see the same codes.
#ifndef QTAB_CASES_H
#define QTAB_CASES_H

#include <cstdint>
#include <string>
#include <vector>

#include "swbank.h"
#include "swbank_qtab.h"

namespace qcase {

struct Case {
  std::string name;
  bool protein, gotoh;
  int match, mismatch;  // DNA: sw_fill_matrix; protein: BLOSUM62
  bool odd_n;           // DNA: one entry of the N column differs (no LUT mode)
  bool asym;            // DNA: s(a, b) = -2 for a < b (still LUT mode): a transposed index shows
  int open, extend;
  std::vector<int> qlens;  // one query, or a set
  qtab::Options opt;
};

inline std::vector<int8_t> matrix(const Case& c) {
  const int A = c.protein ? SW_PROTEIN_ALPHA : SW_DNA_ALPHA;
  std::vector<int8_t> m((size_t)A * A);
  sw_fill_matrix(c.protein ? SW_ALPHABET_PROTEIN : SW_ALPHABET_DNA, c.match, c.mismatch, m.data());
  if (c.odd_n) m[2 * A + 4] = -2;
  for (int a = 0; c.asym && a < 4; ++a)
    for (int b = a + 1; b < 4; ++b) m[a * A + b] = -2;
  return m;
}

// Query i of a case: LCG codes; DNA gets an N about every 31st code.
inline std::vector<uint8_t> query(const Case& c, size_t i) {
  std::vector<uint8_t> q((size_t)c.qlens[i]);
  uint32_t x = 12345u + 977u * (uint32_t)i + (uint32_t)c.qlens[i];
  for (uint8_t& v : q) {
    x = x * 1664525u + 1013904223u;
    v = c.protein ? (uint8_t)((x >> 16) % SW_PROTEIN_ALPHA)
                  : (x >> 8) % 31 == 0 ? (uint8_t)4 : (uint8_t)((x >> 24) & 3);
  }
  return q;
}

inline std::vector<Case> cases() {
  std::vector<Case> v;
  auto add = [&](std::string name, bool protein, bool gotoh, int match, int mismatch, int open,
                 int extend, std::vector<int> qlens, qtab::Options opt = qtab::Options()) {
    v.push_back({name, protein, gotoh, match, mismatch, false, false, open, extend, qlens, opt});
  };
  for (int n : {1, 16, 17, 128, 129, 257, 512, 513, 1025})
    add("dna_merged_" + std::to_string(n), false, false, 5, -4, -12, -4, {n});
  for (int n : {16, 17, 513}) add("dna_gotoh_" + std::to_string(n), false, true, 5, -4, -12, -4, {n});
  add("dna_col0_33", false, false, 3, -3, -1, -1, {33});
  add("dna_pm9_33", false, false, 9, -9, -12, -4, {33});
  add("dna_oddn_33", false, false, 5, -4, -12, -4, {33});
  v.back().odd_n = true;
  add("dna_gotoh_u16only_33", false, true, 5, -4, -2000, -100, {33});
  for (int g = 0; g < 2; ++g)
    for (int n : {1, 300, 513})
      add(std::string("blosum62_") + (g ? "gotoh_" : "merged_") + std::to_string(n), true, g != 0,
          0, 0, -11, -1, {n});
  {  // R = 32 under the column-0 rule: the u16 kernel exists, the f16 one does not
    qtab::Options o;
    o.R = 32;
    add("dna_col0_R32_nof16_33", false, false, 3, -3, -1, -1, {33}, o);
  }
  for (int rows : {128, 256, 512, 0}) {
    qtab::Options o;
    o.mq_pair = rows != 0;
    if (rows) o.mq_pair_rows = rows;
    add("dna_set_" + (rows ? "pair" + std::to_string(rows) : std::string("nopair")), false, false,
        5, -4, -12, -4, {40, 128, 300}, o);
  }
  // beyond the branch list: the DNA matrices above are symmetric in A/C/G/T, so the LUT and pair
  // tables would read the same with the matrix index transposed; these two are not
  for (int g = 0; g < 2; ++g) {
    add(g ? "dna_asym_gotoh_33" : "dna_asym_merged_33", false, g != 0, 5, -4, -12, -4, {33});
    v.back().asym = true;
  }
  add("dna_asym_set", false, false, 5, -4, -12, -4, {40, 70});
  v.back().asym = true;
  // the refusals
  add("refuse_range", false, false, 127, -128, -12, -4, {33});
  add("refuse_gotoh_penalties", false, true, 5, -4, -32767, -32767, {33});
  {
    qtab::Options o;
    o.seg = 100;
    add("refuse_seg_multiple", false, false, 5, -4, -12, -4, {513}, o);
    o.seg = 1024;
    add("refuse_seg_tall", false, false, 5, -4, -12, -4, {513}, o);
    o = qtab::Options();
    o.RB = 3;
    add("refuse_no_variant", false, false, 5, -4, -12, -4, {33}, o);
  }
  return v;
}

}  // namespace qcase

#endif  // QTAB_CASES_H
