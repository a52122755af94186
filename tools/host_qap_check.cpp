// host_qap_check.cpp -- the column-major view of mnt753_r1cs_qap_at (csrc/qap_transpose.hpp) on designed systems, without a device.
// Stand-alone (its own main); tests/test_qap_cpu.py compiles it plain and under ASan + UBSan and runs it directly.
//
// Checked on every system, for L = 4 and for the library's chunk length:
//   * the chunks of a column partition that column's terms: every term of the matrix is named exactly once, by a chunk of its own
//     (matrix, column), rows ascending inside a column;
//   * no chunk is empty or longer than L, and only the last chunk of a column is shorter than L;
//   * the work list is a permutation of the chunks by non-increasing length;
//   * the counts of the plan (split columns, longest column).
// Systems: empty matrices, a single term, all terms in one column, columns of L - 1, L, L + 1 and 2 L + 1 terms, duplicate (row, col)
// pairs, a seeded ragged system.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../snark-challenge-prover-reference_amd/csrc/qap_transpose.hpp"

using namespace mnt753;

struct System {
  const char* name;
  uint64_t nc, ncols;
  std::vector<uint64_t> rp[3];
  std::vector<uint32_t> col[3];
};

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s L=%u: ", s.name, L); printf(__VA_ARGS__); printf("\n"); ++g_fail; return; } } while (0)

static void check(const System& s, uint32_t L) {
  const uint64_t* rpp[3] = {s.rp[0].data(), s.rp[1].data(), s.rp[2].data()};
  const uint32_t* cp[3] = {s.col[0].data(), s.col[1].data(), s.col[2].data()};
  QapTranspose t;
  CHECK(qap_build_transpose(s.nc, s.ncols, rpp, cp, L, t), "builder refused");
  const uint64_t total = s.rp[0][s.nc] + s.rp[1][s.nc] + s.rp[2][s.nc];
  CHECK(t.base[3] == total && t.perm_row.size() == total && t.perm_k.size() == total, "term count");
  CHECK(t.col_chunk.size() == 3 * s.ncols + 1, "col_chunk size");
  const uint64_t n_chunks = t.chunk_len.size();
  CHECK(t.chunk_start.size() == n_chunks && t.order.size() == n_chunks && t.col_chunk[3 * s.ncols] == n_chunks, "chunk count");
  std::vector<std::vector<uint8_t>> seen(3);
  for (int k = 0; k < 3; ++k) seen[k].assign(s.rp[k][s.nc], 0);
  // the row of every term, from the row-major arrays
  std::vector<std::vector<uint32_t>> row_of(3);
  for (int k = 0; k < 3; ++k) {
    row_of[k].resize(s.rp[k][s.nc]);
    for (uint64_t r = 0; r < s.nc; ++r) for (uint64_t i = s.rp[k][r]; i < s.rp[k][r + 1]; ++i) row_of[k][i] = (uint32_t)r;
  }
  uint64_t split = 0, longest = 0, expect_start = 0;
  for (int k = 0; k < 3; ++k) {
    for (uint64_t c = 0; c < s.ncols; ++c) {
      const uint64_t lo = t.col_chunk[k * s.ncols + c], hi = t.col_chunk[k * s.ncols + c + 1];
      CHECK(lo <= hi && hi <= n_chunks, "chunk range of matrix %d column %llu", k, (unsigned long long)c);
      uint64_t terms = 0;
      uint32_t prev_row = 0;
      for (uint64_t j = lo; j < hi; ++j) {
        CHECK(t.chunk_len[j] >= 1 && t.chunk_len[j] <= L, "chunk %llu has %u terms", (unsigned long long)j, t.chunk_len[j]);
        CHECK(j + 1 == hi || t.chunk_len[j] == L, "an inner chunk is short");
        CHECK(t.chunk_start[j] == expect_start, "chunk %llu does not follow its predecessor", (unsigned long long)j);
        CHECK(t.chunk_start[j] >= t.base[k] && t.chunk_start[j] + t.chunk_len[j] <= t.base[k + 1], "chunk outside its matrix");
        for (uint64_t p = t.chunk_start[j]; p < t.chunk_start[j] + t.chunk_len[j]; ++p) {
          const uint32_t term = t.perm_k[p];
          CHECK(term < seen[k].size(), "term index out of range");
          CHECK(!seen[k][term], "term named twice");
          seen[k][term] = 1;
          CHECK(s.col[k][term] == c, "term in the wrong column");
          CHECK(t.perm_row[p] == row_of[k][term], "row of a term");
          CHECK(terms == 0 || t.perm_row[p] >= prev_row, "rows not ascending inside a column");
          prev_row = t.perm_row[p];
          ++terms;
        }
        expect_start += t.chunk_len[j];
      }
      if (hi - lo > 1) ++split;
      if (terms > longest) longest = terms;
    }
    for (uint8_t v : seen[k]) CHECK(v, "a term of matrix %d is in no chunk", k);
  }
  CHECK(expect_start == total, "chunks do not cover the permutation");
  CHECK(split == t.split_columns && longest == t.longest_column, "plan counts");
  std::vector<uint8_t> listed(n_chunks, 0);
  for (uint64_t i = 0; i < n_chunks; ++i) {
    CHECK(t.order[i] < n_chunks && !listed[t.order[i]], "work list is not a permutation");
    listed[t.order[i]] = 1;
    CHECK(i == 0 || t.chunk_len[t.order[i]] <= t.chunk_len[t.order[i - 1]], "work list not by decreasing length");
  }
}

// a system from (matrix, row, column) triples given in row order
static System make(const char* name, uint64_t nc, uint64_t ncols, const std::vector<std::vector<std::pair<uint32_t, uint32_t>>>& terms) {
  System s;
  s.name = name; s.nc = nc; s.ncols = ncols;
  for (int k = 0; k < 3; ++k) {
    s.rp[k].assign(nc + 1, 0);
    for (auto& t : terms[k]) ++s.rp[k][t.first + 1];
    for (uint64_t r = 0; r < nc; ++r) s.rp[k][r + 1] += s.rp[k][r];
    std::vector<uint64_t> at(s.rp[k].begin(), s.rp[k].end() - 1);
    s.col[k].assign(terms[k].size() + 1, 0);      // (+1: data() of an empty vector may be null)
    for (auto& t : terms[k]) s.col[k][at[t.first]++] = t.second;
  }
  return s;
}

int main() {
  typedef std::vector<std::pair<uint32_t, uint32_t>> T;
  int systems = 0;
  for (uint32_t L : {4u, QAP_CHUNK_TERMS}) {
    std::vector<System> all;
    all.push_back(make("empty matrices", 5, 7, {T{}, T{}, T{}}));
    all.push_back(make("no constraints", 0, 3, {T{}, T{}, T{}}));
    all.push_back(make("a single term", 3, 4, {T{}, T{{1, 2}}, T{}}));
    {
      T one;
      for (uint32_t r = 0; r < 3 * L + 2; ++r) one.push_back({r, 0});
      all.push_back(make("all terms in one column", 3 * L + 2, 5, {one, T{}, one}));
    }
    {
      // columns 1 .. 4 of matrix a hold L - 1, L, L + 1 and 2 L + 1 terms; b holds duplicates of (row, col); c is ragged
      const uint32_t want[4] = {L - 1, L, L + 1, 2 * L + 1};
      const uint32_t nc = 2 * L + 1;
      T a, b, c;
      for (uint32_t r = 0; r < nc; ++r) {
        for (uint32_t j = 0; j < 4; ++j) if (r < want[j]) a.push_back({r, j + 1});
        b.push_back({r, 2}); b.push_back({r, 2}); b.push_back({r, r % 3});
        if (r % 2) b.push_back({r, r % 3});
      }
      uint64_t x = 0x9e3779b97f4a7c15ull;
      for (uint32_t r = 0; r < nc; ++r) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        for (uint32_t j = 0; j < x % 10; ++j) c.push_back({r, (uint32_t)((x >> (8 + 4 * j)) % 6)});
      }
      all.push_back(make("designed column lengths, duplicates, ragged", nc, 6, {a, b, c}));
    }
    for (const System& s : all) { check(s, L); ++systems; }
  }
  // refusals: a column index out of range, a chunk length of zero
  {
    System s = make("bad column", 2, 3, {T{{0, 1}}, T{}, T{}});
    s.col[0][0] = 3;
    const uint64_t* rpp[3] = {s.rp[0].data(), s.rp[1].data(), s.rp[2].data()};
    const uint32_t* cp[3] = {s.col[0].data(), s.col[1].data(), s.col[2].data()};
    QapTranspose t;
    if (qap_build_transpose(s.nc, s.ncols, rpp, cp, 4, t)) { printf("FAIL: a column out of range was accepted\n"); ++g_fail; }
    s.col[0][0] = 1;
    if (qap_build_transpose(s.nc, s.ncols, rpp, cp, 0, t)) { printf("FAIL: L = 0 was accepted\n"); ++g_fail; }
  }
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK: %d systems\n", systems);
  return 0;
}
