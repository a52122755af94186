// Column-major view of a constraint system for the evaluation of the QAP at a point (mnt753_r1cs_qap_at).
// Plain host code without HIP: the library builds it on the first call, tools/host_qap_check.cpp checks it on designed systems.
//
// The matrices a, b, c lie by row (CSR); At / Bt / Ct are sums by column (r1cs_to_qap.tcc:135-153).  The view is a permutation, not a
// second copy of the coefficients: per term its row and its index into the matrix's coefficient array (8 bytes against the 112 of a
// coefficient), grouped by (matrix, column), rows ascending inside a column (a counting sort over the columns: O(terms + columns)).
// Every column is cut into chunks of at most L terms, one device thread each; the chunks are handed out by decreasing length, as the
// rows of the witness-map evaluation are (csrc/mnt753_r1cs.hip), so that the 64 chunks of a wave have the same length to within one
// wherever the lengths allow it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace mnt753 {

// Terms per chunk.  Not chosen by measurement: the constant column of a 2^20-row system holds ~1.9 M terms, 256 cuts it into ~7400
// chunks -- a chunk is then a chain of 256 products and the fold of that column a chain of ~7400 additions, the same order of time.
constexpr uint32_t QAP_CHUNK_TERMS = 256;

struct QapTranspose {
  uint32_t L = 0;
  uint64_t ncols = 0;                     // columns per matrix (num_variables + 1)
  uint64_t base[4] = {0, 0, 0, 0};        // terms of matrix k are perm[base[k] .. base[k + 1])
  std::vector<uint32_t> perm_row;         // per term, grouped by (matrix, column): the constraint row
  std::vector<uint32_t> perm_k;           //           and the index of the term in the matrix's own (row-major) arrays
  std::vector<uint64_t> chunk_start;      // per chunk, in (matrix, column) order: first term in perm
  std::vector<uint32_t> chunk_len;        //            1 .. L terms
  std::vector<uint64_t> col_chunk;        // 3 ncols + 1: the chunks of column c of matrix k are [col_chunk[k ncols + c], col_chunk[k ncols + c + 1])
  std::vector<uint32_t> order;            // the chunks by decreasing length (ties: ascending chunk id)
  uint64_t split_columns = 0;             // columns cut into more than one chunk
  uint64_t longest_column = 0;            // terms
  size_t device_bytes() const {
    return 4 * perm_row.size() + 4 * perm_k.size() + 8 * chunk_start.size() + 4 * chunk_len.size() + 8 * col_chunk.size() + 4 * order.size();
  }
};

// row_ptr[k]: nc + 1 offsets, col[k]: column of every term (< ncols).  false: a count does not fit 32 bits or an index is out of range.
inline bool qap_build_transpose(uint64_t nc, uint64_t ncols, const uint64_t* const row_ptr[3], const uint32_t* const col[3], uint32_t L,
                                QapTranspose& out) {
  out = QapTranspose();
  if (L == 0 || nc >= 0xffffffffull || ncols >= 0xffffffffull) return false;
  out.L = L;
  out.ncols = ncols;
  for (int k = 0; k < 3; ++k) {
    const uint64_t nnz = row_ptr[k][nc];
    if (nnz >= 0xffffffffull) return false;
    out.base[k + 1] = out.base[k] + nnz;
  }
  const uint64_t total = out.base[3];
  out.perm_row.resize(total);
  out.perm_k.resize(total);
  out.col_chunk.assign(3 * ncols + 1, 0);
  std::vector<uint64_t> fill(ncols + 1);
  uint64_t n_chunks = 0;
  for (int k = 0; k < 3; ++k) {
    const uint64_t nnz = row_ptr[k][nc];
    // counting sort of the matrix's terms by column; visiting the rows in order keeps them ascending inside a column
    fill.assign(ncols + 1, 0);
    for (uint64_t i = 0; i < nnz; ++i) {
      if (col[k][i] >= ncols) return false;
      ++fill[col[k][i] + 1];
    }
    for (uint64_t c = 0; c < ncols; ++c) {
      const uint64_t len = fill[c + 1];
      if (len > out.longest_column) out.longest_column = len;
      const uint64_t chunks = (len + L - 1) / L;
      if (chunks > 1) ++out.split_columns;
      out.col_chunk[k * ncols + c] = n_chunks;
      for (uint64_t j = 0; j < chunks; ++j) {
        out.chunk_start.push_back(out.base[k] + fill[c] + j * L);
        out.chunk_len.push_back((uint32_t)(j + 1 < chunks ? L : len - j * L));
      }
      n_chunks += chunks;
      fill[c + 1] += fill[c];             // fill[c] = first slot of column c
    }
    for (uint64_t row = 0; row < nc; ++row)
      for (uint64_t i = row_ptr[k][row]; i < row_ptr[k][row + 1]; ++i) {
        const uint64_t slot = out.base[k] + fill[col[k][i]]++;
        out.perm_row[slot] = (uint32_t)row;
        out.perm_k[slot] = (uint32_t)i;
      }
  }
  out.col_chunk[3 * ncols] = n_chunks;
  if (n_chunks >= 0xffffffffull) return false;
  // the chunks by decreasing length: a counting sort over the lengths 1 .. L
  std::vector<uint64_t> start(L + 2, 0);
  for (uint64_t i = 0; i < n_chunks; ++i) ++start[L - out.chunk_len[i] + 1];
  for (uint32_t l = 1; l <= L; ++l) start[l] += start[l - 1];
  out.order.resize(n_chunks);
  for (uint64_t i = 0; i < n_chunks; ++i) out.order[start[L - out.chunk_len[i]]++] = (uint32_t)i;
  return true;
}

}  // namespace mnt753
