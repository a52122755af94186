// What main.cpp's commands share below the wrapper: the file helpers, the constraint-system file, and owners for the handles of
// the C ABI.  Included by main.cpp only.
#pragma once

#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mnt753_hip.h"

// The file helpers report on stderr as "main_hip: <text>" with the text their caller hands them, and return false; the caller
// chooses the exit code.
static bool refuse(const std::string& text) { fprintf(stderr, "main_hip: %s\n", text.c_str()); return false; }

// exactly `bytes` from the start of the file; refuse_longer: a file that goes on behind them is of the wrong size as well
static bool read_exact(const char* path, void* dst, size_t bytes, bool refuse_longer, const std::string& cannot_open, const std::string& wrong_size) {
  FILE* f = fopen(path, "rb");
  if (!f) return refuse(cannot_open);
  const bool ok = fread(dst, 1, bytes, f) == bytes && !(refuse_longer && fgetc(f) != EOF);
  fclose(f);
  return ok || refuse(wrong_size);
}

// the last `bytes` of the file
static bool read_tail(const char* path, void* dst, size_t bytes, const std::string& cannot_open, const std::string& cannot_seek, const std::string& too_short) {
  FILE* f = fopen(path, "rb");
  if (!f) return refuse(cannot_open);
  if (fseek(f, -(long)bytes, SEEK_END) != 0) { fclose(f); return refuse(cannot_seek); }
  const bool ok = fread(dst, 1, bytes, f) == bytes;
  fclose(f);
  return ok || refuse(too_short);
}

// the whole file, which holds u64 words
static bool read_words(const char* path, std::vector<uint64_t>& out, const std::string& cannot_open, const std::string& not_words) {
  FILE* f = fopen(path, "rb");
  if (!f) return refuse(cannot_open);
  uint64_t buf[4096];
  size_t got;
  out.clear();
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) {
    if (got % 8) { fclose(f); return refuse(not_words); }
    out.insert(out.end(), buf, buf + got / 8);
  }
  fclose(f);
  return true;
}

// the parts (pointer, bytes) one behind the other into a new file
static bool write_file(const std::string& path, const std::vector<std::pair<const void*, size_t>>& parts, const std::string& cannot_open, const std::string& cannot_write) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return refuse(cannot_open);
  bool ok = true;
  for (auto& p : parts) ok = ok && fwrite(p.first, 1, p.second, f) == p.second;
  return (fclose(f) == 0 && ok) || refuse(cannot_write);
}

// r1cs.bin: u64 num_inputs, m, nc; per matrix a, b, c: u64 row_ptr[nc + 1], u32 col[nnz], Fr coeff[nnz]
struct R1csFile {
  uint64_t head[3] = {0, 0, 0};
  std::vector<uint64_t> rp[3], cf[3];
  std::vector<uint32_t> col[3];
  bool load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "main_hip: cannot open %s\n", path); return false; }
    bool ok = fread(head, 8, 3, f) == 3 && head[2] < ((uint64_t)1 << 40);
    for (int k = 0; ok && k < 3; ++k) {
      rp[k].resize(head[2] + 1);
      ok = fread(rp[k].data(), 8, rp[k].size(), f) == rp[k].size() && rp[k][head[2]] < ((uint64_t)1 << 40);
      if (!ok) break;
      const size_t nnz = rp[k][head[2]];
      col[k].resize(nnz + 1); cf[k].resize(12 * nnz + 12);
      ok = fread(col[k].data(), 4, nnz, f) == nnz && fread(cf[k].data(), 96, nnz, f) == nnz;
    }
    fclose(f);
    if (!ok) fprintf(stderr, "main_hip: %s is not a constraint-system file\n", path);
    return ok;
  }
  // the same layout, the matrices in the order given (1, 0, 2: a and b exchanged)
  bool store(const char* path, const int order[3]) const {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    bool ok = fwrite(head, 8, 3, f) == 3;
    for (int j = 0; ok && j < 3; ++j) {
      const int k = order[j];
      const size_t nnz = rp[k][head[2]];
      ok = fwrite(rp[k].data(), 8, rp[k].size(), f) == rp[k].size() && fwrite(col[k].data(), 4, nnz, f) == nnz && fwrite(cf[k].data(), 96, nnz, f) == nnz;
    }
    return (fclose(f) == 0) && ok;
  }
};

// Owners for what the C ABI hands out: released on every way out of the scope, return or throw.
struct AbiRelease {
  void operator()(mnt753_r1cs* p) const { mnt753_r1cs_free(p); }
  void operator()(mnt753_domain* p) const { mnt753_domain_free(p); }
  void operator()(mnt753_vk* p) const { mnt753_vk_destroy(p); }
};
struct DevRelease { void operator()(void* p) const { mnt753_dev_free(p); } };
typedef std::unique_ptr<mnt753_r1cs, AbiRelease> R1csHandle;
typedef std::unique_ptr<mnt753_domain, AbiRelease> DomainHandle;
typedef std::unique_ptr<mnt753_vk, AbiRelease> VkHandle;
typedef std::unique_ptr<void, DevRelease> DevMem;
