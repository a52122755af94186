// mint_compress.cpp -- mints libff's COMPRESSED point streams (TEST INFRASTRUCTURE; tools/mint_compress.sh compiles and runs it).
//
// OUR program, compiled against the REFERENCE's own libff where it lies, with the flags of oracle/build_ref.sh EXCEPT
// NO_PT_COMPRESSION: the group files are compiled a second time without that define (tools/mint_compress.sh), so operator<< and
// operator>> of the four groups are libff's default, compressed ones (mnt4753_g1.cpp:389-450, mnt4753_g2.cpp:419-460 and the two
// mnt6753 files).  Nothing in it is this repository's arithmetic.
//
//   mint_compress <out_dir> <g16_mnt4/full.bin> <g16_mnt6/full.bin>
//
// Writes into <out_dir>, per group <g> of mnt4_g1, mnt4_g2, mnt6_g1, mnt6_g2:
//   <g>/points.bin   16 points in uncompressed wire words (write_g1 / write_g2 of libsnark/serialization.hpp): k G for k = 1 .. 15 with
//                    the identity in the sixth place; the program fails unless both parities of y occur
//   <g>/stream.bin   operator<< of the same points, back to back; read back with operator>> and compared
// and per curve mnt{4,6}/proof_stream.bin: operator<< of A, B, C of the proof in full.bin (what r1cs_gg_ppzksnark_proof::operator<<
// writes where OUTPUT_NEWLINE is empty: the three records back to back).
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include <libsnark/serialization.hpp>

static FILE* open_or_die(const std::string& p, const char* mode) {
  FILE* f = fopen(p.c_str(), mode);
  if (!f) { perror(p.c_str()); exit(1); }
  return f;
}
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "mint_compress: expectation failed: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static void write_bytes(const std::string& path, const std::string& bytes) {
  FILE* f = open_or_die(path, "wb");
  fwrite(bytes.data(), 1, bytes.size(), f);
  fclose(f);
}

template <typename G>
static unsigned parity_of(const G& g);
template <> unsigned parity_of(const mnt4753_G1& g) { mnt4753_G1 c(g); c.to_affine_coordinates(); return c.Y().as_bigint().data[0] & 1; }
template <> unsigned parity_of(const mnt6753_G1& g) { mnt6753_G1 c(g); c.to_affine_coordinates(); return c.Y().as_bigint().data[0] & 1; }
template <> unsigned parity_of(const mnt4753_G2& g) { mnt4753_G2 c(g); c.to_affine_coordinates(); return c.Y().c0.as_bigint().data[0] & 1; }
template <> unsigned parity_of(const mnt6753_G2& g) { mnt6753_G2 c(g); c.to_affine_coordinates(); return c.Y().c0.as_bigint().data[0] & 1; }

template <typename ppT, typename G, void (*WRITE)(FILE*, G)>
static void mint_group(const std::string& dir, size_t record) {
  std::vector<G> pts;
  G acc = G::zero();
  unsigned seen[2] = {0, 0};
  for (int k = 1; k <= 15; ++k) {
    acc = acc + G::one();
    if (k == 6) pts.push_back(G::zero());
    pts.push_back(acc);
    ++seen[parity_of<G>(acc)];
  }
  REQUIRE(pts.size() == 16 && seen[0] > 0 && seen[1] > 0, "%s: both parities of y among the multiples (%u even, %u odd)", dir.c_str(), seen[0], seen[1]);
  FILE* f = open_or_die(dir + "/points.bin", "wb");
  for (const G& p : pts) WRITE(f, p);
  fclose(f);
  std::ostringstream out;
  for (const G& p : pts) out << p;
  const std::string bytes = out.str();
  REQUIRE(bytes.size() == record * pts.size(), "%s: %zu bytes per record expected, stream has %zu for %zu points", dir.c_str(), record, bytes.size(), pts.size());
  std::istringstream in(bytes);
  for (const G& p : pts) {
    G back;
    in >> back;
    REQUIRE(back == p, "%s: operator>> does not give back what operator<< wrote", dir.c_str());
  }
  write_bytes(dir + "/stream.bin", bytes);
  printf("%s: 16 points, %u even, %u odd, %zu stream bytes\n", dir.c_str(), seen[0], seen[1], bytes.size());
}

template <typename ppT>
static void mint_proof(const std::string& full_bin, const std::string& out_path, size_t want) {
  FILE* f = open_or_die(full_bin, "rb");
  const G1<ppT> A = read_g1<ppT>(f);
  const G2<ppT> B = read_g2<ppT>(f);
  const G1<ppT> C = read_g1<ppT>(f);
  fclose(f);
  REQUIRE(A.is_well_formed() && B.is_well_formed() && C.is_well_formed(), "%s: a point of the proof is off its curve", full_bin.c_str());
  std::ostringstream out;
  out << A << B << C;
  const std::string bytes = out.str();
  REQUIRE(bytes.size() == want, "%s: %zu bytes expected, got %zu", out_path.c_str(), want, bytes.size());
  std::istringstream in(bytes);
  G1<ppT> a, c;
  G2<ppT> b;
  in >> a >> b >> c;
  REQUIRE(a == A && b == B && c == C, "%s: the proof does not survive the round trip", out_path.c_str());
  write_bytes(out_path, bytes);
  printf("%s: %zu bytes\n", out_path.c_str(), bytes.size());
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: mint_compress <out_dir> <g16_mnt4/full.bin> <g16_mnt6/full.bin>\n"); return 2; }
  const std::string out = argv[1];
  libff::inhibit_profiling_info = true;
  mnt4753_pp::init_public_params();
  mnt6753_pp::init_public_params();
  mint_group<mnt4753_pp, mnt4753_G1, write_g1<mnt4753_pp>>(out + "/mnt4_g1", 98);
  mint_group<mnt4753_pp, mnt4753_G2, write_g2<mnt4753_pp>>(out + "/mnt4_g2", 194);
  mint_group<mnt6753_pp, mnt6753_G1, write_g1<mnt6753_pp>>(out + "/mnt6_g1", 98);
  mint_group<mnt6753_pp, mnt6753_G2, write_g2<mnt6753_pp>>(out + "/mnt6_g2", 290);
  mint_proof<mnt4753_pp>(argv[2], out + "/mnt4/proof_stream.bin", 390);
  mint_proof<mnt6753_pp>(argv[3], out + "/mnt6/proof_stream.bin", 486);
  return 0;
}
